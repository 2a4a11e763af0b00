#!/bin/bash
# tools/build_codec_variant.sh NAME "-DFLAG=..." -- libkbbq_engine.so with the device I/O units (io_common.hip: k_inflate;
# bgzf_writer.hip: k_deflate; the readers, which share io_common.h's structs with them) compiled with extra flags, as
# tools/build/libkbbq_NAME.so (the other objects are the tree's own: run `make -C kbbq_amd/csrc` first).  For A/B runs of the
# codec kernels through KBBQ_LIB (tools/inflate_variants.sh, tools/deflate_variants.sh).
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
name=$1; shift
mkdir -p $R/tools/build
cd $R/kbbq_amd/csrc
objs=
for u in io_common bgzf_writer fastq_reader gzip_stream bam_reader; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-function -Wno-unused-value -Wno-unused-result -ffp-contract=off "$@" \
        -c -o $R/tools/build/${u}_$name.o $u.hip
    objs="$objs $R/tools/build/${u}_$name.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/tools/build/libkbbq_$name.so engine.o host_model.o $objs bgzf_host.o exchange.o -lpthread -ldl
rm -f $objs
echo built tools/build/libkbbq_$name.so
