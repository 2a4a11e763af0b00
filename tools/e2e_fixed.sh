#!/bin/bash
# tools/e2e_fixed.sh TAG [GENOME_LEN] [OTHER_KBBQ] [FORMAT] -- `kbbq --fixed` end to end on the bench's own reads as a file
# (kbbq --io-test synth-fastq | synth-bam | synth-sam, 30x of GENOME_LEN; FORMAT fastq -- the default -- bam or sam) with a
# differently stored copy of it as the corrected file (no errors: fine for timing) -- FASTQ and SAM: the uncompressed text;
# BAM: the same stream deflated again by the host writer (kbbq --io-test bgzf), whose blocks have other sizes, so the
# pieces of the two files end at other records.  Both files on the GPU (the default), the host loop (KBBQ_DEVICE_READER=0:
# tally_fixed over the host parsers), and -- OTHER_KBBQ given ("" to skip) -- another build of the command line, e.g. the
# commit before, on the same files.  Per-phase split (KBBQ_TIMING=1), wall time, and the md5 of every decompressed output,
# which must agree.  Every run has its own time limit.
# Log: $KBBQ_OUT (default out/) /e2e_fixed_TAG.log
set -o pipefail
tag=${1:-a}; G=${2:-100000000}; other=$3; fmt=${4:-fastq}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${KBBQ_OUT:-$R/out}
D=$(mktemp -d "${TMPDIR:-/tmp}/kbbq_e2e_fixed.XXXXXX") || exit 1
trap 'rm -rf "$D"' EXIT
L=$OUT/e2e_fixed_$tag.log
mkdir -p $OUT
: > $L
df -h $D | tail -1 >> $L
case $fmt in
    fastq) in=$D/in.fq.gz; fixed=$D/fixed.fq ;;
    bam) in=$D/in.bam; fixed=$D/fixed.bam ;;
    sam) in=$D/in.sam.gz; fixed=$D/fixed.sam ;;
    *) echo "format $fmt: fastq, bam or sam"; exit 2 ;;
esac
timeout -k 10 600 $R/kbbq_amd/kbbq --io-test synth-$fmt $G 30 > $in 2>> $L || { echo "generating the input failed" | tee -a $L; exit 1; }
if [ $fmt = bam ]; then gzip -dc $in | timeout -k 10 600 $R/kbbq_amd/kbbq --io-test bgzf 16 > $fixed || exit 1
else gzip -dc $in > $fixed || exit 1; fi
echo "format $fmt: $(basename $in) $(stat -c %s $in) bytes, $(basename $fixed) $(stat -c %s $fixed) bytes" | tee -a $L
sums=""
run() {   # name, binary, env...
    local name=$1 bin=$2; shift 2
    local s=$(date +%s%N)
    env "$@" KBBQ_TIMING=1 timeout -k 10 ${E2E_LIMIT:-900} $bin --fixed $fixed $in 2> $D/err_$name.txt | tee >(wc -c > $D/out_$name.bytes) | gzip -dc | md5sum > $D/out_$name.md5
    local rc=$?
    local e=$(date +%s%N)
    echo "== $name wall_ms $(( (e - s) / 1000000 )) rc $rc out_bytes $(cat $D/out_$name.bytes) md5 $(cut -c1-32 $D/out_$name.md5)" | tee -a $L
    grep -E "timing|Error" $D/err_$name.txt | sed 's/^/   /' | tee -a $L
    [ $rc -eq 0 ] || exit $rc      # (a run that failed or ran into its limit ends the script: nothing more is started)
    sums="$sums $(cut -c1-32 $D/out_$name.md5)"
}
[ -n "$other" ] && run other $other
run device $R/kbbq_amd/kbbq
run host_loop $R/kbbq_amd/kbbq KBBQ_DEVICE_READER=0
[ $(echo $sums | tr ' ' '\n' | sort -u | wc -l) -eq 1 ] || { echo "OUTPUTS DIFFER" | tee -a $L; exit 1; }
echo "outputs agree" | tee -a $L
