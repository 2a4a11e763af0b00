#!/bin/bash
# tools/round_profile.sh TAG [ROUND] -- the round's profiler record for HEAD at full scale (BASELINE configs[1]); ROUND = file prefix (default r04):
# in $KBBQ_OUT (default out/):
#   ${rnd}_bench_driver_TAG.json        python bench.py --full --gpus 1 --steps 20 --warmup 5 (the driver's command, with the roofline)
#   ${rnd}_kernel_stats_TAG.csv         rocprofv3 --kernel-trace --stats of one step of the same command
#   ${rnd}_kernel_stats_inorder_TAG.csv the same with KBBQ_NO_OVERLAP=1 (exclusive durations)
#   ${rnd}_pmc_TAG_summary.txt          rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes) of one in-order 3e8-genome step
#   ${rnd}_pmc_latest_TAG.json          the same as the JSON bench.py quotes (copy to profiles/${rnd}_pmc_latest.json)
set -o pipefail
tag=$1
rnd=${2:-r04}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${KBBQ_OUT:-$R/out}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof$tag -o ${rnd} -- python3 $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-pcie --no-exclusive-step > $OUT/prof$tag.json 2> $OUT/prof$tag.log || { tail -5 $OUT/prof$tag.log; exit 1; }
find $OUT/prof$tag -name "*kernel_stats.csv" -exec cp {} $OUT/${rnd}_kernel_stats_$tag.csv \;
rm -rf $OUT/prof$tag
echo "profile done"
# the same with every kernel in order on one stream: the exclusive durations the roofline object quotes
KBBQ_NO_OVERLAP=1 timeout -k 10 420 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/profi$tag -o ${rnd} -- python3 $R/bench.py --steps 1 --warmup 0 --no-cpu-baseline --no-pcie --no-exclusive-step > $OUT/profi$tag.json 2> $OUT/profi$tag.log || { tail -5 $OUT/profi$tag.log; exit 1; }
find $OUT/profi$tag -name "*kernel_stats.csv" -exec cp {} $OUT/${rnd}_kernel_stats_inorder_$tag.csv \;
rm -rf $OUT/profi$tag
echo "in-order profile done"
export KBBQ_NO_OVERLAP=1
for c in FETCH_SIZE WRITE_SIZE; do
    timeout -k 10 400 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc${tag}_$c -- \
        python3 $R/bench.py --genome-len 300000000 --steps 1 --warmup 0 --no-cpu-baseline --no-pcie --no-exclusive-step > $OUT/pmc${tag}_$c.log 2>&1 || { tail -5 $OUT/pmc${tag}_$c.log; exit 1; }
    echo "$c done"
done
unset KBBQ_NO_OVERLAP
python3 $R/tools/pmc_summary.py $OUT/pmc${tag}_FETCH_SIZE $OUT/pmc${tag}_WRITE_SIZE > $OUT/${rnd}_pmc_${tag}_summary.txt
rm -rf $OUT/pmc${tag}_FETCH_SIZE $OUT/pmc${tag}_WRITE_SIZE
(cd $R && python3 tools/pmc_json.py $OUT/${rnd}_pmc_${tag}_summary.txt $OUT/${rnd}_pmc_latest_$tag.json profiles/${rnd}_pmc_fetch_write_$tag.txt)
echo "pmc done"
cd $R
timeout -k 10 600 python $R/bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${rnd}_bench_driver_$tag.json 2> $OUT/${rnd}_bench_driver_$tag.log || { tail -5 $OUT/${rnd}_bench_driver_$tag.log; exit 1; }
python3 -c "
import json
d=json.loads(open('$OUT/${rnd}_bench_driver_$tag.json').read().strip().splitlines()[-1])
print('driver-like', d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['avg_launch_ms'], d['roofline']['traffic'])"
