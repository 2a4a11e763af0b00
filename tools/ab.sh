#!/bin/bash
# tools/ab.sh TAG -- GPU parity suite, then the 1/10-scale bench of the library in the tree (--full: the line tools/ab_show.py
# reads); results in $KBBQ_OUT (default out/): ab_TAG.json
set -o pipefail
tag=$1
OUT=${KBBQ_OUT:-out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q 2>&1 | tee $OUT/gpu_tests_$tag.log | tail -4 || exit 1
timeout -k 10 200 python bench.py --full --genome-len 300000000 --no-cpu-baseline --steps 2 > $OUT/ab_$tag.json 2> $OUT/ab_$tag.log
echo bench rc $?
