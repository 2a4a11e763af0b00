#!/bin/bash
# tools/e2e_sam.sh TAG [GENOME_LEN] -- SAM text end to end beside its BAM twin: the bench's own reads (30x of GENOME_LEN) written
# as a BAM file (kbbq --io-test synth-bam) and as the SAM lines whose twins those records are (synth-sam), each recalibrated by
# `kbbq` with KBBQ_TIMING=1 KBBQ_QUAL_DIGEST=1.  The two digests -- the trusted k-mers inserted and the sum of the recalibrated
# qualities -- must agree; the timing lines of both runs (scan wall time, the reader's index + pack kernels, the writer's format
# kernel) stand side by side in the log.  Every step has its own time limit, and a step that fails ends the script.
# Log: $KBBQ_OUT (default out/) /e2e_sam_TAG.log
set -o pipefail
tag=${1:-a}; G=${2:-100000000}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${KBBQ_OUT:-$R/out}
D=$(mktemp -d "${TMPDIR:-/tmp}/kbbq_e2e_sam.XXXXXX") || exit 1
trap 'rm -rf "$D"' EXIT
L=$OUT/e2e_sam_$tag.log
mkdir -p $OUT
: > $L
K=$R/kbbq_amd/kbbq
run() {   # name, input
    local s=$(date +%s%N)
    KBBQ_TIMING=1 KBBQ_QUAL_DIGEST=1 KBBQ_SEED=12345 timeout -k 10 ${E2E_LIMIT:-900} $K $2 2> $D/err_$1.txt | wc -c > $D/out_$1.bytes || return 1
    local e=$(date +%s%N)
    echo "== $1 wall_ms $(( (e - s) / 1000000 )) in_bytes $(stat -c %s $2) out_bytes $(cat $D/out_$1.bytes)" | tee -a $L
    grep -E "timing|digest|Error" $D/err_$1.txt | sed 's/^/   /' | tee -a $L
    grep digest $D/err_$1.txt > $D/digest_$1.txt
}
df -h $D | tail -1 >> $L
timeout -k 10 600 $K --io-test synth-bam $G 30 > $D/in.bam 2>> $L &&
timeout -k 10 600 $K --io-test synth-sam $G 30 > $D/in.sam.gz 2>> $L &&
run bam $D/in.bam &&
run sam $D/in.sam.gz &&
[ -s $D/digest_bam.txt ] && cmp -s $D/digest_bam.txt $D/digest_sam.txt || { echo "A STEP FAILED OR THE DIGESTS DIFFER" | tee -a $L; exit 1; }
echo "digests agree" | tee -a $L
