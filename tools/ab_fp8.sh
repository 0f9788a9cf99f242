#!/bin/bash
# A/B (mode fp8): the 1 - 4 row token step streaming the e4m3 copies (csrc/gemv_fp8.hip, options fp8_weights / fp8_chain, ASRModel(mode="fp8")) against
# the default chain, and the snapped model on the default chains in between (fp8_chain=0: what the snap alone costs or buys - nothing is expected).
# B = 1 call shape (ASRModel.transcribe of 5 s / 75 tokens and 20 s / 150 tokens, one at a time) and 16 streaming sessions; one MI355X, full dims, alternating runs, p50 in ms.
#   tools/ab_fp8.sh [REPS] [PARENT_TREE]    PARENT_TREE: a built checkout of the parent commit - its default variant then runs beside this tree's in every repeat
#                                           ("option off is the parent's step": the two must differ by less than the repeats do)
# Writes profiles/fp8_ab.txt (and prints it).  Every run has a time limit of its own, and the first run that fails ends the script.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
reps=${1:-2}; parent=$2
out=profiles/fp8_ab.txt
one() {   # one TREE LABEL [bench options]: one bench run in TREE, one line
  local tree=$1 label=$2; shift 2
  (cd "$tree" && timeout -k 10 420 python bench.py --streaming --sessions 16 --ingest ring --slots 2 --continuous --single --opt decode_chunk=2 "$@" 2>/dev/null) | tail -1 | python3 -c "
import json,sys
d=json.loads(sys.stdin.read()); print('[$label]', 'single_5s', round(d['single_5s']['latency_ms']['p50'],1), 'single_20s', round(d['single_20s']['latency_ms']['p50'],1), 'partial p50', round(d['partial_latency_ms']['p50'],1), 'final p50/p99', round(d['final_latency_ms']['p50'],1), round(d['final_latency_ms']['p99'],1))"
}
{
echo "# tools/ab_fp8.sh $reps${parent:+ <parent tree>}: bench.py --streaming --sessions 16 --ingest ring --slots 2 --continuous --single --opt decode_chunk=2, one MI355X, full dims, p50 in ms"
for rep in $(seq "$reps"); do
  if [ -n "$parent" ]; then one "$parent" "parent, default" || exit 1; fi
  one . "default" || exit 1
  one . "fp8_weights=1 fp8_chain=0" --opt fp8_weights=1 --opt fp8_chain=0 || exit 1
  one . "fp8_weights=1" --opt fp8_weights=1 || exit 1
done
} | tee "$out"
