#!/bin/bash
# A/B: per-token log-probabilities (option token_logprobs: greedy_kernel<T, true> in every decode step, csrc/greedy.hip) against the
# default engine.  `python bench.py` with and without `--opt token_logprobs=1`, alternating, two repetitions on one MI355X; the headline (segments/s)
# and ms_per_step of every run go to profiles/token_logprobs_ab.txt.  Arguments are handed to bench.py (e.g. --gpus 1 --steps 20 --warmup 3).
# The first run that fails - a non-zero status of bench.py, its time limit, or a result line that does not parse - ends the script: nothing more is
# started on the card.  bench.py's stderr of the run in hand is kept in profiles/token_logprobs_ab.stderr.txt (not committed).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
out=profiles/token_logprobs_ab.txt
errlog=profiles/token_logprobs_ab.stderr.txt
{
  echo "# tools/ab_token_logprobs.sh $*: python bench.py $* [--opt token_logprobs=1], alternating, two repetitions"
  echo "# columns: variant | headline 20s-segments/s | ms_per_step"
} > "$out"
for rep in 1 2; do
for v in "" "--opt token_logprobs=1"; do
  line=$(timeout -k 10 900 python bench.py "$@" $v 2> "$errlog" | tail -1)
  st=$?
  if [ $st -ne 0 ]; then echo "bench.py $* $v ended with status $st: stopping (stderr in $errlog)" | tee -a "$out"; exit $st; fi
  printf '%s\n' "$line" | python3 -c "
import json,sys
d=json.loads(sys.stdin.read())
print('[${v:-default}]', '|', round(d['value'],2), '|', round(d['ms_per_step'],3))" | tee -a "$out"
  st=$?
  if [ $st -ne 0 ]; then echo "bench.py $* $v printed no result line: stopping (stderr in $errlog)" | tee -a "$out"; exit $st; fi
done
done
