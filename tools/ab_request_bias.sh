#!/bin/bash
# A/B: option request_bias (greedy_kernel<T, LP, true, true>, csrc/greedy.hip) against the default engine.  `python bench.py` for the parent
# commit, this tree untouched and this tree with --opt request_bias=1, back to back on one MI355X; the headline (segments/s) and ms_per_step of every run go
# to profiles/request_bias_ab.txt.  Arguments are handed to bench.py (e.g. --gpus 1 --no-extras --no-cpu-baseline).
#   AB_PARENT=<dir>  a built checkout of the parent commit: its `python bench.py` runs first in every repetition, as the control of "off did not move"
#   AB_REPS=<n>      repetitions (default 3)
#   AB_OUT=<file>    the result file (default profiles/request_bias_ab.txt)
# The "on" leg: bench.py's headline is the bulk pipeline, which carries no per-request tables, and --opt passes integers, so the tables come from the
# measurement option request_bias_fill=32: every request gets 32 length-1 entries of bias +0.0 on ids spread over the vocabulary.  The tokens stay the
# unbiased ones (the workload does not change), the kernel does the full work of a 32-entry table: prologue, 32 bits in the "biased" map, a list scan at each.
# The first run that fails - a non-zero status of bench.py, its time limit, or a result line that does not parse - ends the script: nothing more is started
# on the card.  bench.py's stderr of the run in hand is kept beside the result file (*.stderr.txt, not committed).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
root=$PWD
out=${AB_OUT:-profiles/request_bias_ab.txt}
case "$out" in /*) ;; *) out=$root/$out ;; esac
errlog=${out%.txt}.stderr.txt
reps=${AB_REPS:-3}
on="--opt request_bias=1 --opt request_bias_fill=32"
variants=(off on)
[ -n "$AB_PARENT" ] && variants=(parent off on)
{
  echo "# tools/ab_request_bias.sh $*: python bench.py $* on one MI355X, back to back, $reps repetition(s):"
  [ -n "$AB_PARENT" ] && echo "#   [parent] the parent commit (its library built from its own sources in a checkout of its own)"
  echo "#   [off]    this tree untouched"
  echo "#   [on]     this tree, $on (a 32-entry table of neutral biases per request)"
  echo "# columns: variant | repetition | headline 20s-segments/s | ms_per_step"
} > "$out"
for rep in $(seq 1 "$reps"); do
for v in "${variants[@]}"; do
  dir=$root; extra=""
  [ "$v" = parent ] && dir=$AB_PARENT
  [ "$v" = on ] && extra=$on
  line=$(cd "$dir" && timeout -k 10 600 python bench.py "$@" $extra 2> "$errlog" | tail -1)
  st=$?
  if [ $st -ne 0 ]; then echo "[$v] bench.py $* $extra ended with status $st: stopping (stderr in $errlog)" | tee -a "$out"; exit $st; fi
  printf '%s\n' "$line" | python3 -c "
import json,sys
d=json.loads(sys.stdin.read())
print('[$v]', '|', $rep, '|', round(d['value'],2), '|', round(d['ms_per_step'],3))" | tee -a "$out"
  st=$?
  if [ $st -ne 0 ]; then echo "[$v] bench.py $* $extra printed no result line: stopping (stderr in $errlog)" | tee -a "$out"; exit $st; fi
done
done
