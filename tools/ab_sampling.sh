#!/bin/bash
# A/B: option sampling (greedy_kernel<T, true, ., ., true>, csrc/greedy.hip) against the default engine.  `python bench.py` for the parent
# commit and this tree untouched (the headline: the bulk pipeline), then this tree through a non-bulk scheduler (--pipeline off: batches in flight on slots)
# with log-probabilities only, with the sampling kernels at temperature 0 and with them at temperature 0.6, back to back on one MI355X; the headline
# (segments/s) and ms_per_step of every run go to profiles/sampling_ab.txt.  Arguments are handed to bench.py (e.g. --gpus 1 --no-extras --no-cpu-baseline).
#   AB_PARENT=<dir>  a built checkout of the parent commit: its `python bench.py` runs first in every repetition, as the control of "off did not move"
#   AB_REPS=<n>      repetitions (default 3)
#   AB_OUT=<file>    the result file (default profiles/sampling_ab.txt)
# The sampled legs: the bulk pipeline carries no per-request values, so they run with --pipeline off, and [lp] is their own baseline (the LP kernels the SAMPLE
# kernels grow from).  --opt passes integers, so the temperature comes from the measurement option sampling_fill_milli=600: request r of every batch is decoded
# at 0.6 with seed r - the same draw every time, so bench.py's token check still holds.
# The first run that fails - a non-zero status of bench.py, its time limit, or a result line that does not parse - ends the script: nothing more is started
# on the card.  bench.py's stderr of the run in hand is kept beside the result file (*.stderr.txt, not committed).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
root=$PWD
out=${AB_OUT:-profiles/sampling_ab.txt}
case "$out" in /*) ;; *) out=$root/$out ;; esac
errlog=${out%.txt}.stderr.txt
reps=${AB_REPS:-3}
lp="--pipeline off --opt token_logprobs=1"
t0="$lp --opt sampling=1"
t06="$t0 --opt sampling_fill_milli=600"
variants=(off lp t0 t06)
[ -n "$AB_PARENT" ] && variants=(parent off lp t0 t06)
{
  echo "# tools/ab_sampling.sh $*: python bench.py $* on one MI355X, back to back, $reps repetition(s):"
  [ -n "$AB_PARENT" ] && echo "#   [parent] the parent commit (its library built from its own sources in a checkout of its own)"
  echo "#   [off]    this tree untouched (the bulk pipeline)"
  echo "#   [lp]     this tree, $lp (non-bulk, the LP kernels)"
  echo "#   [t0]     this tree, $t0 (the SAMPLE kernels, every row at temperature 0)"
  echo "#   [t06]    this tree, $t06 (every row at temperature 0.6)"
  echo "# columns: variant | repetition | headline 20s-segments/s | ms_per_step"
} > "$out"
for rep in $(seq 1 "$reps"); do
for v in "${variants[@]}"; do
  dir=$root; extra=""
  [ "$v" = parent ] && dir=$AB_PARENT
  [ "$v" = lp ] && extra=$lp
  [ "$v" = t0 ] && extra=$t0
  [ "$v" = t06 ] && extra=$t06
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
