#!/bin/bash
# A/B: option truncation (greedy_kernel<T, true, ., ., true, ., ., true>, csrc/greedy.hip, csrc/truncsel.h) against the default engine and against
# plain sampling.  `python bench.py` for the parent commit and this tree untouched, the two alternating (the headline: the bulk pipeline; with the option off
# launch_greedy picks the parent's kernels, so [off] must lie inside the spread of [parent]'s own repeats), then this tree through a non-bulk scheduler
# (--pipeline off) sampling at 0.6 without the option, with the TRUNC kernels and every filter off, and with top_k = 50, top_p = 0.9 on every row, back to back on
# one MI355X; the headline (segments/s) and ms_per_step of every run go to profiles/truncation_ab.txt.  Arguments are handed to bench.py (e.g. --gpus 1 --no-extras
# --no-cpu-baseline).
#   AB_PARENT=<dir>  a built checkout of the parent commit: its `python bench.py` runs first in every repetition
#   AB_REPS=<n>      repetitions (default 3)
#   AB_OUT=<file>    the result file (default profiles/truncation_ab.txt)
# --opt passes integers: the temperature comes from sampling_fill_milli=600 (request r at 0.6 with seed r) and the cut from truncation_fill=1 (top_k = 50,
# top_p = 0.9 on every row of a batch without values) - the same draw every time, so bench.py's token check still holds.
# The first run that fails - a non-zero status of bench.py, its time limit, or a result line that does not parse - ends the script: nothing more is started
# on the card.  bench.py's stderr of the run in hand is kept beside the result file (*.stderr.txt, not committed).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
root=$PWD
out=${AB_OUT:-profiles/truncation_ab.txt}
case "$out" in /*) ;; *) out=$root/$out ;; esac
errlog=${out%.txt}.stderr.txt
reps=${AB_REPS:-3}
t06="--pipeline off --opt token_logprobs=1 --opt sampling=1 --opt sampling_fill_milli=600"
tr0="$t06 --opt truncation=1"
trk="$tr0 --opt truncation_fill=1"
variants=(off t06 tr0 trk)
[ -n "$AB_PARENT" ] && variants=(parent off t06 tr0 trk)
{
  echo "# tools/ab_truncation.sh $*: python bench.py $* on one MI355X, back to back, $reps repetition(s):"
  [ -n "$AB_PARENT" ] && echo "#   [parent] the parent commit (its library built from its own sources in a checkout of its own)"
  echo "#   [off]    this tree untouched (the bulk pipeline)"
  echo "#   [t06]    this tree, $t06 (the SAMPLE kernels, every row at temperature 0.6)"
  echo "#   [tr0]    this tree, $tr0 (the TRUNC kernels, every filter off: the branch around the select)"
  echo "#   [trk]    this tree, $trk (top_k = 50, top_p = 0.9 on every row)"
  echo "# columns: variant | repetition | headline 20s-segments/s | ms_per_step"
} > "$out"
for rep in $(seq 1 "$reps"); do
for v in "${variants[@]}"; do
  dir=$root; extra=""
  [ "$v" = parent ] && dir=$AB_PARENT
  [ "$v" = t06 ] && extra=$t06
  [ "$v" = tr0 ] && extra=$tr0
  [ "$v" = trk ] && extra=$trk
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
