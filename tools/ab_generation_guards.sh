#!/bin/bash
# A/B: the generation guards (sonic_set_generation: repetition_penalty, no_repeat_ngram_size and suppress_tokens inside greedy_kernel<T, LP, true>,
# csrc/greedy.hip) against the default engine.  `python bench.py` without and with all three guards on, alternating, on one MI355X;
# the headline (segments/s) and ms_per_step of every run go to profiles/generation_guards_ab.txt.  Arguments are handed to bench.py
# (e.g. --gpus 1 --steps 20 --warmup 3).
#   AB_PARENT=<dir>  a built checkout of the parent commit: its `python bench.py` runs first in every repetition, as the control of "off did not move"
#   AB_REPS=<n>      repetitions (default 2)
#   AB_OUT=<file>    the result file (default profiles/generation_guards_ab.txt)
# Limitation: the guards go in through bench.py's --opt, i.e. as the integer keys of sonic_set_option (penalty 1.1 in thousandths, n-gram size 3,
# gen_suppress_token), and that key carries ONE id - the "on" leg measures a one-entry suppress list.  The list's length only sets how many of the
# prologue's at most 256 LDS ORs happen (one trip of the 1024 threads either way); the loop's work per score does not depend on it.
# The first run that fails - a non-zero status of bench.py, its time limit, or a result line that does not parse - ends the script: nothing more is
# started on the card.  bench.py's stderr of the run in hand is kept beside the result file (*.stderr.txt, not committed).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
root=$PWD
out=${AB_OUT:-profiles/generation_guards_ab.txt}
case "$out" in /*) ;; *) out=$root/$out ;; esac
errlog=${out%.txt}.stderr.txt
reps=${AB_REPS:-2}
on="--opt gen_repetition_penalty_milli=1100 --opt gen_no_repeat_ngram_size=3 --opt gen_suppress_token=5"
variants=(off on)
[ -n "$AB_PARENT" ] && variants=(parent off on)
{
  echo "# tools/ab_generation_guards.sh $*: python bench.py $* on one MI355X, alternating, $reps repetition(s):"
  [ -n "$AB_PARENT" ] && echo "#   [parent] the parent commit (its library built from its own sources in a checkout of its own)"
  echo "#   [off]    this tree untouched"
  echo "#   [on]     this tree, $on (a one-entry suppress list: --opt carries one id)"
  echo "# columns: variant | repetition | headline 20s-segments/s | ms_per_step"
} > "$out"
for rep in $(seq 1 "$reps"); do
for v in "${variants[@]}"; do
  dir=$root; extra=""
  [ "$v" = parent ] && dir=$AB_PARENT
  [ "$v" = on ] && extra=$on
  line=$(cd "$dir" && timeout -k 10 900 python bench.py "$@" $extra 2> "$errlog" | tail -1)
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
