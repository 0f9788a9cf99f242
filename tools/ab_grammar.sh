#!/bin/bash
# A/B: option grammar (greedy_kernel<T, true, true, ., ., ., true>, csrc/greedy.hip) against the log-probability kernels it grows from: the decode
# step time at 32 and 64 rows on one MI355X.  Every leg is a process of its own: an engine of the full dimensions with synthetic weights and option
# token_logprobs, R requests of 20 s decoded for up to 64 token steps through the hipGraph loop, AB_RUNS times after two warm-up runs; the leg's figure is the
# median over those runs of sonic_timings' decode_ms / decode_steps (device events around the decode loop).  Legs, back to back, AB_REPS times:
#   [parent]      the option does not exist: a built checkout of the parent commit (AB_PARENT=<dir>; left out when unset)
#   [off]         this tree, option off: the kernels of the parent, instantiated from the new source
#   [free]        this tree, option on, every row free (state -1): the GRAMMAR kernel of the guard family, its prologue skipped row by row
#   [constrained] this tree, option on, every row under one 1 000-phrase grammar (random phrases of 2 .. 4 tokens, repeat: behind every phrase any of the 1 000 may
#                 follow, or EOS - the nodes behind a phrase end have about 1 000 edges): edges OR-ed into the map, the map inverted, the transition bisected.  The
#                 rows' tokens differ from the other legs' (that is the point) and a row may end early on EOS; a finished row keeps running its block until the
#                 batch ends, so the step does not get cheaper, and the steps a run took are printed beside its time
# The spread line at the end is the largest difference between two repetitions of the same leg: [off] against [parent] has to lie within it, and a verdict
# line per row count says whether it does.
#   AB_REPS=<n> repetitions (default 3)   AB_RUNS=<n> timed runs per leg (default 10)   AB_OUT=<file> (default profiles/grammar_ab.txt)
# The first leg that fails - a non-zero status, its time limit, or no result line - ends the script: nothing more is started on the card.  The stderr of the
# leg in hand is kept beside the result file (*.stderr.txt, not committed).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
root=$PWD
out=${AB_OUT:-profiles/grammar_ab.txt}
case "$out" in /*) ;; *) out=$root/$out ;; esac
errlog=${out%.txt}.stderr.txt
reps=${AB_REPS:-3}; runs=${AB_RUNS:-10}
legs=(off free constrained)
[ -n "$AB_PARENT" ] && legs=(parent off free constrained)
prog='
import sys, numpy as np
from sonicscribe_amd import spec, synth
from sonicscribe_amd.engine import Engine
R, leg, runs = int(sys.argv[1]), sys.argv[2], int(sys.argv[3])
d = spec.FULL
e = Engine(d, 0, 0, max_batch=R, max_ctx=1024)
e.set_option("token_logprobs", 1)
if leg in ("free", "constrained"):
    e.set_option("grammar", 1)
e.load_synthetic(20260128)
kw = {}
if leg == "constrained":
    from sonicscribe_amd.grammar import Grammar
    rng = np.random.default_rng(1000)
    ids = np.setdiff1d(np.arange(1000, d.vocab - 1000), list(d.eos_ids) + [d.audio_token_id])
    phrases = [tuple(int(t) for t in rng.choice(ids, int(rng.integers(2, 5)), replace=False)) for _ in range(1000)]
    g = Grammar._build([phrases], phrases, d.eos_ids, d.vocab, d.audio_token_id)      # repeat: any phrase may follow a phrase
    kw["request_grammar"] = [e.grammar_create(g)] * R
segs = [synth.synth_pcm(100 + r, 320000) for r in range(R)]
n_audio = spec.audio_token_count(spec.valid_frames(320000))
prompts = [[1, 17, 23, 5] + [d.audio_token_id] * n_audio + [7, 301, 302, 303, 9, 11]] * R
ms, steps = [], []
for i in range(runs + 2):
    out = e.transcribe_batch(segs, prompts, [64] * R, want_logprobs=True, **kw)
    t = e.timings()
    if i >= 2:
        ms.append(t["decode_ms"] / max(1, t["decode_steps"])); steps.append(t["decode_steps"])
print("RESULT %.4f %.4f %.4f %d" % (float(np.median(ms)), min(ms), max(ms), int(np.median(steps))))
e.close()
'
{
  echo "# tools/ab_grammar.sh: decode step time (ms; median of $runs runs of up to 64 token steps, sonic_timings decode_ms / decode_steps) on one MI355X, $reps repetition(s)"
  echo "# columns: leg | rows | repetition | median ms/step | min | max | token steps of a run"
} > "$out"
for rep in $(seq 1 "$reps"); do
for R in 32 64; do
for v in "${legs[@]}"; do
  dir=$root; leg=$v
  [ "$v" = parent ] && { dir=$AB_PARENT; leg=off; }
  line=$(cd "$dir" && timeout -k 10 240 python3 -c "$prog" $R $leg $runs 2> "$errlog" | grep '^RESULT' | tail -1)
  st=$?
  if [ $st -ne 0 ] || [ -z "$line" ]; then echo "[$v] rows $R ended with status $st and no result line: stopping (stderr in $errlog)" | tee -a "$out"; exit 1; fi
  set -- $line
  echo "[$v] | $R | $rep | $2 | $3 | $4 | $5" | tee -a "$out"
done
done
done
python3 - "$out" <<'PY' | tee -a "$out"
import sys, collections
rows = collections.defaultdict(list)
for l in open(sys.argv[1]):
    if l.startswith("["):
        leg, R, rep, med, lo, hi, steps = [x.strip() for x in l.split("|")]
        rows[leg, int(R)].append(float(med))
spread = max(max(v) - min(v) for v in rows.values())
print("# run-to-run spread (largest difference between two repetitions of one leg): %.4f ms" % spread)
for R in (32, 64):
    m = {leg: sorted(v)[len(v) // 2] for (leg, r), v in rows.items() if r == R}
    base = m.get("[parent]", m["[off]"])
    print("# rows %d: " % R + ", ".join("%s %.4f ms (%+.4f)" % (leg, x, x - base) for leg, x in sorted(m.items())))
    if "[parent]" in m:
        d = abs(m["[off]"] - m["[parent]"])
        print("# rows %d: |[off] - [parent]| = %.4f ms, %s the run-to-run spread of %.4f ms" % (R, d, "WITHIN" if d <= spread else "OUTSIDE", spread))
PY
