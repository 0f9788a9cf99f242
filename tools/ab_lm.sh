#!/bin/bash
# A/B: shallow fusion (options lm / lm_weight: lm_step_kernel, csrc/lm.hip, and greedy_kernel<T, true, true, ., ., ., false, ., true>, csrc/greedy.hip)
# against the log-probability kernels it grows from: the decode step time at 32 and 64 rows on one MI355X.  Every leg is a process of its own: an engine of the full
# dimensions with synthetic weights and option token_logprobs, R requests of 20 s decoded for up to 64 token steps through the hipGraph loop, AB_RUNS times after two
# warm-up runs; the leg's figure is the median over those runs of sonic_timings' decode_ms / decode_steps (device events around the decode loop).  Legs, back to
# back, AB_REPS times:
#   [parent]  the option does not exist: a built checkout of the parent commit (AB_PARENT=<dir>; left out when unset)
#   [off]     this tree, option off: the kernels of the parent, instantiated from the new source
#   [zero]    this tree, a 3-gram model of about 1 M edges on the handle at weight 0: both kernels run, the vector is zeros and the tokens are the [off] leg's
#   [lm]      the same model at weight 0.3: the tokens differ from the other legs' (that is the point); the steps a run took are printed beside its time
# The model: 200 000 random trigrams over 20 000 ids with their bigrams and unigrams (ngram.NGramLM.from_ngrams) - about 1 M edges, most of them at the 20 000 bigram
# contexts' nodes; every step of a row walks a chain of up to two links and writes its levels' edges over the dense pass.
# The spread line at the end is the largest difference between two repetitions of the same leg: [off] against [parent] has to lie within it, and a verdict line per
# row count says whether it does.
#   AB_REPS=<n> repetitions (default 3)   AB_RUNS=<n> timed runs per leg (default 10)   AB_OUT=<file> (default profiles/lm_ab.txt)
# The first leg that fails - a non-zero status, its time limit, or no result line - ends the script: nothing more is started on the card.  The stderr of the leg in
# hand is kept beside the result file (*.stderr.txt, not committed).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
root=$PWD
out=${AB_OUT:-profiles/lm_ab.txt}
case "$out" in /*) ;; *) out=$root/$out ;; esac
errlog=${out%.txt}.stderr.txt
reps=${AB_REPS:-3}; runs=${AB_RUNS:-10}
legs=(off zero lm)
[ -n "$AB_PARENT" ] && legs=(parent off zero lm)
prog='
import sys, numpy as np
from sonicscribe_amd import spec, synth
from sonicscribe_amd.engine import Engine
R, leg, runs = int(sys.argv[1]), sys.argv[2], int(sys.argv[3])
d = spec.FULL
e = Engine(d, 0, 0, max_batch=R, max_ctx=1024)
e.set_option("token_logprobs", 1)
e.load_synthetic(20260128)
edges = 0
if leg in ("zero", "lm"):
    from sonicscribe_amd.ngram import NGramLM
    rng = np.random.default_rng(1000)
    ids = rng.choice(np.arange(1000, d.vocab - 1000), 20000, replace=False)
    grams = {(int(t),): (float(w), -0.5) for t, w in zip(ids, rng.uniform(-12, -4, len(ids)))}
    ctx = [(int(a), int(b)) for a, b in zip(rng.choice(ids, 20000), rng.choice(ids, 20000))]
    for c in ctx:
        grams[c] = (float(rng.uniform(-6, -1)), -0.4)
    for c in ctx:
        for t in ids[rng.integers(0, len(ids), 10)]:
            grams[c + (int(t),)] = (float(rng.uniform(-4, -0.1)), 0.0)
    for c0 in sorted(set(c[0] for c in ctx)):             # wide bigram nodes: 60 further continuations of every first id
        for t in ids[rng.integers(0, len(ids), 60)]:
            grams.setdefault((c0, int(t)), (float(rng.uniform(-6, -1)), 0.0))
    lm = NGramLM.from_ngrams(d.vocab, grams, floor=-15.0)
    edges = lm.n_edges
    e.set_lm(e.lm_create(lm), 0.0 if leg == "zero" else 0.3)
segs = [synth.synth_pcm(100 + r, 320000) for r in range(R)]
n_audio = spec.audio_token_count(spec.valid_frames(320000))
prompts = [[1, 17, 23, 5] + [d.audio_token_id] * n_audio + [7, 301, 302, 303, 9, 11]] * R
ms, steps = [], []
for i in range(runs + 2):
    out = e.transcribe_batch(segs, prompts, [64] * R, want_logprobs=True)
    t = e.timings()
    if i >= 2:
        ms.append(t["decode_ms"] / max(1, t["decode_steps"])); steps.append(t["decode_steps"])
print("RESULT %.4f %.4f %.4f %d %d" % (float(np.median(ms)), min(ms), max(ms), int(np.median(steps)), edges))
e.close()
'
{
  echo "# tools/ab_lm.sh: decode step time (ms; median of $runs runs of up to 64 token steps, sonic_timings decode_ms / decode_steps) on one MI355X, $reps repetition(s)"
  echo "# columns: leg | rows | repetition | median ms/step | min | max | token steps of a run | edges of the model"
} > "$out"
for rep in $(seq 1 "$reps"); do
for R in 32 64; do
for v in "${legs[@]}"; do
  dir=$root; leg=$v
  [ "$v" = parent ] && { dir=$AB_PARENT; leg=off; }
  line=$(cd "$dir" && timeout -k 10 300 python3 -c "$prog" $R $leg $runs 2> "$errlog" | grep '^RESULT' | tail -1)
  st=$?
  if [ $st -ne 0 ] || [ -z "$line" ]; then echo "[$v] rows $R ended with status $st and no result line: stopping (stderr in $errlog)" | tee -a "$out"; exit 1; fi
  set -- $line
  echo "[$v] | $R | $rep | $2 | $3 | $4 | $5 | $6" | tee -a "$out"
done
done
done
python3 - "$out" <<'PY' | tee -a "$out"
import sys, collections
rows = collections.defaultdict(list)
for l in open(sys.argv[1]):
    if l.startswith("["):
        leg, R, rep, med = [x.strip() for x in l.split("|")][:4]
        rows[(leg, int(R))].append(float(med))
spread = max((max(v) - min(v) for v in rows.values()), default=0.0)
print("# spread: the largest difference between two repetitions of one leg: %.4f ms" % spread)
for R in (32, 64):
    m = {leg: sum(v) / len(v) for (leg, r), v in rows.items() if r == R}
    if "[off]" not in m:
        continue
    line = "# rows %d: mean of the medians" % R + "".join("  %s %.4f" % (k, m[k]) for k in ("[parent]", "[off]", "[zero]", "[lm]") if k in m)
    if "[parent]" in m:
        two = rows[("[parent]", R)]
        own = max(two) - min(two)
        line += "  | off - parent %+.4f ms, two parent runs differ by %.4f: %s" % (m["[off]"] - m["[parent]"], own, "within" if abs(m["[off]"] - m["[parent]"]) <= max(own, spread) else "OUTSIDE")
    if "[zero]" in m:
        line += "  | zero - off %+.4f ms, lm - off %+.4f ms" % (m["[zero]"] - m["[off]"], m["[lm]"] - m["[off]"])
    print(line)
PY
