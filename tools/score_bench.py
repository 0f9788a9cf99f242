"""What scoring given transcripts costs, host call to return -> profiles/score_bench.json (a record, not a test; DESIGN.md 6.8 and 6.14 quote it).

Full dimensions, synthetic weights, one 20 s segment.  First shape, 8 candidates of 150 tokens each, four measurements on ONE handle:
  (a) fanout    the parallel forced run with forced_fanout = 8: one encoder pass, eight sequences in one prefill
  (b) staged8   the parallel forced run with the audio staged eight times: eight encoder passes
  (c) stepwise  the same eight sequences through the step-by-step forced run (option forced_parallel off): the eager decode loop, one step per token
  (d) shared    (a) with forced_share_prompt: the prompt is prefilled once, seven sequences pack only their own tokens
Second shape ("phrase_list"), 32 candidates of 6 tokens each on a handle of max_batch 32: (a) and (d) alone.
Wall time per call: warm-up rounds, then the forms alternating round by round (so drift hits all of them alike); median, 10th / 90th percentile and the
count are reported for each, and the device's own stage times of the last round.  Nothing is asserted.

    python tools/score_bench.py [--rounds 7] [--warmup 2] [--candidates 8] [--tokens 150] [--tiny]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sonicscribe_amd import spec, synth  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs) * 1e3, 3), "p10_ms": round(xs[len(xs) // 10] * 1e3, 3), "p90_ms": round(xs[(len(xs) * 9) // 10] * 1e3, 3), "n": len(xs)}


def bits_equal(a, b):
    return bool(np.array_equal(a.astype(np.float32).view(np.uint32), b.astype(np.float32).view(np.uint32)))


def measure(d, a, C, n_tok, which):
    """the forms named in `which` on one handle of max_batch max(8, C), alternating -> the shape's record"""
    from sonicscribe_amd.engine import Engine
    eng = Engine(d, 0, 0, max_batch=max(8, C), max_ctx=1024)
    eng.set_option("token_logprobs", 1)
    eng.load_synthetic(20260128)
    mem0 = eng.memory_info()[0]
    pcm = synth.synth_pcm(10, int(a.seconds * 16000))
    n_audio = spec.audio_token_count(spec.valid_frames(len(pcm)))
    prompt = [1, 17, 23, 5] + [d.audio_token_id] * n_audio + [7, 301, 302, 303, 9, 11]
    rng = np.random.default_rng(1)
    bad = set(d.eos_ids) | {d.audio_token_id}
    ok = np.array([t for t in range(d.vocab) if t not in bad], np.int32)
    force = ok[rng.integers(0, len(ok), (C, n_tok))].astype(np.int32)

    def fanout():
        eng.set_option("forced_parallel", 1)
        return eng.score_batch([pcm], [prompt] * C, force, fanout=C)

    def shared():
        eng.set_option("forced_parallel", 1)
        return eng.score_batch([pcm], [prompt] * C, force, fanout=C, share_prompt=True)

    def staged():
        eng.set_option("forced_parallel", 1)
        return eng.score_batch([pcm] * C, [prompt] * C, force)

    def stepwise():
        eng.set_option("forced_parallel", 0)
        eng.set_forced_ids(force)
        try:
            return eng.transcribe_batch([pcm] * C, [prompt] * C, [n_tok] * C, want_logprobs=True)
        finally:
            eng.set_forced_ids(None)
    every = {"fanout": fanout, "staged8": staged, "stepwise": stepwise, "shared": shared}
    forms = [(k, every[k]) for k in which]
    t = {k: [] for k, _ in forms}
    dev, last, tokens = {}, {}, {}
    for r in range(a.warmup + a.rounds):
        order = forms[r % len(forms):] + forms[:r % len(forms)]
        for name, fn in order:
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            last[name] = out
            if r >= a.warmup:
                t[name].append(dt)
                tm = eng.timings()
                dev[name] = {k: round(float(tm[k]), 3) for k in ("mel_ms", "encoder_ms", "prefill_ms", "decode_ms", "total_ms")}
                if name in ("fanout", "shared"):
                    tokens[name] = int(eng.debug_read("score_tokens", (1,))[0])
    mem1 = eng.memory_info()[0]
    eng.close()
    lp = {k: np.concatenate([np.asarray(x, np.float64) for x in v[2]]) for k, v in last.items()}
    rec = {"dims": "tiny" if a.tiny else "full", "seconds": a.seconds, "candidates": C, "tokens": n_tok, "prompt_tokens": len(prompt),
           "rounds": a.rounds, "warmup": a.warmup, "wall": {k: spread(v) for k, v in t.items()}, "device_last_round": dev, "prefill_tokens": tokens,
           "score_buffers_bytes": int(mem1 - mem0)}
    w = rec["wall"]
    if "staged8" in lp:
        rec["fanout_equals_staged8_bits"] = bits_equal(lp["fanout"], lp["staged8"])
        rec["staged8_over_fanout"] = round(w["staged8"]["median_ms"] / w["fanout"]["median_ms"], 2)
    if "stepwise" in lp:
        rec["max_abs_dlp_parallel_vs_stepwise"] = float(np.abs(lp["fanout"] - lp["stepwise"]).max())
        rec["stepwise_over_fanout"] = round(w["stepwise"]["median_ms"] / w["fanout"]["median_ms"], 2)
    rec["max_abs_dlp_shared_vs_fanout"] = float(np.abs(lp["shared"] - lp["fanout"]).max())
    rec["shared_equals_fanout_bits"] = bits_equal(lp["shared"], lp["fanout"])
    rec["shared_over_fanout"] = round(w["shared"]["median_ms"] / w["fanout"]["median_ms"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=150)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    a = ap.parse_args()
    d = spec.TINY if a.tiny else spec.FULL
    rec = measure(d, a, a.candidates, a.tokens, ("fanout", "staged8", "stepwise", "shared"))
    rec["phrase_list"] = measure(d, a, 32, 6, ("fanout", "shared"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
