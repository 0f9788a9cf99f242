"""What row forks are worth to best_of, host call to return -> profiles/best_of_bench.json (a record, not a test; DESIGN.md 6.12 quotes it).

Full dimensions, synthetic weights, 12 audios of 20 s, best_of = 5, one temperature, 60 (audio, seed) pairs on one handle of 64 rows:
  forked     ONE Engine.transcribe_batch of the 12 audios with forks = [5] * 12: 12 windows through log-mel, encoder and prefill, 60 rows through the head and the loop
  unforked   the same 60 pairs as 60 requests of one Engine.transcribe_batch - every audio five times - which is all a handle without forks can do
Wall times: warm-up rounds, then the two forms alternating round by round; median, 10th / 90th percentile and the count.  Beside them the device's stage times of
each form's last run (sonic_timings), fork_kv_kernel's time in the forked run from the engine's events (sonic_debug_read "fork_ms"), sonic_memory_info before and
after the first forked run, and how many of the 60 rows carry the same ids in both forms (beyond 32 rows the decode step's batch invariance is not promised: a
count, not a check).  Nothing is asserted.

    python tools/best_of_bench.py [--rounds 7] [--warmup 2] [--audios 12] [--best-of 5] [--tokens 64] [--tiny]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sonicscribe_amd import sampling, spec, synth  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs) * 1e3, 3), "p10_ms": round(xs[len(xs) // 10] * 1e3, 3), "p90_ms": round(xs[(len(xs) * 9) // 10] * 1e3, 3), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--audios", type=int, default=12)
    ap.add_argument("--best-of", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "best_of_bench.json"))
    a = ap.parse_args()
    from sonicscribe_amd.engine import Engine
    d = spec.TINY if a.tiny else spec.FULL
    A, N, n = a.audios, a.best_of, int(a.seconds * 16000)
    segs = [synth.synth_pcm(300 + i, n) for i in range(A)]
    prompt = [1, 17, 23, 5] + [d.audio_token_id] * spec.audio_token_count(spec.valid_frames(n)) + [7, 301, 302, 303, 9, 11]
    eng = Engine(d, 0, 0, max_batch=64, max_ctx=1024)
    eng.set_option("token_logprobs", 1)
    eng.set_option("sampling", 1)
    eng.load_synthetic(20260128)
    rows = Engine.fork_rows([N] * A)
    pair = {r: (i, j) for i, rr in enumerate(rows) for j, r in enumerate(rr)}                  # row -> (audio, fork)
    samp = [(a.temperature, sampling.fork_seed(1000 * pair[r][0], pair[r][1])) for r in range(A * N)]

    def forked():
        ids, _ = eng.transcribe_batch(segs, [prompt] * A, [a.tokens] * A, request_sampling=samp, forks=[N] * A)
        ms = np.zeros(1, np.float32)
        eng._check(eng.lib.sonic_debug_read(eng.h, b"fork_ms", 0, ms.ctypes.data_as(ctypes.c_void_p), 1))
        return ids, dict(eng.timings()), float(ms[0])

    def unforked():        # the same rows in the same order: row r is audio pair[r][0] with fork pair[r][1]'s seed
        ids, _ = eng.transcribe_batch([segs[pair[r][0]] for r in range(A * N)], [prompt] * (A * N), [a.tokens] * (A * N), request_sampling=samp)
        return ids, dict(eng.timings()), 0.0
    mem0 = eng.memory_info()[0]
    forked()
    mem1 = eng.memory_info()[0]
    forms = [("forked", forked), ("unforked", unforked)]
    t, last = {k: [] for k, _ in forms}, {}
    for r in range(a.warmup + a.rounds):
        k = r % len(forms)
        for name, fn in forms[k:] + forms[:k]:
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                t[name].append(dt)
                last[name] = out
    stages = ("mel_ms", "encoder_ms", "prefill_ms", "decode_ms", "total_ms")
    res = {"dims": "tiny" if a.tiny else "full", "seconds": a.seconds, "audios": A, "best_of": N, "rows": A * N, "tokens": a.tokens, "temperature": a.temperature,
           "prompt_tokens": len(prompt), "wall": {k: spread(v) for k, v in t.items()},
           "device": {k: {s: round(float(last[k][1][s]), 3) for s in stages} | {"decode_steps": int(last[k][1]["decode_steps"])} for k in last},
           "fork_kernel_ms": round(last["forked"][2], 4),
           "fork_kernel_bytes": int(2 * A * d.dec_layers * d.dec_kv_heads * len(prompt) * d.dec_head_dim * 2 * N),      # K and V: read once, written N - 1 times
           "memory_added_bytes": int(mem1 - mem0),
           "rows_with_equal_ids": int(sum(np.array_equal(x, y) for x, y in zip(last["forked"][0], last["unforked"][0])))}
    eng.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
