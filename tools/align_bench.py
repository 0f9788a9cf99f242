"""What word timestamps cost, host call to return -> profiles/align_bench.json (a record, not a test; DESIGN.md 6.9 quotes it).

Full dimensions, synthetic weights, one 20 s segment, one transcript of 150 tokens, the default heads (every head of the last half of the decoder layers).
  engine    score-only (option forced_align off) against score + align on ONE scoring handle, the option switched between the calls
  model     ASRModel.transcribe against ASRModel.transcribe(word_timestamps=True): the second encodes the audio once more on the scoring handle
Wall time per call: warm-up rounds, then the two forms alternating round by round; median, 10th / 90th percentile and the count, and the device's own stage times
of the last round.  The align handle's extra bytes are sonic_memory_info before and after its first align run, behind a score-only run.  Nothing is asserted.

    python tools/align_bench.py [--rounds 7] [--warmup 2] [--tokens 150] [--tiny]
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


def alternate(forms, warmup, rounds, after=None):
    t = {k: [] for k, _ in forms}
    extra = {}
    for r in range(warmup + rounds):
        order = forms[r % 2:] + forms[:r % 2]
        for name, fn in order:
            t0 = time.perf_counter()
            out = fn()
            dt = time.perf_counter() - t0
            if r >= warmup:
                t[name].append(dt)
                if after:
                    extra[name] = after(out)
    return {k: spread(v) for k, v in t.items()}, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=150)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    a = ap.parse_args()
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.engine import Engine
    d = spec.TINY if a.tiny else spec.FULL
    n_tok = a.tokens
    eng = Engine(d, 0, 0, max_batch=8, max_ctx=1024)
    eng.set_option("token_logprobs", 1)
    eng.set_option("forced_parallel", 1)
    eng.load_synthetic(20260128)
    pcm = synth.synth_pcm(10, int(a.seconds * 16000))
    n_audio = spec.audio_token_count(spec.valid_frames(len(pcm)))
    prompt = [1, 17, 23, 5] + [d.audio_token_id] * n_audio + [7, 301, 302, 303, 9, 11]
    rng = np.random.default_rng(1)
    bad = set(d.eos_ids) | {d.audio_token_id}
    ok = np.array([t for t in range(d.vocab) if t not in bad], np.int32)
    force = ok[rng.integers(0, len(ok), (1, n_tok))].astype(np.int32)

    def score():
        eng.set_option("forced_align", 0)
        return eng.score_batch([pcm], [prompt], force)

    def align():
        eng.set_option("forced_align", 1)
        return eng.score_batch([pcm], [prompt], force, align=True)
    score()
    mem0 = eng.memory_info()[0]
    times = align()[2][0].times
    mem1 = eng.memory_info()[0]

    def stages(_):
        tm = eng.timings()
        return {k: round(float(tm[k]), 3) for k in ("mel_ms", "encoder_ms", "prefill_ms", "total_ms")}
    wall_e, dev_e = alternate([("score", score), ("score_align", align)], a.warmup, a.rounds, stages)
    heads = ((d.dec_layers + 1) // 2) * d.dec_heads
    eng.close()

    m = ASRModel.from_synthetic(d, max_batch=8, max_ctx=1024, token_logprobs=True, scoring=True, timestamps=True)
    wav = pcm.astype(np.float32) / 32768.0
    wall_m, _ = alternate([("transcribe", lambda: m.transcribe(wav, max_new_tokens=n_tok)),
                           ("transcribe_word_timestamps", lambda: m.transcribe(wav, max_new_tokens=n_tok, word_timestamps=True))], a.warmup, a.rounds)
    r = m.transcribe(wav, max_new_tokens=n_tok, word_timestamps=True)
    m.close()
    rec = {"dims": "tiny" if a.tiny else "full", "seconds": a.seconds, "tokens": n_tok, "prompt_tokens": len(prompt), "audio_tokens": n_audio, "heads": heads,
           "rounds": a.rounds, "warmup": a.warmup, "engine_wall": wall_e, "engine_device_last_round": dev_e, "model_wall": wall_m,
           "align_over_score": round(wall_e["score_align"]["median_ms"] / wall_e["score"]["median_ms"], 3),
           "word_timestamps_over_transcribe": round(wall_m["transcribe_word_timestamps"]["median_ms"] / wall_m["transcribe"]["median_ms"], 3),
           "align_buffers_bytes": int(mem1 - mem0), "times_non_decreasing": bool(np.all(np.diff(times) >= 0)),
           "transcribed_tokens": int(len(r.token_ids)), "words": len(r.words)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
