"""What resampling inside the ring append costs, host call to return -> profiles/resample_bench.json.

  append      a 64 ms chunk at 48000 / 44100 / 8000 Hz appended to 1 and to 128 rate rings, against the plain 16 kHz append (1024 samples) on
              the same build: median of >= 50 timed rounds after warm-up, the two forms alternating round by round.  A round appends one
              chunk to every ring; the rings' streams are drained outside the timer, so queued work cannot pile up behind it.
  whole file  a file of --file-seconds at 44100 Hz through transcribe_file(sampling_rate=44100) up to the segments_summary record, against
              host resample_sinc_hann + re-quantise + 16 kHz file mode.

    python tools/resample_bench.py [--rounds 60] [--file-seconds 600] [--tiny]
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

from sonicscribe_amd import frontend, spec, synth, vad_net  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median_us": round(statistics.median(xs) * 1e6, 1), "p10_us": round(xs[len(xs) // 10] * 1e6, 1), "p90_us": round(xs[(len(xs) * 9) // 10] * 1e6, 1),
            "n": len(xs)}


def append_cost(eng, rate, n_rings, rounds, warm=10):
    chunk = np.random.default_rng(rate).integers(-20000, 20000, size=int(rate * 0.064)).astype(np.int16)
    plain_chunk = chunk[:1024] if len(chunk) >= 1024 else np.resize(chunk, 1024)
    rated = [eng.ring_create(40 * 16000, rate=rate) for _ in range(n_rings)]
    plain = [eng.ring_create(40 * 16000) for _ in range(n_rings)]
    t = {"rate": [], "plain": []}
    try:
        for r in range(warm + rounds):
            for name, rings, data in (("rate", rated, chunk), ("plain", plain, plain_chunk)) if r % 2 == 0 else (("plain", plain, plain_chunk), ("rate", rated, chunk)):
                t0 = time.perf_counter()
                for ring in rings:
                    ring.append(data)
                dt = time.perf_counter() - t0
                for ring in rings:                                      # drain every ring's stream outside the timer
                    if ring.head:
                        ring.read(ring.head - 1, 1)
                if r >= warm:
                    t[name].append(dt / n_rings)
    finally:
        for ring in rated + plain:
            ring.close()
    return {"rate_hz": rate, "rings": n_rings, "chunk_samples": int(len(chunk)), "per_append": {k: spread(v) for k, v in t.items()}}


def whole_file(model, vad, seconds, rate=44100, repeats=3):
    n16 = seconds * 16000
    x16 = np.zeros(n16, np.float64)
    for a in range(0, seconds - 8, 10):
        x16[a * 16000:(a + 8) * 16000] = synth.synth_pcm(a, 8 * 16000) * 0.7
    x = np.rint(x16[(np.arange(int(n16 * rate / 16000)) * 16000 // rate)]).astype(np.int16)

    def until_summary(audio, **kw):
        t0 = time.perf_counter()
        it = model.transcribe_file(audio, vad, **kw)
        for rec in it:
            if rec["type"] == "segments_summary":
                break
        dt = time.perf_counter() - t0
        it.close()
        return dt

    dev, host = [], []
    for _ in range(repeats):
        dev.append(until_summary(x, sampling_rate=rate))
        t0 = time.perf_counter()
        y = frontend.resample_sinc_hann(x.astype(np.float32) / np.float32(32768.0), rate, 16000)
        q = np.clip(np.rint(y * np.float32(32768.0)), -32768, 32767).astype(np.int16)
        pre = time.perf_counter() - t0
        host.append(pre + until_summary(q))
    return {"file_seconds": seconds, "rate_hz": rate, "device_s": sorted(round(v, 4) for v in dev), "host_resample_then_file_mode_s": sorted(round(v, 4) for v in host)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--file-seconds", type=int, default=600)
    ap.add_argument("--tiny", action="store_true", help="TINY model dims (the resampler and the VAD do not depend on the model size)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.vad import VADProcessor
    model = ASRModel.from_synthetic(spec.TINY if a.tiny else spec.FULL, device="cuda:0", max_batch=16, max_ctx=1024)
    vad = VADProcessor(weights=vad_net.synthetic_weights(7, **vad_net.RESPONSIVE))
    res = {"tool": "tools/resample_bench.py", "rounds": a.rounds, "model": "TINY" if a.tiny else "FULL", "append": [], "whole_file": None}
    try:
        for rate in (48000, 44100, 8000):
            for n_rings in (1, 128):
                res["append"].append(append_cost(model.models[0], rate, n_rings, max(50, a.rounds)))
        res["whole_file"] = whole_file(model, vad, a.file_seconds)
    finally:
        vad.close()
        model.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
