"""File mode and the ring VAD against the host forms they replace, on one MI355X (synthetic weights); writes profiles/file_mode.json.

  1. VAD pass over a 10-minute file: VADProcessor.detect_voice_activity on the host float tensor (upload of the whole file + a host copy
     per call) against detect_voice_activity_ring on a ring that already holds the file.  Also the one-off append of the file to the ring.
  2. File mode as a whole, time to the segments_summary record and to the last record:
       * the reference's shape on the existing API: host VAD, plan_segments, then three threads calling transcribe() per segment
         (main.py:429-445's semaphore of three)
       * ASRModel.transcribe_file on the default scheduler and on bulk=True (max_batch=64, decoders=3, slots=4)
  3. Streaming tick, 128 sessions x 640 ms: is_voice_active_batch on host windows against ring_scorer on ring ranges.

Every figure is host call to host result: median and p90 over --iters calls behind --warmup untimed ones (whole-file runs: --file-iters),
one process, nothing else on the GPU.  Record, do not gate: no threshold is set anywhere."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sonicscribe_amd import filemode, spec, synth, vad_net  # noqa: E402

SR = 16000


def stats(ts):
    ts = np.asarray(ts, np.float64)
    return {"median_ms": round(float(np.median(ts)), 3), "p90_ms": round(float(np.percentile(ts, 90)), 3), "min_ms": round(float(ts.min()), 3), "n": int(ts.size)}


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def make_file(seconds, seed=3):
    """speech-like sections of 2-40 s between silences of 1.2-3 s: the VAD yields many segments, some longer than 30 s"""
    rng = np.random.default_rng(seed)
    x = np.zeros(seconds * SR, np.int16)
    pos = SR
    while pos < x.size - SR:
        n = int(rng.uniform(2.0, 40.0) * SR)
        b = min(x.size, pos + n)
        x[pos:b] = np.rint(synth.synth_pcm(seed * 100 + pos % 9973, b - pos) * rng.uniform(0.3, 1.0)).astype(np.int16)
        pos = b + int(rng.uniform(1.2, 3.0) * SR)
    return x


def reference_shape(model, vad, f32, hotwords=None):
    """host VAD -> plan -> three threads of transcribe(); returns (ms to the summary, ms to the last result, segments)"""
    t0 = time.perf_counter()
    ts, _ = vad.detect_voice_activity(f32[None, :])
    final, summary = filemode.plan_segments(f32.size, ts, True, 30.0)
    t_summary = (time.perf_counter() - t0) * 1e3
    todo, lock, texts = list(range(len(final))), threading.Lock(), [None] * len(final)

    def worker():
        while True:
            with lock:
                if not todo:
                    return
                i = todo.pop(0)
            s = final[i]
            texts[i] = model.transcribe(f32[None, s["start_sample"]:s["end_sample"]], 16000, max_new_tokens=256, hotwords=hotwords)
    th = [threading.Thread(target=worker) for _ in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return t_summary, (time.perf_counter() - t0) * 1e3, len(final)


def file_mode(model, vad, pcm):
    t0 = time.perf_counter()
    t_summary, n = None, 0
    for rec in model.transcribe_file(pcm, vad):
        if rec["type"] == "segments_summary":
            t_summary = (time.perf_counter() - t0) * 1e3
        n += rec["type"] == "segment_result"
    return t_summary, (time.perf_counter() - t0) * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="full", choices=["tiny", "full"])
    ap.add_argument("--minutes", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--file-iters", type=int, default=3)
    ap.add_argument("--skip-file", action="store_true", help="only the VAD pass and the streaming tick")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "file_mode.json"))
    a = ap.parse_args()
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.vad import VADProcessor
    dims = spec.FULL if a.dims == "full" else spec.TINY
    vad = VADProcessor(weights=vad_net.synthetic_weights(7, **vad_net.RESPONSIVE))
    pcm = make_file(a.minutes * 60)
    f32 = pcm.astype(np.float32) / np.float32(32768.0)
    res = {"what": f"file mode and ring VAD against their host forms; {a.dims} dims, {a.minutes}-minute synthetic file, one MI355X, synthetic weights",
           "method": f"host call to host result; median / p90 of {a.iters} calls after {a.warmup} untimed (whole files: {a.file_iters} after 1)"}

    model = ASRModel.from_synthetic(dims, device="cuda:0", max_batch=32, max_ctx=1024)
    eng = model.model
    # 1. VAD pass
    ring = eng.ring_create(pcm.size)
    t0 = time.perf_counter()
    first = ring.append(pcm)
    eng.synchronize()
    append_ms = (time.perf_counter() - t0) * 1e3
    host = vad.detect_voice_activity(f32[None, :])
    dev = vad.detect_voice_activity_ring(ring, first, pcm.size)
    res["vad_pass"] = {"host_tensor": timed(lambda: vad.detect_voice_activity(f32[None, :]), a.iters, a.warmup),
                       "ring": timed(lambda: vad.detect_voice_activity_ring(ring, first, pcm.size), a.iters, a.warmup),
                       "ring_append_once_ms": round(append_ms, 3), "same_timestamps": host == dev, "speech_segments": len(host[0])}
    ring.close()

    # 3. streaming tick: 128 sessions x one 640 ms window
    S, n = 128, 10240
    seqs = [np.rint(synth.synth_pcm(i, n) * 0.5).astype(np.int16) for i in range(S)]
    rings = [eng.ring_create(30 * SR) for _ in range(S)]
    pieces = [[(r, r.append(s), n)] for r, s in zip(rings, seqs)]
    thr = np.full(S, 0.5)
    score = vad.ring_scorer()
    same = bool(np.array_equal(vad.is_voice_active_batch(seqs, thr), score(np.arange(S), pieces, thr)))
    res["tick_128"] = {"host_windows": timed(lambda: vad.is_voice_active_batch(seqs, thr), a.iters, a.warmup),
                       "ring_ranges": timed(lambda: score(np.arange(S), pieces, thr), a.iters, a.warmup),
                       "host_probs_only": timed(lambda: vad.probs(seqs), a.iters, a.warmup),
                       "ring_probs_only": timed(lambda: vad.probs_rings(eng, pieces), a.iters, a.warmup), "same_decisions": same}
    for r in rings:
        r.close()

    # 2. file mode as a whole
    if not a.skip_file:
        fm = {}
        reference_shape(model, vad, f32)                                   # warm-up: graphs of every batch size
        runs = [reference_shape(model, vad, f32) for _ in range(a.file_iters)]
        fm["three_transcribe_threads"] = {"to_summary": stats([r[0] for r in runs]), "to_last_record": stats([r[1] for r in runs]), "segments": runs[0][2]}
        file_mode(model, vad, pcm)
        runs = [file_mode(model, vad, pcm) for _ in range(a.file_iters)]
        fm["transcribe_file_default"] = {"to_summary": stats([r[0] for r in runs]), "to_last_record": stats([r[1] for r in runs]), "segments": runs[0][2]}
        model.close()
        model = ASRModel.from_synthetic(dims, device="cuda:0", max_batch=64, max_ctx=1024, bulk=True, decoders=3, slots=4)
        file_mode(model, vad, pcm)
        runs = [file_mode(model, vad, pcm) for _ in range(a.file_iters)]
        fm["transcribe_file_bulk"] = {"to_summary": stats([r[0] for r in runs]), "to_last_record": stats([r[1] for r in runs]), "segments": runs[0][2]}
        res["file_mode"] = fm
    model.close()
    vad.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
