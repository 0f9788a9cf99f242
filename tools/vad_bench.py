"""Silero VAD network on the GPU (sonic_vad_probs via sonicscribe_amd.vad.VADProcessor), synthetic weights:
  * ms per streaming tick: 16 and 128 sessions x one 640 ms window (10 240 int16 samples), host call to host result (H2D, both kernels,
    D2H; probs = the network alone, decide = + get_speech_timestamps' post-processing per session = is_voice_active_batch)
  * the same while another thread keeps a dispatcher decoding (ASRModel.transcribe_batch in a loop)
  * ms per minute of audio for one 10-minute sequence (file mode, detect_voice_activity's network pass)
  * the CPU stand-in: the float64 torch.nn restatement of tests/vad_torch_ref.py at 16 threads.  The real Silero (silero_vad package,
    TorchScript) was not installed on the measuring host, so no CPU number of the reference's own VAD is measured.
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from sonicscribe_amd import spec, synth, vad_net  # noqa: E402


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return {"median_ms": round(float(np.median(ts)), 4), "p90_ms": round(float(np.percentile(ts, 90)), 4), "n": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--dims", default="full", choices=["tiny", "full"], help="dimensions of the decode that runs beside the VAD")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from sonicscribe_amd.vad import VADProcessor
    w = vad_net.synthetic_weights(7, **vad_net.RESPONSIVE)
    vad = VADProcessor(weights=w)
    ticks = {S: [synth.synth_pcm(i, 10240) for i in range(S)] for S in (16, 128)}
    thr = {S: np.full(S, 0.5) for S in ticks}
    res = {"what": "Silero VAD network (synthetic weights, fp32) on one MI355X; host call to host result", "idle": {}, "beside_decode": {}}
    for S, seqs in ticks.items():
        res["idle"][f"tick_{S}_probs"] = timed(lambda: vad.probs(seqs), a.iters)
        res["idle"][f"tick_{S}_decide"] = timed(lambda: vad.is_voice_active_batch(seqs, thr[S]), a.iters)
    ten = synth.synth_pcm(5, 10 * 60 * 16000)
    r = timed(lambda: vad.probs([ten]), 5, warmup=1)
    res["idle"]["file_10min"] = dict(r, ms_per_audio_minute=round(r["median_ms"] / 10.0, 4), windows=vad_net.n_windows(ten.size))

    from sonicscribe_amd.asr import ASRModel
    m = ASRModel.from_synthetic(spec.FULL if a.dims == "full" else spec.TINY, device="cuda:0", max_batch=32, max_ctx=512)
    audio = [synth.synth_pcm(100 + i, 16000 * 5).astype(np.float32) / 32768.0 for i in range(32)]
    m.transcribe_batch(audio[:2], 16000, max_new_tokens=8)
    stop, batches = threading.Event(), [0]

    def decode_loop():
        while not stop.is_set():
            m.transcribe_batch(audio, 16000, max_new_tokens=64)
            batches[0] += 1
    th = threading.Thread(target=decode_loop)
    th.start()
    time.sleep(1.0)
    try:
        for S, seqs in ticks.items():
            res["beside_decode"][f"tick_{S}_probs"] = timed(lambda: vad.probs(seqs), a.iters)
        r = timed(lambda: vad.probs([ten]), 3, warmup=1)
        res["beside_decode"]["file_10min"] = dict(r, ms_per_audio_minute=round(r["median_ms"] / 10.0, 4))
    finally:
        stop.set()
        th.join()
    res["beside_decode"]["decode"] = f"{a.dims} dims, 32 x 5 s requests, 64 new tokens, {batches[0]} batches during the VAD calls"
    m.close()
    vad.close()

    if not a.no_cpu:
        import torch
        from vad_torch_ref import TorchVAD
        torch.set_num_threads(16)
        ref = TorchVAD(w)
        res["cpu_standin"] = {
            "what": "tests/vad_torch_ref.py (float64 torch.nn layers) at 16 threads; the real silero_vad TorchScript model is not installed on the measuring host",
            "tick_128_probs": timed(lambda: ref.probs_batch(ticks[128]), 3, warmup=1),
            "tick_16_probs": timed(lambda: ref.probs_batch(ticks[16]), 3, warmup=1),
        }
        one = ten[:60 * 16000]
        r = timed(lambda: ref.probs(one), 1, warmup=0)
        res["cpu_standin"]["ms_per_audio_minute"] = r["median_ms"]
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
