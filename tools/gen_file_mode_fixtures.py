#!/usr/bin/env python3
"""Generate tests/golden/file_mode.npz from the REFERENCE's own file-mode code.  TEST INFRASTRUCTURE ONLY.

Runs only where the reference checkout is present (REFERENCE_DIR, default /root/reference); never in a test, never on the GPU machine,
never imported by the product.  It holds none of the reference's text: it imports backend/main.py itself and records what its functions
return.

How main.py is imported offline (the technique of oracle/gen_vad_fixtures.py): its third-party and sibling imports that are absent or
heavy are replaced by stub modules before the import - dotenv, pydub (through utils), silero_vad (through vad), fastapi_cdn_host,
python_multipart (only its version probe), and the siblings asr / vad / vad_processor_manager / debug / connection_manager / utils /
models_manager.  backend/config.py is the real file.

What is recorded, per case (a file length, scripted VAD timestamps, a config):
  * `cut_long_segments` and `get_segments_summary` are called directly on the raw segments;
  * the `get_segments` closure is reached by driving the endpoint function `transcribe_file(file=fake, stream=False, config_str=...)`
    itself with `convert_audio_to_wav` / `audiosegment_to_tensor` / `standardize_audio_tensor` stubbed to hand over an index tensor of the
    case's length, a scripted `vad_processor` that returns the case's timestamps, and an `asr_model` that records the sample count and
    first-sample tag of every tensor it is handed.  The tensor holds sample index / 2**24 at every position, so the first value of a slice
    names its start sample exactly (fp32 holds integers up to 2**24).
The endpoint could be driven offline; no case needed the hand-derived fallback.

Usage:  python tools/gen_file_mode_fixtures.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import asyncio
import importlib.machinery
import json
import os
import sys
import types
from unittest import mock

import numpy as np

REF = os.path.join(os.environ.get("REFERENCE_DIR", "/root/reference"), "backend")
SR = 16000

# name -> (total_samples, scripted timestamps or None, config)
CASES = {
    "vad_off_short": (5 * SR, None, {"vad_enabled": False}),
    "vad_off_long": (100 * SR + 123, None, {"vad_enabled": False}),
    "vad_off_long_15": (100 * SR + 123, None, {"vad_enabled": False, "max_segment_duration": 15}),
    "below_one_second": (SR - 1, [{"start": 100, "end": 9000}], {}),
    "tiny_file": (1000, None, {"vad_enabled": False}),
    "no_speech": (20 * SR, [], {}),
    "touching_ends": (20 * SR, [{"start": 0, "end": 3 * SR}, {"start": 10 * SR, "end": 20 * SR}], {}),
    "end_clamped": (20 * SR, [{"start": 5 * SR, "end": 20 * SR + 400}, {"start": 20 * SR + 50, "end": 20 * SR + 900}], {}),
    "pair_closer_than_100": (20 * SR, [{"start": 4000, "end": 4040}, {"start": 8000, "end": 8000 + 1601}, {"start": 12000, "end": 12000 + 1600}], {}),
    "only_short_pairs": (20 * SR, [{"start": 4000, "end": 4040}, {"start": 9000, "end": 9100}], {}),
    "exactly_max_30": (100 * SR, [{"start": SR, "end": 31 * SR}, {"start": 40 * SR, "end": 70 * SR + 1}], {}),
    "exactly_max_15": (100 * SR, [{"start": SR, "end": 16 * SR}, {"start": 40 * SR, "end": 70 * SR}], {"max_segment_duration": 15}),
    "last_sub_dropped_30": (100 * SR, [{"start": 2 * SR, "end": 62 * SR + 1600}, {"start": 70 * SR, "end": 75 * SR}], {}),
    "last_sub_kept_30": (100 * SR, [{"start": 2 * SR, "end": 62 * SR + 1601}], {}),
    "last_sub_dropped_15": (100 * SR, [{"start": 0, "end": 45 * SR + 800}], {"max_segment_duration": 15, "hotwords": ["iPhone"]}),
    "mixed_30": (120 * SR, [{"start": 3 * SR, "end": 9 * SR}, {"start": 9 * SR + 8000, "end": 10 * SR + 3200}, {"start": 20 * SR, "end": 61 * SR},
                            {"start": 75 * SR, "end": 110 * SR + 77}], {}),
    "mixed_15": (120 * SR, [{"start": 3 * SR, "end": 9 * SR}, {"start": 9 * SR + 8000, "end": 10 * SR + 3200}, {"start": 20 * SR, "end": 61 * SR},
                            {"start": 75 * SR, "end": 110 * SR + 77}], {"max_segment_duration": 15}),
    "fractional_max": (50 * SR, [{"start": 0, "end": 50 * SR}], {"max_segment_duration": 7.3}),
}


def _stub(name, **attrs):
    m = mock.MagicMock(name=name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__name__ = name
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference():
    for name in ("dotenv", "fastapi_cdn_host", "asr", "vad", "vad_processor_manager", "debug", "connection_manager", "utils", "models_manager"):
        _stub(name)
    pm = types.ModuleType("python_multipart")
    pm.__version__ = "0.0.20"
    pm.__spec__ = importlib.machinery.ModuleSpec("python_multipart", None)
    sys.modules.setdefault("python_multipart", pm)
    sys.path.insert(0, REF)
    import main as ref_main          # the reference file itself
    return ref_main


class FakeUpload:
    filename, size = "case.wav", 4

    async def read(self):
        return b"RIFF"


class ScriptedVAD:
    def __init__(self, ts):
        self.ts, self.calls = ts, 0

    def detect_voice_activity(self, audio, threshold=None):
        self.calls += 1
        return [dict(t) for t in self.ts], len(self.ts) > 0


class RecordingASR:
    def __init__(self):
        self.calls = []

    def transcribe(self, tensor, sampling_rate=16000, max_new_tokens=128, hotwords=None, **kw):
        flat = tensor.reshape(-1)
        self.calls.append((int(round(float(flat[0]) * 2 ** 24)), int(flat.numel()), int(max_new_tokens), list(hotwords or [])))
        return f" seg@{self.calls[-1][0]} "


def run_case(ref_main, total, ts, config):
    import torch
    assert total <= 2 ** 24
    audio = torch.arange(total, dtype=torch.float32) / float(2 ** 24)
    ref_main.convert_audio_to_wav = lambda content, name: "audio"
    ref_main.audiosegment_to_tensor = lambda a: audio
    ref_main.standardize_audio_tensor = lambda t: t
    vad, asr = ScriptedVAD(ts or []), RecordingASR()
    ref_main.vad_processor, ref_main.asr_model = vad, asr
    out = asyncio.run(ref_main.transcribe_file(file=FakeUpload(), stream=False, config_str=json.dumps(config) if config else None))
    max_seg = float(config.get("max_segment_duration") or ref_main.AppConfig.MAX_SEGMENT_DURATION)
    results = out["segments"]
    # ranges the endpoint handed to the model, in call order -> by start sample (up to three run concurrently)
    ranges = sorted((a, a + n) for a, n, _, _ in asr.calls)
    return {"total_samples": total, "timestamps": ts, "config": config, "max_segment_duration": max_seg, "vad_calls": vad.calls,
            "decoded_ranges": ranges, "max_new_tokens": sorted({c[2] for c in asr.calls}), "hotwords_seen": [c[3] for c in asr.calls][:1],
            "segment_results": [{k: r[k] for k in ("segment_index", "original_index", "start_time", "end_time", "duration", "is_long_segment", "text")}
                                for r in results],
            "n_results": len(results), "total_duration": out["total_duration"], "config_echo": out["config"]}


def run_direct(ref_main, rec):
    """cut_long_segments + get_segments_summary called directly.  Their input, the raw segments of the get_segments closure, is recorded from
    a second run of the endpoint with the system default maximum raised so far that nothing is cut: one decode per raw segment."""
    total, sr = rec["total_samples"], SR
    uncut_cfg = {k: v for k, v in rec["config"].items() if k != "max_segment_duration"}
    default = ref_main.AppConfig.MAX_SEGMENT_DURATION       # the config model bounds the request's value, not the system default
    ref_main.AppConfig.MAX_SEGMENT_DURATION = 1e9
    try:
        uncut = run_case(ref_main, total, rec["timestamps"], uncut_cfg)
    finally:
        ref_main.AppConfig.MAX_SEGMENT_DURATION = default
    raw = []
    for r, (a, b) in zip(uncut["segment_results"], uncut["decoded_ranges"]):
        d = (b - a) / sr
        raw.append({"original_index": r["original_index"], "start_sample": a, "end_sample": b, "start_time": a / sr, "end_time": b / sr,
                    "duration": d, "is_long_segment": d > rec["max_segment_duration"]})
    final = ref_main.cut_long_segments(raw, sr, total, total / sr, max_segment_duration=rec["max_segment_duration"])
    for i, seg in enumerate(final):
        seg["segment_index"] = i + 1
    return {"raw": raw, "final": final, "summary": ref_main.get_segments_summary(final, sr)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    ref_main = load_reference()
    cases = {}
    for name, (total, ts, config) in CASES.items():
        rec = run_case(ref_main, total, ts, config)
        rec["direct"] = run_direct(ref_main, rec) if total >= 1600 else None
        cases[name] = rec
        print(f"{name}: {rec['n_results']} decoded of {len(rec['direct']['final']) if rec['direct'] else '-'} planned, ranges {rec['decoded_ranges'][:4]}"
              f"{' ...' if len(rec['decoded_ranges']) > 4 else ''}")
    np.savez_compressed(os.path.join(a.out, "file_mode.npz"), cases=json.dumps(cases))
