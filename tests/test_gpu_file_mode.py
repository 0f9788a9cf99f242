"""File mode on the device (ASRModel.transcribe_file / transcribe_files, sonicscribe_amd/filemode.py): record for record, string for
string, equal to the composition of what existed before it - host `vad.detect_voice_activity(float tensor)` -> `plan_segments` ->
`model.transcribe(float slice, max_new_tokens=256, hotwords=...)` per segment - apart from wall-clock values.  TINY model, synthetic VAD
weights, a bursty two-minute int16 file."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vad_torch_ref import TorchVAD  # noqa: E402

from sonicscribe_amd import filemode, spec, synth, vad_net  # noqa: E402

pytestmark = pytest.mark.gpu

VAD_SEED = 7
FILE_SEED = 115         # chosen on the CPU (tests/vad_torch_ref.py): every probability of the file is >= 1e-3 away from 0.5 and 0.35
SR = 16000
WALL = ("timestamp", "processing_time", "completed_at")
SECTIONS = [(2.0, 7.5), (10.0, 10.9), (14.0, 55.0), (58.5, 66.0), (70.0, 104.0), (108.0, 118.7)]


def bursty(i, n, rng):
    """tests/test_gpu_vad.py::bursty: synth_pcm bursts of random loudness between short silences"""
    x = np.zeros(n, np.float64)
    pos = 0
    while pos < n:
        gap, burst = int(rng.integers(0, 6000)), int(rng.integers(2000, 12000))
        a, b = min(n, pos + gap), min(n, pos + gap + burst)
        if b > a:
            x[a:b] = synth.synth_pcm(1000 * i + pos, b - a) * rng.uniform(0.05, 1.0)
        pos = b
    return np.rint(x).astype(np.int16)


def make_file(seed, seconds=120, sections=SECTIONS):
    """bursty sections between silences longer than the VAD's 1 s: several speech segments, two of them longer than 30 s"""
    rng = np.random.default_rng(seed)
    x = np.zeros(seconds * SR, np.int16)
    for k, (a, b) in enumerate(sections):
        a, b = int(a * SR), int(b * SR)
        x[a:b] = bursty(seed * 10 + k, b - a, rng)
    return x


@pytest.fixture(scope="module")
def weights():
    return vad_net.synthetic_weights(VAD_SEED, **vad_net.RESPONSIVE)


@pytest.fixture(scope="module")
def vad(weights):
    from sonicscribe_amd.vad import VADProcessor
    v = VADProcessor(weights=weights)
    yield v
    v.close()


@pytest.fixture(scope="module")
def model():
    from sonicscribe_amd.asr import ASRModel
    m = ASRModel.from_synthetic(spec.TINY, device="cuda:0", max_batch=16, max_ctx=1024)
    yield m
    m.close()


@pytest.fixture(scope="module")
def pcm():
    return make_file(FILE_SEED)


def as_float(pcm):
    return pcm.astype(np.float32) / np.float32(32768.0)


def strip(rec):
    return {k: v for k, v in rec.items() if k not in WALL}


def compose(model, vad, pcm, vad_enabled=True, hotwords=None, max_seg=None, filename=""):
    """the records file mode must yield, from the parts that existed before it"""
    f = as_float(pcm)
    total, max_seg = len(pcm), float(max_seg or 30.0)
    ts = None
    if vad_enabled and total / SR >= 1.0:
        ts, _ = vad.detect_voice_activity(f[None, :])
    final, summary = filemode.plan_segments(total, ts, vad_enabled, max_seg)
    hot = list(hotwords) if hotwords else []
    out = [{"type": "initialization", "filename": filename, "file_size": 2 * total, "total_duration": round(total / SR, 2), "total_segments": len(final),
            "config": {"vad_enabled": vad_enabled, "hotwords": hot, "max_segment_duration": max_seg}},
           {"type": "segments_summary", "segments": summary, "total_segments": len(final)}]
    ok = bad = 0
    for seg in final:
        a, b = seg["start_sample"], seg["end_sample"]
        if b - a < 1600:
            bad += 1
            out.append({"type": "segment_error", "segment_index": seg["segment_index"], "original_index": seg["original_index"],
                        "is_long_segment": seg["is_long_segment"], "progress": round((ok + bad) / len(final) * 100, 1)})
            continue
        text = model.transcribe(f[None, a:b], 16000, max_new_tokens=256, hotwords=hotwords)
        ok += 1
        out.append({"type": "segment_result", "segment_index": seg["segment_index"], "original_index": seg["original_index"],
                    "start_time": round(seg["start_time"], 3), "end_time": round(seg["end_time"], 3), "duration": round(seg["duration"], 3),
                    "text": text.strip(), "is_long_segment": seg["is_long_segment"], "hotwords_used": hot,
                    "progress": round((ok + bad) / len(final) * 100, 1)})
    out.append({"type": "final_summary", "total_segments": len(final), "successful_segments": ok, "failed_segments": bad,
                "total_duration": round(total / SR, 2), "message": "转录完成", "hotwords_used": hot, "vad_enabled": vad_enabled})
    return out, final


def run(model, vad, audio, **kw):
    recs = [strip(r) for r in model.transcribe_file(audio, vad, **kw)]
    for r in recs:
        if r["type"] == "segment_error":
            r.pop("error")
    return recs


def test_input_is_not_vacuous(model, vad, weights, pcm):
    p = TorchVAD(weights).probs(pcm)
    margin = min(np.abs(p - 0.5).min(), np.abs(p - 0.35).min())
    print(f"\nfile: {len(p)} windows, nearest probability to a threshold: {margin:.3g}")
    assert margin >= 1e-3                                   # zero exclusions: no decision of this file is near its threshold
    ts, has = vad.detect_voice_activity(as_float(pcm)[None, :])
    assert has and ts == vad_net.speech_timestamps(p, len(pcm), 0.5, **vad_net.FILE_PARAMS)
    final, _ = filemode.plan_segments(len(pcm), ts, True, 30.0)
    assert len(ts) >= 3 and len(final) >= 3 and any(s["sub_segment_count"] > 1 for s in final)
    wide, _ = filemode.plan_segments(len(pcm), ts, True, 45.0)
    assert any(s["end_sample"] - s["start_sample"] > 30 * SR for s in wide)      # one request of several windows


def test_equals_the_composition(model, vad, pcm):
    want, final = compose(model, vad, pcm, filename="two_minutes.wav")
    got = run(model, vad, pcm, filename="two_minutes.wav")
    assert got == want
    assert [r["type"] for r in got[:2]] == ["initialization", "segments_summary"] and got[-1]["type"] == "final_summary"
    assert len({r["text"] for r in got if r["type"] == "segment_result"}) >= 3
    # a maximum above 30 s: segments longer than one encoder window are single requests of several windows sharing one peak
    assert run(model, vad, pcm, max_segment_duration=45.0) == compose(model, vad, pcm, max_seg=45.0)[0]


def test_modes(model, vad, pcm):
    assert run(model, vad, pcm, vad_enabled=False) == compose(model, vad, pcm, vad_enabled=False)[0]
    half = pcm[2 * SR:2 * SR + SR // 2]
    assert run(model, vad, half) == compose(model, vad, half)[0]
    zeros = np.zeros(20 * SR, np.int16)
    got = run(model, vad, zeros)
    assert got == compose(model, vad, zeros)[0] and got[0]["total_segments"] == 1
    want = compose(model, vad, pcm)[0]
    assert run(model, vad, as_float(pcm)[None, :]) == want
    import torch
    assert run(model, vad, torch.from_numpy(as_float(pcm)).unsqueeze(0)) == want
    hot = ["iPhone", "MacBook"]
    got = run(model, vad, pcm, hotwords=hot)
    assert got == compose(model, vad, pcm, hotwords=hot)[0] and got[-1]["hotwords_used"] == hot
    assert [r["text"] for r in got if r["type"] == "segment_result"] != [r["text"] for r in want if r["type"] == "segment_result"]
    assert run(model, vad, pcm, max_segment_duration=15) == compose(model, vad, pcm, max_seg=15)[0]
    with pytest.raises(ValueError, match="not int16 / 32768"):
        next(model.transcribe_file(as_float(pcm) * np.float32(0.3), vad))


def test_error_isolation(model, vad, pcm, monkeypatch):
    want = [r for r in run(model, vad, pcm) if r["type"] == "segment_result"]
    real = filemode.plan_segments

    def with_stub(total, ts, vad_enabled, max_seg, sample_rate=16000):
        final, _ = real(total, ts, vad_enabled, max_seg, sample_rate)
        short = dict(final[1], start_sample=final[1]["end_sample"] + 10, end_sample=final[1]["end_sample"] + 810, duration=0.05)
        final = final[:2] + [short] + final[2:]
        for i, s in enumerate(final):
            s["segment_index"] = i + 1
        return final, filemode.segments_summary(final)

    monkeypatch.setattr(filemode, "plan_segments", with_stub)
    got = list(model.transcribe_file(pcm, vad))
    errs = [r for r in got if r["type"] == "segment_error"]
    assert len(errs) == 1 and errs[0]["segment_index"] == 3 and "800" in errs[0]["error"]
    assert [r["text"] for r in got if r["type"] == "segment_result"] == [r["text"] for r in want]
    assert got[-1]["failed_segments"] == 1 and got[-1]["successful_segments"] == len(want)
    monkeypatch.undo()
    tiny = pcm[2 * SR:2 * SR + 1000]                      # a whole file below 0.1 s: the reference's segment_error (main.py:606-607)
    got = run(model, vad, tiny, vad_enabled=False)
    assert got == compose(model, vad, tiny, vad_enabled=False)[0] and got[2]["type"] == "segment_error"


def test_summary_before_any_result(model, vad, pcm):
    g = model.transcribe_file(pcm, vad)
    first, second = next(g), next(g)
    assert first["type"] == "initialization" and second["type"] == "segments_summary"
    assert len(second["segments"]) == first["total_segments"] >= 3
    rest = list(g)
    assert [r["type"] for r in rest[:-1]] == ["segment_result"] * first["total_segments"]
    assert [r["segment_index"] for r in rest[:-1]] == list(range(1, first["total_segments"] + 1))


def test_schedulers_agree(vad, pcm, model):
    """the default scheduler (row-level, `model`), the batch-by-batch one and the bulk pipeline give the same texts"""
    from sonicscribe_amd.asr import ASRModel
    want = [r.get("text") for r in run(model, vad, pcm)]
    assert sum(t is not None for t in want) >= 3
    for kw in ({"continuous": False}, {"continuous": True}, {"bulk": True, "max_batch": 32}):
        m = ASRModel.from_synthetic(spec.TINY, device="cuda:0", **{"max_batch": 16, "max_ctx": 1024, **kw})
        try:
            assert [r.get("text") for r in run(m, vad, pcm)] == want, kw
            assert [r.get("text") for r in run(m, vad, pcm, max_segment_duration=45.0)] == \
                [r.get("text") for r in run(model, vad, pcm, max_segment_duration=45.0)], kw      # multi-window requests too
            assert len(getattr(m.model, "_rings", [])) == 0
        finally:
            m.close()


def test_concurrency(model, vad, pcm):
    files = [pcm, make_file(FILE_SEED + 1, 60, [(1.0, 9.0), (12.0, 48.0), (51.0, 58.0)]), pcm[10 * SR:70 * SR]]
    solo = [run(model, vad, f, filename=f"f{i}") for i, f in enumerate(files)]
    got = [None, None]

    def work(i):
        got[i] = run(model, vad, files[i], filename=f"f{i}")

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert got == solo[:2]
    its = model.transcribe_files(files, vad, filenames=["f0", "f1", "f2"])
    many = []
    for it in its:
        recs = [strip(r) for r in it]
        many.append(recs)
    assert many == solo


def test_ring_lifetime(model, vad, pcm):
    """the file's ring is gone after exhaustion, after close() of a half-consumed generator and of a never-started one: by the library's
    own account (sonic_memory_info counts ring memory; a stale handle is refused by the registry), not only by the Python list"""
    import ctypes as C
    import types
    eng = model.model
    base = eng.memory_info()[0]
    registered = len(getattr(eng, "_rings", []))

    def stale_of(ring):
        return types.SimpleNamespace(h=C.c_void_p(ring.h.value), engine=eng)

    def assert_gone(stale):
        assert len(eng._rings) == registered and eng.memory_info()[0] == base
        with pytest.raises(RuntimeError, match="or was destroyed"):
            vad.probs_rings(eng, [[(stale, 0, 512)]])

    g = model.transcribe_file(pcm, vad)
    next(g)
    assert len(eng._rings) == registered + 1              # the file's ring lives while the generator does
    assert eng.memory_info()[0] == base + 2 * len(pcm)
    stale = stale_of(eng._rings[-1])
    assert len(vad.probs_rings(eng, [[(stale, 0, 512)]])[0]) == 1
    list(g)
    assert_gone(stale)
    g = model.transcribe_file(pcm, vad)
    next(g), next(g), next(g)
    stale = stale_of(eng._rings[-1])
    g.close()                                             # half consumed
    assert_gone(stale)
    its = model.transcribe_files([pcm[:30 * SR], pcm[:20 * SR]], vad)
    assert len(eng._rings) == registered + 2 and eng.memory_info()[0] == base + 2 * 50 * SR
    stales = [stale_of(r) for r in eng._rings[-2:]]
    its[0].close()                                        # never started
    list(its[1])
    for st in stales:
        assert_gone(st)
    assert run(model, vad, pcm[:20 * SR]) == compose(model, vad, pcm[:20 * SR])[0]      # and the model still works
