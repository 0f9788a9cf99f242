"""Silero VAD network on the GPU (csrc/vad.hip, sonic_vad_*, sonicscribe_amd/vad.py) against the float64 torch.nn restatement
(tests/vad_torch_ref.py) on synthetic weights: probabilities, batch invariance, the reference's decisions, the streaming gate, a VAD call
beside a running decode, and - where the silero_vad package is importable - the real model."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vad_torch_ref import TorchVAD  # noqa: E402

from sonicscribe_amd import spec, synth, vad_net  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 7
CHUNK = 1024


@pytest.fixture(scope="module")
def weights():
    return vad_net.synthetic_weights(SEED, **vad_net.RESPONSIVE)


@pytest.fixture(scope="module")
def vad(weights):
    from sonicscribe_amd.vad import VADProcessor
    v = VADProcessor(weights=weights)
    yield v
    v.close()


@pytest.fixture(scope="module")
def ref(weights):
    return TorchVAD(weights)


def bursty(i, n, rng):
    """synth_pcm bursts of random loudness between silences: probabilities cross every threshold"""
    x = np.zeros(n, np.float64)
    pos = 0
    while pos < n:
        gap, burst = int(rng.integers(0, 6000)), int(rng.integers(2000, 12000))
        a, b = min(n, pos + gap), min(n, pos + gap + burst)
        if b > a:
            x[a:b] = synth.synth_pcm(1000 * i + pos, b - a) * rng.uniform(0.05, 1.0)
        pos = b
    return np.rint(x).astype(np.int16)


def test_probs_match_torch_layers(vad, ref):
    rng = np.random.default_rng(1)
    seqs = [bursty(i, 10240, rng) for i in range(128)]
    got, want = vad.probs(seqs), ref.probs_batch(seqs)
    d = max(np.abs(g - w).max() for g, w in zip(got, want))
    allp = np.concatenate(want)
    print(f"\n128 x 10240: max|dp| = {d:.3g} (p in [{allp.min():.3f}, {allp.max():.3f}])")
    assert d <= 1e-5
    ragged = [synth.synth_pcm(50 + i, n) for i, n in enumerate([1, 511, 512, 513, 10239, 10240, 7 * 16000 + 3])]
    got, want = vad.probs(ragged), ref.probs_batch(ragged)
    assert [len(g) for g in got] == [vad_net.n_windows(len(s)) for s in ragged]
    d = max(np.abs(g - w).max() for g, w in zip(got, want))
    print(f"ragged: max|dp| = {d:.3g}")
    assert d <= 1e-5
    # float input: the same samples as x / 32768 give the same bits; a float buffer above 1 is peak-normalised first
    f32 = [s.astype(np.float32) / np.float32(32768.0) for s in ragged]
    for a, b in zip(vad.probs(f32), got):
        assert np.array_equal(a, b)
    loud = [s.astype(np.float32) for s in ragged[3:]]
    d = max(np.abs(g - w).max() for g, w in zip(vad.probs(loud), ref.probs_batch(loud)))
    assert d <= 1e-5


def test_long_sequence(vad, ref):
    x = bursty(7, 5 * 60 * 16000, np.random.default_rng(2))
    got, want = vad.probs([x])[0], ref.probs(x)
    assert len(got) == 9375
    d = np.abs(got - want).max()
    print(f"\n5 min (9375 steps): max|dp| = {d:.3g}")
    assert d <= 1e-4


def test_batch_invariance(vad):
    rng = np.random.default_rng(3)
    seqs = [bursty(i, int(n), rng) for i, n in enumerate(rng.integers(1, 30000, size=128))]
    batch = vad.probs(seqs)
    rev = vad.probs(seqs[::-1])[::-1]
    for i in (0, 5, 64, 127):
        solo = vad.probs([seqs[i]])[0]
        assert np.array_equal(solo, batch[i]) and np.array_equal(solo, rev[i]), i
    for a, b in zip(batch, rev):
        assert np.array_equal(a, b)


def near(p, thr, eps=1e-5):
    neg = max(thr - 0.15, 0.01)
    return bool((np.abs(p - thr) <= eps).any() or (np.abs(p - neg) <= eps).any())


def test_decisions_equal_float64(vad, ref):
    rng = np.random.default_rng(4)
    seqs = [bursty(i, 10240, rng) for i in range(128)]
    thr = rng.choice([0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9], size=128)
    got = vad.is_voice_active_batch(seqs, thr)
    want_p = ref.probs_batch(seqs)
    excluded = 0
    for i in range(128):
        if near(want_p[i], thr[i]):
            excluded += 1
            continue
        want = len(vad_net.speech_timestamps(want_p[i], 10240, float(thr[i]), **vad_net.CHUNK_PARAMS)) > 0
        assert got[i] == want, i
    print(f"\ndecisions: {128 - excluded} equal, {excluded} within 1e-5 of a threshold (excluded); speech in {int(got.sum())}")
    assert excluded <= 8 and 0 < got.sum() < 128
    assert vad.is_voice_active(seqs[0].astype(np.float32) / 32768.0, float(thr[0])) == got[0]
    assert not vad.is_voice_active_batch([np.zeros(0, np.int16)], [0.5])[0]
    # file mode: 2 minutes of bursts and silences
    x = np.zeros(120 * 16000, np.float64)
    for k, (a, b) in enumerate([(3, 9), (9.5, 10.2), (20, 41), (43, 44), (60, 62), (75, 100), (101.5, 110)]):
        x[int(a * 16000):int(b * 16000)] = synth.synth_pcm(900 + k, int(b * 16000) - int(a * 16000)) * (0.3 + 0.1 * k)
    x = (x / 32768.0).astype(np.float32)
    ts, is_sp = vad.detect_voice_activity(x)
    p = ref.probs(x)
    assert not near(p, 0.5)
    assert ts == vad_net.speech_timestamps(p, len(x), 0.5, **vad_net.FILE_PARAMS) and is_sp and len(ts) >= 3
    assert vad.detect_voice_activity(np.zeros(0, np.float32)) == ([], False)


def _script(S, n_ticks, rng):
    wire = []
    for s in range(S):
        x = np.zeros(n_ticks * CHUNK, np.int16)
        for _ in range(3):
            a = int(rng.integers(0, n_ticks - 30)) * CHUNK
            n = int(rng.integers(10, 40)) * CHUNK
            x[a:a + n] = (synth.synth_pcm(s * 7 + a, min(n, x.size - a)) * rng.uniform(0.2, 1.0)).astype(np.int16)
        wire.append(x)
    return wire


def _run_sessions(model, wire, n_ticks, scorer):
    from sonicscribe_amd.sessions import GatedSessions
    S = len(wire)
    g = GatedSessions(model, [f"c{i}" for i in range(S)])
    events = []
    for t in range(n_ticks):
        for s in range(S):
            g.add_audio_chunk(s, wire[s][t * CHUNK:(t + 1) * CHUNK].tobytes(), timestamp=1000.0 + 0.064 * (t + 1))
        events.extend((e["session"], e["type"], e.get("start_chunk_id"), e.get("end_chunk_id")) for e in g.tick(scorer, now=1000.0 + 0.064 * (t + 1)))
    g.close()
    return events


def test_streaming_loop(vad, ref):
    from sonicscribe_amd.asr import ASRModel
    rng = np.random.default_rng(6)
    S, n_ticks = 16, 160
    wire = _script(S, n_ticks, rng)
    close = []

    def cpu_decisions(pcm, thr):
        out = []
        for p, t in zip(pcm, thr):
            pr = ref.probs(p)
            close.append(near(pr, t))
            out.append(len(vad_net.speech_timestamps(pr, len(p), float(t), **vad_net.CHUNK_PARAMS)) > 0)
        return np.array(out, bool)

    gpu = vad.scorer()
    n_calls, n_windows, differ = [0], [0], []

    def checked_gpu(rows, pcm, thr):          # the GPU scorer, each call also checked window by window against float64
        n_calls[0] += 1
        n_windows[0] += len(rows)
        k = len(close)
        a, b = gpu(rows, pcm, thr), cpu_decisions(pcm, thr)
        differ.extend(i for i in range(len(rows)) if a[i] != b[i] and not close[k + i])
        return a

    m = ASRModel.from_synthetic(spec.TINY, device="cuda:0", max_batch=8, max_ctx=512)
    try:
        want = _run_sessions(m, wire, n_ticks, lambda r, p, t: cpu_decisions(p, t))
        got = _run_sessions(m, wire, n_ticks, checked_gpu)
    finally:
        m.close()
    print(f"\nstreaming: {len(got)} events, {n_windows[0]} windows in {n_calls[0]} calls, {sum(close)} of {len(close)} windows within 1e-5 of a threshold")
    assert not differ
    assert sum(close) <= len(close) // 50
    if not any(close):
        assert got == want
    assert len({e[0] for e in got if e[1] == "speech_start"}) >= S // 2


def test_vad_beside_decode(vad, ref):
    """a VAD call while a dispatcher decodes: correct probabilities, and the decode's tokens equal the same decode without VAD"""
    from sonicscribe_amd.asr import ASRModel
    m = ASRModel.from_synthetic(spec.TINY, device="cuda:0", max_batch=8, max_ctx=512)
    try:
        pcms = [synth.synth_pcm(300 + i, 16000 * (2 + i % 3)) for i in range(8)]
        from sonicscribe_amd import frontend
        audio = [frontend.pcm_bytes_to_float(p.tobytes()) for p in pcms]
        alone = m.transcribe_batch(audio, 16000, max_new_tokens=24)
        seqs = [bursty(i, 10240, np.random.default_rng(8)) for i in range(128)]
        want = ref.probs_batch(seqs)
        got, res = [], []
        th = threading.Thread(target=lambda: res.append(m.transcribe_batch(audio, 16000, max_new_tokens=24)))
        th.start()
        for _ in range(10):
            got.append(vad.probs(seqs))
        th.join()
        assert res == [alone]
        for g in got:
            assert max(np.abs(a - b).max() for a, b in zip(g, want)) <= 1e-5
            assert all(np.array_equal(a, b) for a, b in zip(g, got[0]))
    finally:
        m.close()


def test_real_silero_model():
    silero = pytest.importorskip("silero_vad")
    import torch
    from sonicscribe_amd.vad import VADProcessor
    model = silero.load_silero_vad()
    v = VADProcessor(weights=None)
    try:
        rng = np.random.default_rng(9)
        x = (bursty(3, 60 * 16000, rng) / 32768.0).astype(np.float32)
        model.reset_states()
        want = []
        for a in range(0, len(x), 512):
            c = torch.tensor(x[a:a + 512])
            if len(c) < 512:
                c = torch.nn.functional.pad(c, (0, 512 - len(c)))
            want.append(model(c, 16000).item())
        got = v.probs([x])[0]
        assert np.abs(got - np.array(want)).max() <= 1e-4
        t = torch.tensor(x)
        assert v.detect_voice_activity(x)[0] == silero.get_speech_timestamps(t, model, threshold=0.5, sampling_rate=16000,
                                                                            min_speech_duration_ms=300, max_speech_duration_s=float("inf"),
                                                                            min_silence_duration_ms=1000)
        for a in range(0, len(x) - 10240, 10240 * 7):
            c = x[a:a + 10240]
            ref_ts = silero.get_speech_timestamps(torch.tensor(c), model, threshold=0.5, sampling_rate=16000, min_speech_duration_ms=100,
                                                  max_speech_duration_s=1.0, min_silence_duration_ms=100)
            assert v.is_voice_active(c, 0.5) == (len(ref_ts) > 0)
    finally:
        v.close()
