"""Host side of the Silero VAD network (sonicscribe_amd/vad_net.py): the state-dict loader, get_speech_timestamps' post-processing on
hand-built probabilities, and the torch restatement's window / context bookkeeping (tests/vad_torch_ref.py) against silero's contract."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sonicscribe_amd import vad_net  # noqa: E402

W = 512


def full_sd(seed=0):
    w = vad_net.synthetic_weights(seed)
    sd = {"_model." + k: v for k, v in w.items()}
    sd.update({"_model_8k." + k: np.zeros(1, np.float32) for k in w})      # the 8 kHz sub-model: ignored whatever its shapes
    return sd


def test_loader_accepts_and_refuses():
    w = vad_net.weights_from_state_dict(full_sd())
    assert list(w) == list(vad_net.LAYOUT) and all(w[k].shape == s and w[k].dtype == np.float32 for k, s in vad_net.LAYOUT.items())
    assert sum(a.size for a in w.values()) == 309_633          # ~1.24 MB of fp32
    bad = full_sd()
    bad["_model.encoder.1.reparam_conv.weight"] = np.zeros((64, 128, 5), np.float32)
    with pytest.raises(ValueError, match="encoder.1.reparam_conv.weight has shape"):
        vad_net.weights_from_state_dict(bad)
    bad = full_sd()
    del bad["_model.decoder.rnn.weight_hh"]
    with pytest.raises(ValueError, match="missing.*decoder.rnn.weight_hh"):
        vad_net.weights_from_state_dict(bad)
    bad = full_sd()
    bad["_model.decoder.extra"] = np.zeros(1)
    with pytest.raises(ValueError, match="unexpected"):
        vad_net.weights_from_state_dict(bad)


def test_synthetic_weights_are_default_init():
    w = vad_net.synthetic_weights(3)
    assert np.abs(w["encoder.0.reparam_conv.weight"]).max() <= 1 / np.sqrt(129 * 3)
    assert np.abs(w["decoder.rnn.weight_hh"]).max() <= 1 / np.sqrt(128)
    b = w["stft.forward_basis_buffer"][:, 0]
    assert b[0].sum() == pytest.approx(128.0) and np.abs(b[129]).max() == 0.0        # DC row: the Hann window; its imaginary row: zeros
    assert np.array_equal(vad_net.synthetic_weights(3)["decoder.rnn.bias_ih"], w["decoder.rnn.bias_ih"])


def ts(probs, n=None, **kw):
    probs = np.asarray(probs, np.float64)
    return vad_net.speech_timestamps(probs, len(probs) * W if n is None else n, **kw)


FILE = dict(vad_net.FILE_PARAMS)            # min_speech 300 ms = 4800 samples, min_silence 1000 ms = 16000 samples


def test_min_speech_boundary():
    # speech from window 10 to 14, then 4 windows (2048 samples) of silence >= min_silence (1600): the segment ends at window 14
    p = [0.0] * 10 + [0.9] * 4 + [0.0] * 8
    out = ts(p, threshold=0.5, min_speech_ms=100, max_speech_s=float("inf"), min_silence_ms=100)
    assert out == [{"start": 10 * W - 480, "end": 14 * W + 480}]
    # only 3 windows (1536 samples) of silence before the audio ends: the segment stays open and closes at the end of the audio
    out = ts(p[:18], threshold=0.5, min_speech_ms=100, max_speech_s=float("inf"), min_silence_ms=100)
    assert out == [{"start": 10 * W - 480, "end": 18 * W}]
    # exactly min_speech (min_speech_ms = 64 -> 1024 samples = 2 windows): dropped; one window longer: kept
    p2 = [0.0] * 4 + [0.9] * 2 + [0.0] * 10
    assert ts(p2, threshold=0.5, min_speech_ms=64, min_silence_ms=100) == []
    p3 = [0.0] * 4 + [0.9] * 3 + [0.0] * 10
    assert ts(p3, threshold=0.5, min_speech_ms=64, min_silence_ms=100) == [{"start": 4 * W - 480, "end": 7 * W + 480}]


def test_hysteresis_and_short_silence():
    # between neg_threshold (0.35) and threshold (0.5) nothing starts and nothing ends
    assert ts([0.45] * 40, threshold=0.5, **FILE) == []
    p = [0.9] * 10 + [0.4] * 60 + [0.1] * 40
    out = ts(p, threshold=0.5, **FILE)
    assert out == [{"start": 0, "end": 70 * W + 480}]
    # a silence shorter than min_silence does not end the segment: 20 windows = 10240 < 16000 samples
    p = [0.9] * 10 + [0.1] * 20 + [0.9] * 10 + [0.1] * 40
    assert ts(p, threshold=0.5, **FILE) == [{"start": 0, "end": 40 * W + 480}]


def test_open_segment_at_end():
    p = [0.1] * 10 + [0.8] * 20
    n = 30 * W - 100                                       # the last window is partial: the segment ends at the audio's end
    assert ts(p, n=n, threshold=0.5, **FILE) == [{"start": 10 * W - 480, "end": n}]


def test_neg_threshold_clamp():
    # threshold 0.1: neg = max(-0.05, 0.01) = 0.01, so 0.02 does not count as silence and 0.005 does
    p = [0.5] * 10 + [0.02] * 40
    assert ts(p, threshold=0.1, **FILE) == [{"start": 0, "end": 50 * W}]
    p = [0.5] * 10 + [0.005] * 40
    assert ts(p, threshold=0.1, **FILE) == [{"start": 0, "end": 10 * W + 480}]


def test_speech_pad_merges_close_segments():
    kw = dict(threshold=0.5, min_speech_ms=100, min_silence_ms=64, max_speech_s=float("inf"))
    p = [0.0] * 4 + [0.9] * 6 + [0.0] * 3 + [0.9] * 6 + [0.0] * 10
    # the first segment ends at 10 * 512 after 2 windows of silence (min_silence 1024), the next starts at 13 * 512: a gap of 1536 >= 2 * pad
    out = ts(p, **kw)
    assert out == [{"start": 4 * W - 480, "end": 10 * W + 480}, {"start": 13 * W - 480, "end": 19 * W + 480}]
    # min_silence 0: one silent window ends the segment at 10 * 512, the next starts at 11 * 512; the gap of 512 < 2 * pad is split in halves
    p = [0.0] * 4 + [0.9] * 6 + [0.0] * 1 + [0.9] * 6 + [0.0] * 10
    out = ts(p, threshold=0.5, min_speech_ms=100, min_silence_ms=0, max_speech_s=float("inf"))
    assert out == [{"start": 4 * W - 480, "end": 10 * W + 256}, {"start": 10 * W + 256, "end": 17 * W + 480}]


def test_max_speech_branch_refused():
    # is_voice_active: 14 528 samples of max speech; 20 windows (10 240 samples) cannot reach it, 30 windows can
    ok = np.full(20, 0.9)
    assert ts(ok, **vad_net.CHUNK_PARAMS, threshold=0.5) == [{"start": 0, "end": 20 * W}]
    with pytest.raises(NotImplementedError):
        ts(np.full(30, 0.9), **vad_net.CHUNK_PARAMS, threshold=0.5)
    with pytest.raises(ValueError):
        vad_net.speech_timestamps(np.zeros(3), 5 * W)


def silero_contract(x):
    """silero's model loop, literally: 512-sample chunks (last zero-padded), each preceded by the last 64 samples the model saw"""
    ctx = np.zeros(64)
    out = []
    for a in range(0, len(x), 512):
        c = np.asarray(x[a:a + 512], np.float64)
        c = np.pad(c, (0, 512 - len(c)))
        inp = np.concatenate([ctx, c])
        ctx = inp[-64:]
        out.append(inp)
    return np.array(out).reshape(-1, 576)


@pytest.mark.parametrize("n", [1, 512, 513, 10240, 7 * 16000 + 3])
def test_torch_reference_window_bookkeeping(n):
    from vad_torch_ref import windows
    x = np.random.default_rng(n).standard_normal(n)
    w = windows(x)
    assert w.shape == (vad_net.n_windows(n), 576)
    assert np.array_equal(w, silero_contract(x))


def test_torch_reference_runs_layers():
    """the float64 statement: a probability per window in (0, 1), the state reset per sequence (a batch equals solo runs)"""
    from vad_torch_ref import TorchVAD
    m = TorchVAD(vad_net.synthetic_weights(5, **vad_net.RESPONSIVE))
    rng = np.random.default_rng(0)
    a, b = (rng.integers(-8000, 8000, size=n).astype(np.int16) for n in (3000, 1200))
    pa, pb = m.probs_batch([a, b])
    assert len(pa) == 6 and len(pb) == 3 and ((pa > 0) & (pa < 1)).all()
    assert np.allclose(pa, m.probs(a), atol=1e-12, rtol=0) and np.allclose(pb, m.probs(b), atol=1e-12, rtol=0)


def test_vad_processor_refuses_without_weights_or_bad_rate():
    from sonicscribe_amd.vad import VADProcessor
    with pytest.raises(ValueError):
        VADProcessor(sampling_rate=44100, weights=vad_net.synthetic_weights(0))
    try:
        import silero_vad  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="weights="):
            VADProcessor(weights=None)
