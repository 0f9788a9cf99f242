"""The resampler's host side: frontend.resample_bank (the coefficient bank the device kernel csrc/resample.hip builds too), the bound that
frontend.resample_sinc_hann - and, on the GPU, Engine.resample (tests/test_gpu_resample.py) - is held to, the emission rule of a rate ring
and the chunk -> sample-range map of AudioStream over one.

The bound is derived, not measured.  ref64 is the float64 product of the zero-padded frames with the fp32 bank taken to float64, A the same
product on absolute values, u = 2^-24:  |got - ref64| <= (K + 2) * u * A.  K * u * A bounds the fp32 accumulation error of a K-term dot
product in any order; 2 * u * A covers a bank entry that another double libm rounds to the neighbouring fp32 value."""
import math

import numpy as np
import pytest

from sonicscribe_amd import frontend

U = 2.0 ** -24
GEOMETRY = {48000: (3, 1, 19, 41), 44100: (441, 160, 17, 475), 8000: (1, 2, 7, 15), 11025: (441, 640, 7, 455)}
RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000]


def ref64_and_bound(x, in_rate, out_rate=16000):
    """(ref64, A, K) for the float samples x: every output of the zero-padded stream, trimmed to ceil(nf * n / of)"""
    bank, of, nf, width = frontend.resample_bank(in_rate, out_rate)
    K = bank.shape[1]
    x = np.asarray(x, np.float64)
    n = x.size
    n_out = -(-nf * n // of)
    frames = -(-n_out // nf)
    pad = np.zeros(width + max(n, (frames - 1) * of + K))
    pad[width:width + n] = x
    fr = np.lib.stride_tricks.as_strided(pad, shape=(frames, K), strides=(pad.strides[0] * of, pad.strides[0]))
    b = bank.astype(np.float64)
    return (fr @ b.T).reshape(-1)[:n_out], (np.abs(fr) @ np.abs(b).T).reshape(-1)[:n_out], K


def resample_sinc_hann_before(wav, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """frontend.resample_sinc_hann as it stood before resample_bank was factored out of it, verbatim"""
    wav = np.asarray(wav, dtype=np.float32)
    if orig_freq == new_freq or wav.size == 0:
        return wav
    g = math.gcd(int(orig_freq), int(new_freq))
    of, nf = int(orig_freq) // g, int(new_freq) // g
    base = min(of, nf) * rolloff
    width = math.ceil(lowpass_filter_width * of / base)
    idx = np.arange(-width, width + of, dtype=np.float64)[None, :] / of
    t = (np.arange(0, -nf, -1, dtype=np.float64)[:, None] / nf + idx) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        kern = np.where(t == 0, 1.0, np.sin(t) / t)
    kern = (kern * window * (base / of)).astype(np.float32)          # [nf][2*width + of]
    length = wav.shape[-1]
    x = np.pad(wav, (width, width + of))
    n_out = (x.size - kern.shape[1]) // of + 1
    frames = np.lib.stride_tricks.as_strided(x, shape=(n_out, kern.shape[1]), strides=(x.strides[0] * of, x.strides[0]))
    out = (frames @ kern.T).reshape(-1)
    target = int(math.ceil(nf * length / of))
    return out[:target].astype(np.float32)


def test_bank_geometry():
    for rate, (of, nf, width, K) in GEOMETRY.items():
        bank, o, n, w = frontend.resample_bank(rate, 16000)
        assert (o, n, w) == (of, nf, width) and bank.shape == (nf, K) and bank.dtype == np.float32 and K == 2 * width + of
        assert frontend.resample_geometry(rate, 16000) == (of, nf, width, K)
    assert frontend.resample_geometry(11025, 16000)[1] * 455 == 291200          # the largest bank of the common rates
    # a low-pass at unit DC gain: every phase sums to about 1 (the Hann-windowed sinc is not normalised exactly)
    for rate in RATES:
        bank = frontend.resample_bank(rate, 16000)[0]
        assert np.abs(bank.astype(np.float64).sum(axis=1) - 1.0).max() < 2e-2, rate


@pytest.mark.parametrize("rate", RATES + [16000])
def test_resample_sinc_hann_is_unchanged(rate):
    rng = np.random.default_rng(rate)
    for n in (0, 1, 2, 440, 441, 442, 4099):
        x = rng.standard_normal(n).astype(np.float32)
        a, b = frontend.resample_sinc_hann(x, rate, 16000), resample_sinc_hann_before(x, rate, 16000)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (rate, n)
    x = rng.standard_normal(1000).astype(np.float32)
    assert frontend.resample_sinc_hann(x, 16000, rate).tobytes() == resample_sinc_hann_before(x, 16000, rate).tobytes()


@pytest.mark.parametrize("rate", RATES)
def test_resample_sinc_hann_within_the_bound(rate):
    rng = np.random.default_rng(rate + 1)
    of, nf, width, K = frontend.resample_geometry(rate, 16000)
    worst = 0.0
    for n in (1, max(1, of - 1), of, of + 1, width, K, K + 1, 4099):
        x = rng.standard_normal(n).astype(np.float32)
        got = frontend.resample_sinc_hann(x, rate, 16000)
        ref, A, k = ref64_and_bound(x, rate)
        assert k == K and got.shape == ref.shape == (-(-nf * n // of),)
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= (K + 2) * U * A).all(), (rate, n)
        worst = max(worst, float((err / np.maximum((K + 2) * U * A, 1e-300)).max()))
    print(f"{rate} -> 16000: worst err / bound = {worst:.3f}")


def test_emission_rule():
    for rate in (48000, 44100, 8000, 11025, 32000):
        of, nf, width, K = frontend.resample_geometry(rate, 16000)
        J = [frontend.resample_emitted(n, of, nf, width) for n in range(0, 3 * K + 5)]
        for n, j in enumerate(J):
            # outputs j < J(N) are exactly those of the frames whose last tap, input index i * of + width + of - 1, exists
            whole = [i for i in range(0, n + 1) if i * of + width + of - 1 < n]
            assert j == nf * len(whole), (rate, n)
            assert j <= -(-nf * n // of)                           # never more than the one-shot trim
        assert J[width + of - 1] == 0 and J[width + of] == nf
        assert all(b >= a for a, b in zip(J, J[1:]))
        # the input the next frame still needs is fewer than K samples
        for n, j in enumerate(J):
            assert n - max(0, (j // nf) * of - width) < K


class StubRing:
    """engine.Ring's surface over a rate ring that follows the emission rule (no samples, only counts)"""

    def __init__(self, capacity, rate=16000):
        self.capacity, self.rate, self.head, self.n_in = capacity, rate, 0, 0
        self.geo = frontend.resample_geometry(rate, 16000) if rate != 16000 else None

    def append(self, data):
        first, n = self.head, len(data) // 2
        if self.geo is None:
            self.head += n
        else:
            of, nf, width, _ = self.geo
            self.head += frontend.resample_emitted(self.n_in + n, of, nf, width) - frontend.resample_emitted(self.n_in, of, nf, width)
            self.n_in += n
        return first

    def close(self):
        pass


class StubEngine:
    def __init__(self):
        self.made = []

    def ring_create(self, capacity, rate=16000):
        self.made.append((capacity, rate))
        return StubRing(capacity, rate)


class StubModel:
    target_sr = 16000

    def __init__(self):
        self.models = [StubEngine()]


def test_audio_stream_maps_chunks_to_16k_ranges():
    from sonicscribe_amd.asr import AudioStream
    m = StubModel()
    st = AudioStream(m, "s", 0, buffer_seconds=2.0, margin_seconds=1.0, sampling_rate=48000)
    assert m.models[0].made == [(48000, 48000)] and st.visible == 32000            # capacity and the visible buffer count 16 kHz samples
    of, nf, width, _ = frontend.resample_geometry(48000, 16000)
    sizes = [5, 16, 1, 3072, 3072, 7, 3071, 3073] + [3072] * 40
    total, ranges = 0, []
    for k, n in enumerate(sizes):
        cid = st.add_audio_chunk(b"\0\0" * n, timestamp=float(k))
        total += n
        assert cid == k and st.ring.head == frontend.resample_emitted(total, of, nf, width)
        ranges.append((frontend.resample_emitted(total - n, of, nf, width), frontend.resample_emitted(total, of, nf, width)))
    assert ranges[0] == (0, 0) and ranges[1] == (0, 0) and ranges[2] == (0, 1)       # 5, 21, 22 samples: J = 0, 0, 1 (width + of = 22)
    for cid in range(st.oldest_chunk_id, len(sizes)):
        a, b = ranges[cid]
        assert st.chunk_samples(cid) == (a, b - a) and st.chunk_timestamp(cid) == float(cid)
    # eviction is by 16 kHz samples: a chunk leaves once it starts more than `visible` samples before the head
    assert st.oldest_chunk_id > 0
    floor = st.ring.head - st.visible
    assert ranges[st.oldest_chunk_id][0] >= floor and ranges[st.oldest_chunk_id - 1][0] < floor
    lo, hi = st.oldest_chunk_id, len(sizes) - 1
    assert st.chunk_range_samples(lo, hi) == (ranges[lo][0], ranges[hi][1] - ranges[lo][0])
    assert st.chunk_range_samples(0, hi) == st.chunk_range_samples(lo, hi)
    # a 16 kHz stream is what it was: the ring is created without a rate and a chunk is its own samples
    m16 = StubModel()
    s16 = AudioStream(m16, "s", 0, buffer_seconds=2.0, margin_seconds=1.0)
    assert m16.models[0].made == [(48000, 16000)]
    s16.add_audio_chunk(b"\0\0" * 1024); s16.add_audio_chunk(b"\0\0" * 100)
    assert s16.chunk_samples(0) == (0, 1024) and s16.chunk_samples(1) == (1024, 100)


def test_refusals_name_the_numbers():
    # of = 16001, nf = 16000, width = ceil(6 * 16001 / 15840) = 7, K = 16015: 256 240 000 coefficients, a gigabyte of fp32
    with pytest.raises(ValueError, match=r"16001 -> 16000 Hz.*16000 phases x 16015 taps = 256240000 coefficients.*limit 4194304"):
        frontend.resample_geometry(16001, 16000)
    for bad in (0, -8000):
        with pytest.raises(ValueError, match="must be positive"):
            frontend.resample_geometry(bad, 16000)
    for rate in [8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000]:
        of, nf, width, K = frontend.resample_geometry(rate, 16000)
        assert nf * K <= 291200
    # the binding refuses before it reaches the library
    from sonicscribe_amd import engine

    class NoLib:
        h = None
    with pytest.raises(ValueError, match="16001"):
        engine.Ring(NoLib(), 4096, rate=16001)


def test_file_mode_takes_a_rate_and_no_longer_says_resample():
    from sonicscribe_amd import filemode
    with pytest.raises(ValueError) as ex:
        filemode.as_pcm16(np.array([0.3], np.float32))
    assert "resample" not in str(ex.value) and "sampling_rate=" in str(ex.value)
    import inspect
    for fn in (filemode.transcribe_file, filemode.transcribe_files):
        assert inspect.signature(fn).parameters["sampling_rate"].default == 16000


def test_resample_sinc_hann_against_torchaudio():
    torchaudio = pytest.importorskip("torchaudio")
    import torch
    rng = np.random.default_rng(5)
    for rate in RATES:
        x = rng.standard_normal(4099).astype(np.float32)
        want = torchaudio.functional.resample(torch.from_numpy(x), rate, 16000).numpy()
        got = frontend.resample_sinc_hann(x, rate, 16000)
        ref, A, K = ref64_and_bound(x, rate)
        assert got.shape == want.shape
        # both are fp32 evaluations of the same K-term products over a bank built in double: each lies within the bound of ref64
        assert (np.abs(got.astype(np.float64) - want) <= 2 * (K + 2) * U * A).all(), rate
