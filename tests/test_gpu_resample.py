"""The device resampler (csrc/resample.hip) behind Engine.resample and behind the append of a rate ring (sonic_ring_create_rate).

Against the host: the derived bound of tests/test_resample.py, |got - ref64| <= (K + 2) * u * A, and for ring content
|q - 32768 * ref64| <= 0.5 + 32768 * (K + 2) * u * A (exactly the clip value where ref64 lies beyond full scale by more than that margin).
Everything else is bit for bit: one thread owns one output and sums its K taps in ascending order, so the grid, the cut of the stream into
appends, the neighbours in a buffer and the ring position cannot show.

Worst err / ((K + 2) u A) that test_one_shot_within_the_bound printed on an MI355X (reported, not a threshold): 0.26 at 8 -> 16 kHz, 0.10 at
48 kHz, 0.14 at 32 kHz, 0.15 at 16 -> 8 kHz, 0.008 at 44.1 and 0.009 at 11.025 kHz."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_resample import U, ref64_and_bound  # noqa: E402

from sonicscribe_amd import frontend, spec, synth, vad_net  # noqa: E402

pytestmark = pytest.mark.gpu

WALL = ("timestamp", "processing_time", "completed_at")


@pytest.fixture(scope="module")
def eng():
    from sonicscribe_amd.engine import Engine
    e = Engine(spec.TINY, 0, max_batch=2, max_ctx=512)
    e.load_synthetic(20260128)
    yield e
    e.close()


@pytest.fixture(scope="module")
def vad():
    from sonicscribe_amd.vad import VADProcessor
    v = VADProcessor(weights=vad_net.synthetic_weights(7, **vad_net.RESPONSIVE))
    yield v
    v.close()


def pcm_at(seed, n):
    return np.random.default_rng(seed).integers(-30000, 30000, size=n).astype(np.int16)


def quantise(y):
    """the ring's rounding of the fp32 resampler output: clip(rint(y * 32768)), the product exact in fp32"""
    return np.clip(np.rint(y.astype(np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def J(n, rate):
    of, nf, width, _ = frontend.resample_geometry(rate, 16000)
    return frontend.resample_emitted(n, of, nf, width)


# ------------------------------------------------------------------------------------------------------------------ 1. one-shot
@pytest.mark.parametrize("rates", [(48000, 16000), (44100, 16000), (8000, 16000), (11025, 16000), (32000, 16000), (16000, 8000)])
def test_one_shot_within_the_bound(eng, rates):
    in_rate, out_rate = rates
    of, nf, width, K = frontend.resample_geometry(in_rate, out_rate)
    rng = np.random.default_rng(in_rate + out_rate)
    worst = 0.0
    for n in sorted({1, max(1, of - 1), of, of + 1, width, K, K + 1, 4099}):
        for kind in ("int16", "fp32"):
            if kind == "int16":
                x = rng.integers(-32768, 32768, size=n).astype(np.int16)
                xf = x.astype(np.float64) / 32768.0
            else:
                x = rng.standard_normal(n).astype(np.float32)
                xf = x
            got = eng.resample(x, in_rate, out_rate)
            ref, A, k = ref64_and_bound(xf, in_rate, out_rate)
            assert k == K and got.dtype == np.float32 and got.shape == (-(-nf * n // of),) == ref.shape
            err, bound = np.abs(got.astype(np.float64) - ref), (K + 2) * U * A
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            worst = max(worst, ratio)
            print(f"{in_rate} -> {out_rate} n={n} {kind}: worst err / bound = {ratio:.4f}")
            assert (err <= bound).all(), (in_rate, n, kind)
    print(f"{in_rate} -> {out_rate}: worst err / ((K + 2) u A) = {worst:.4f}")
    # equal rates: Resample returns its input
    x = rng.integers(-32768, 32768, size=100).astype(np.int16)
    assert np.array_equal(eng.resample(x, out_rate, out_rate), x.astype(np.float32) / np.float32(32768.0))


# ------------------------------------------------------------------------------------------------------------------ 2. neighbours
@pytest.mark.parametrize("rate", [48000, 44100, 8000, 11025])
def test_alone_and_inside_a_longer_buffer(eng, rate):
    of, nf, width, K = frontend.resample_geometry(rate, 16000)
    x = pcm_at(rate, 3000)
    alone = eng.resample(x, rate)
    for lead_frames, tail in ((7, 5000), (301, 1)):
        # a whole number of frames in front keeps the phases; 7 * nf and 301 * nf outputs move the stream to other lanes, tiles and blocks
        big = np.concatenate([np.zeros(lead_frames * of, np.int16), x, np.zeros(tail, np.int16)])
        got = eng.resample(big, rate)[lead_frames * nf:lead_frames * nf + len(alone)]
        assert got.tobytes() == alone.tobytes(), (rate, lead_frames)
    # int16 samples and their float form s / 32768 are the same input
    assert eng.resample(x.astype(np.float32) / np.float32(32768.0), rate).tobytes() == alone.tobytes()
    # a slot of the engine shares the bank
    slot = eng.slot()
    try:
        assert slot.resample(x, rate).tobytes() == alone.tobytes()
    finally:
        slot.close()


# ------------------------------------------------------------------------------------------------------------------ 3. chunking
def cuts(n, kind, seed):
    if kind == "ones":
        return [1] * 600 + [n - 600]
    if kind == "whole":
        return [n]
    if kind == "mix":
        rng, out = np.random.default_rng(seed), []
        while sum(out) < n:
            out.append(int(min(rng.integers(1, 5001), n - sum(out))))
        return out
    out = [kind] * (n // kind)
    return out + ([n - sum(out)] if n - sum(out) else [])


@pytest.mark.parametrize("rate", [44100, 48000])
def test_chunking_does_not_show(eng, rate):
    of, nf, width, K = frontend.resample_geometry(rate, 16000)
    n = 20000
    x = pcm_at(rate + 3, n)
    total = -(-nf * n // of)
    want = quantise(eng.resample(x, rate))
    assert len(want) == total
    before_flush = None
    for kind in ("ones", 7, 1023, 3072, "whole", "mix"):
        ring = eng.ring_create(8192, rate=rate)
        try:
            pos = 0
            for c in cuts(n, kind, rate):
                first = ring.append(x[pos:pos + c])
                assert first == J(pos, rate), (kind, pos)               # the head before the call ...
                pos += c
                if c > 1 or pos % 50 == 0 or pos < 2 * K:
                    assert ring.head == J(pos, rate), (kind, pos)       # ... and after it: J(N) whatever the cut
            assert pos == n and ring.head == J(n, rate) < total
            got = ring.read(0, ring.head)
            if before_flush is None:
                before_flush = got
            assert got.tobytes() == before_flush.tobytes() == want[:len(got)].tobytes(), kind
            ring.flush()
            assert ring.head == total
            assert ring.read(0, total).tobytes() == want.tobytes(), kind
            ring.flush()                                                # nothing left to end
            assert ring.head == total
            # the next append starts a new stream with zero history, at the ring's head
            first = ring.append(x[:K + of])
            assert first == total and ring.head == total + J(K + of, rate)
            assert ring.read(total, ring.head - total).tobytes() == want[:ring.head - total].tobytes()
        finally:
            ring.close()


# ------------------------------------------------------------------------------------------------------------------ 4. wrap
def test_wrap_and_ranges_that_left(eng):
    rate, n, cap = 48000, 30000, 4096
    x = pcm_at(11, n)
    want = quantise(eng.resample(x, rate))
    ring = eng.ring_create(cap, rate=rate)
    try:
        for pos in range(0, n, 3071):
            ring.append(x[pos:pos + 3071])
        ring.flush()
        assert ring.head == len(want) == 10000
        assert ring.read(ring.head - cap, cap).tobytes() == want[-cap:].tobytes()
        assert ring.read(7000, 123).tobytes() == want[7000:7123].tobytes()
        for first, cnt in ((ring.head - cap - 1, 10), (0, 1), (ring.head - 5, 6), (-1, 1)):
            with pytest.raises(RuntimeError, match="not in the ring"):
                ring.read(first, cnt)
        # a chunk whose outputs exceed the capacity is refused, and nothing moved
        with pytest.raises(RuntimeError, match="the ring holds 4096"):
            ring.append(np.zeros(3 * (cap + 64), np.int16))
        assert ring.head == 10000
        assert ring.read(ring.head - cap, cap).tobytes() == want[-cap:].tobytes()
    finally:
        ring.close()


# ------------------------------------------------------------------------------------------------------------------ 5. clip
def test_full_scale_square_wave_clips(eng):
    rate = 8000
    of, nf, width, K = frontend.resample_geometry(rate, 16000)
    x = np.where((np.arange(2000) // 8) % 2 == 0, 32767, -32767).astype(np.int16)
    ring = eng.ring_create(4096, rate=rate)
    try:
        ring.append(x)
        ring.flush()
        q = ring.read(0, ring.head).astype(np.float64)
    finally:
        ring.close()
    ref, A, _ = ref64_and_bound(x.astype(np.float64) / 32768.0, rate)
    assert len(q) == len(ref) == 4000
    margin = 0.5 + 32768.0 * (K + 2) * U * A
    r = 32768.0 * ref
    assert (q == 32767).any() and (q == -32768).any()
    over, under = r > 32767 + margin, r < -32768 - margin
    assert over.any() and under.any()                                  # the overshoot is real: sinc ringing on a full-scale edge
    assert (q[over] == 32767).all() and (q[under] == -32768).all()
    assert (np.abs(q - np.clip(r, -32768, 32767)) <= margin).all()


# ------------------------------------------------------------------------------------------------------------------ 6. 16 kHz
def test_rate_16000_is_the_plain_ring(eng):
    a, b = eng.ring_create(4096), eng.ring_create(4096, rate=16000)
    try:
        pos = 0
        for c in [1, 1000, 4096, 3, 2047, 0, 4000]:
            x = pcm_at(100 + c, c)
            assert a.append(x) == b.append(x) == pos
            pos += c
            assert a.head == b.head == pos
        b.flush(); a.flush()
        assert a.head == b.head == pos
        assert a.read(pos - 4096, 4096).tobytes() == b.read(pos - 4096, 4096).tobytes()
        tail = np.concatenate([pcm_at(100 + c, c) for c in [2047, 0, 4000]])[-4096:]
        assert b.read(pos - 4096, 4096).tobytes() == tail.tobytes()
        with pytest.raises(RuntimeError):
            b.append(np.zeros(4097, np.int16))                         # an oversized chunk, as before
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------ 7. downstream
@pytest.fixture(scope="module")
def model():
    from sonicscribe_amd.asr import ASRModel
    m = ASRModel.from_synthetic(spec.TINY, device="cuda:0", max_batch=8, max_ctx=1024)
    yield m
    m.close()


def speechy(seed, n16, rate):
    """synth_pcm bursts between silences longer than the VAD's 1 s, drawn at 16 kHz and held for rate / 16000 samples: int16 at `rate`"""
    x = np.zeros(n16, np.float64)
    for k, (a, b) in enumerate([(0.5, 3.0), (4.6, 8.2), (10.0, 11.5)]):
        a, b = int(a * 16000), min(n16, int(b * 16000))
        if b > a:
            x[a:b] = synth.synth_pcm(seed + k, b - a) * 0.8
    idx = (np.arange(int(n16 * rate / 16000)) * 16000 // rate).astype(np.int64)
    return np.rint(x[idx]).astype(np.int16)


def test_stream_at_48k_decodes_what_the_ring_holds(model):
    x = speechy(40, 6 * 16000, 48000)
    st = model.open_stream("rate-session", buffer_seconds=10.0, margin_seconds=5.0, sampling_rate=48000)
    try:
        ids = [st.add_audio_chunk(x[p:p + 3072].tobytes()) for p in range(0, len(x), 3072)]
        assert st.ring.head == J(len(x), 48000)
        first, n = st.chunk_range_samples(ids[5], ids[-2])
        assert first == J(5 * 3072, 48000) and first + n == J((len(ids) - 1) * 3072, 48000)
        got = st.submit_chunks(ids[5], ids[-2], max_new_tokens=24).result()
        host = st.ring.read(first, n).astype(np.float32) / np.float32(32768.0)
        assert got == model.transcribe(host[None, :], 16000, max_new_tokens=24)
        assert got == st.submit_samples(first, n, max_new_tokens=24).result()
    finally:
        st.close()


def test_vad_reads_a_rate_ring_in_place(eng, vad):
    x = speechy(50, 5 * 16000, 44100)
    ring = eng.ring_create(6 * 16000, rate=44100)
    try:
        ring.append(x[:50000]); ring.append(x[50000:]); ring.flush()
        n = ring.head
        assert n == -(-160 * len(x) // 441)
        back = ring.read(0, n)
        for a, cnt in ((0, n), (777, n - 1000)):
            got = vad.probs_rings(eng, [[(ring, a, cnt)]])[0]
            assert np.array_equal(got, vad.probs([back[a:a + cnt]])[0])
    finally:
        ring.close()


def strip(rec):
    return {k: v for k, v in rec.items() if k not in WALL}


def test_file_mode_at_44100(model, vad):
    from sonicscribe_amd.asr import ASRModel
    x = speechy(60, 12 * 16000, 44100)
    ring = model.models[0].ring_create(13 * 16000, rate=44100)
    try:
        ring.append(x); ring.flush()
        at16 = ring.read(0, ring.head)
    finally:
        ring.close()
    assert len(at16) == -(-160 * len(x) // 441)
    other = ASRModel.from_synthetic(spec.TINY, device="cuda:0", max_batch=8, max_ctx=1024, continuous=False)
    try:
        for m in (model, other):
            want = [strip(r) for r in m.transcribe_file(at16, vad, max_new_tokens=24, filename="f")]
            got = [strip(r) for r in m.transcribe_file(x, vad, max_new_tokens=24, filename="f", sampling_rate=44100)]
            assert got == want
            assert got[0]["file_size"] == 2 * len(at16) and got[0]["total_duration"] == round(len(at16) / 16000, 2)
            assert sum(r["type"] == "segment_result" for r in got) >= 1
            flt = [strip(r) for r in m.transcribe_files([x.astype(np.float32) / np.float32(32768.0)], vad, max_new_tokens=24, filenames=["f"],
                                                         sampling_rate=44100)[0]]
            assert flt == want
            assert len(getattr(m.models[0], "_rings", [])) == 0
    finally:
        other.close()


# ------------------------------------------------------------------------------------------------------------------ 8. lifetime, refusals
def test_refusals_are_host_side_statuses(eng):
    lib = eng.lib
    for rate, text in ((0, "positive"), (-8000, "positive"), (16001, "256240000 coefficients")):
        h = C.c_void_p()
        assert lib.sonic_ring_create_rate(eng.h, 4096, rate, C.byref(h)) == 1 and not h.value
        assert text in lib.sonic_last_error(eng.h).decode() and str(rate) in lib.sonic_last_error(eng.h).decode()
        x, out, n_out = np.zeros(8, np.int16), np.zeros(64, np.float32), C.c_int64()
        rc = lib.sonic_resample(eng.h, x.ctypes.data_as(C.c_void_p), None, 8, rate, 16000, out.ctypes.data_as(C.c_void_p), 64, C.byref(n_out))
        assert rc == 1 and text in lib.sonic_last_error(None).decode()
        with pytest.raises(ValueError):
            eng.ring_create(4096, rate=rate)
        with pytest.raises(ValueError):
            eng.resample(x, rate)
    # both inputs, a short output buffer
    x, xf, out, n_out = np.zeros(64, np.int16), np.zeros(64, np.float32), np.zeros(4, np.float32), C.c_int64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.sonic_resample(eng.h, p(x), p(xf), 64, 48000, 16000, p(out), 4, C.byref(n_out)) == 1
    assert lib.sonic_resample(eng.h, p(x), None, 64, 48000, 16000, p(out), 4, C.byref(n_out)) == 1 and n_out.value == 22
    assert "do not fit" in lib.sonic_last_error(None).decode()
    assert eng.resample(np.zeros(0, np.int16), 48000).shape == (0,)


def test_memory_and_lifetime():
    from sonicscribe_amd.engine import Engine
    e = Engine(spec.TINY, 0, max_batch=2, max_ctx=512)
    try:
        e.load_synthetic(20260128)
        of, nf, width, K = frontend.resample_geometry(12000, 16000)
        base = e.memory_info()[0]
        plain = e.ring_create(4096)
        d_plain = e.memory_info()[0] - base
        assert d_plain == 4096 * 2
        r1 = e.ring_create(4096, rate=12000)
        d1 = e.memory_info()[0] - base - d_plain
        r2 = e.ring_create(4096, rate=12000)
        d2 = e.memory_info()[0] - base - d_plain - d1
        assert d1 - d2 == nf * K * 4                                   # the bank: uploaded once, shared by the second ring
        assert d2 >= 4096 * 2 + 2 * K                                  # the ring and its carry (and the staging of a chunk)
        s = e.slot()
        r3 = s.ring_create(4096, rate=12000)                           # a slot's ring: charged to the owner, the owner's bank
        assert e.memory_info()[0] - base - d_plain - d1 == 2 * d2
        for r in (plain, r1, r2, r3):
            r.close()
        assert e.memory_info()[0] == base + nf * K * 4                 # the bank stays with the engine
        live = e.ring_create(4096, rate=12000)
        live.append(np.zeros(100, np.int16))
    finally:
        e.close()
    # the engine is gone and took its rings along: every call on the ring is refused on the host
    for call in (lambda: live.append(np.zeros(10, np.int16)), lambda: live.flush(), lambda: live.read(0, 1)):
        with pytest.raises(RuntimeError):
            call()


def test_device_entry_against_torchaudio(eng):
    torchaudio = pytest.importorskip("torchaudio")
    import torch
    rng = np.random.default_rng(9)
    for rate in (8000, 11025, 32000, 44100, 48000):
        x = rng.standard_normal(4099).astype(np.float32)
        want = torchaudio.functional.resample(torch.from_numpy(x), rate, 16000).numpy()
        got = eng.resample(x, rate)
        ref, A, K = ref64_and_bound(x, rate)
        assert got.shape == want.shape
        assert (np.abs(got.astype(np.float64) - want) <= 2 * (K + 2) * U * A).all(), rate
