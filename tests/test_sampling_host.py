"""Temperature sampling and the fallback ladder, host side: the noise definition's known answers, the compression ratio, the ladder against a
stub `submit`, the range checks, the surface."""
import os
import re
import threading
from concurrent.futures import Future

import numpy as np
import pytest

from sonicscribe_amd import engine, fallback, sampling
from sonicscribe_amd.fallback import FallbackPolicy, compression_ratio, decode_with_fallback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answers():
    assert _hex(sampling.philox4x32([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(sampling.philox4x32([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(sampling.philox4x32([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # batched: one call, rows broadcast against one key
    got = sampling.philox4x32([[0, 0, 0, 0], [0xFFFFFFFF] * 4], [[0, 0], [0xFFFFFFFF] * 2])
    assert _hex(got[0]) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8" and _hex(got[1]) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_uniforms_and_noise():
    u = sampling.uniforms(0, 0, 4)
    assert np.allclose(u, [0.39904648, 0.88052016, 0.73571283, 0.6054818], rtol=0, atol=5e-9)
    # every value is a 23-bit count plus one half, exact in fp32, strictly inside (0, 1): the two ends included
    for k in (0, (1 << 23) - 1):
        v = (k + 0.5) * 2.0 ** -23
        assert float(np.float32(v)) == v and 0.0 < v < 1.0
    big = sampling.uniforms(0x123456789ABCDEF0, 1000, 59264)
    assert np.array_equal(big.astype(np.float32).astype(np.float64), big) and big.min() > 0 and big.max() < 1
    g = sampling.gumbel_noise(0x123456789ABCDEF0, 1000, 59264)
    assert np.isfinite(g).all() and g.min() > -2.82 and g.max() < 16.65
    # word i & 3 of group i >> 2 belongs to id i; the step is the counter's second word; the seed's halves are the key
    w = sampling.philox4x32([5, 7, 0, 0], [0x9ABCDEF0, 0x12345678])
    assert np.array_equal(sampling.uniforms(0x123456789ABCDEF0, 7, 59264)[20:24], ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23)
    assert (1 + 16.64) * 1.5 * 2.0 ** -23 <= sampling.EPS_G < 1e-4           # the derivation of DESIGN.md 6.6, and the issue's ceiling


def test_sample_reference():
    s = (0.5 * np.arange(16) - 4).astype(np.float32)
    assert sampling.sample_reference(s, 0.0, 5, 3) == 15                       # t = 0: the argmax, whatever the seed
    y = sampling.perturbed(s, 2.0, 11, 0)
    assert sampling.sample_reference(s, 2.0, 11, 0) == int(np.argmax(y))
    s2 = s.copy(); s2[:] = -np.inf
    assert sampling.sample_reference(s2, 1.0, 0, 0) == 0                       # all banned: the first of equal values
    # the definition's own distribution (the figures the GPU test's bound is judged against): chi-square of 4096 seeds against softmax(s / 2)
    p = np.exp(s.astype(np.float64) / 2); p /= p.sum()
    cnt = np.zeros(16)
    for seed in range(4096):
        cnt[sampling.sample_reference(s, 2.0, seed, 0)] += 1
    e = p * 4096
    assert e.min() > 21.7 and abs(((cnt - e) ** 2 / e).sum() - 15.99) < 0.01


def test_compression_ratio():
    rep = "the cat sat on the mat. " * 40
    var = "A quick brown fox jumps over the lazy dog while seven wizards quietly box."
    assert compression_ratio(rep) > 2.4 > compression_ratio(var) > 0
    import zlib
    assert compression_ratio(rep) == len(rep.encode()) / len(zlib.compress(rep.encode()))
    assert compression_ratio("") == 0.0
    assert compression_ratio("héllo wörld " * 30) == len(("héllo wörld " * 30).encode("utf-8")) / len(zlib.compress(("héllo wörld " * 30).encode("utf-8")))


class _Res:
    def __init__(self, text, avg_logprob):
        self.text, self.avg_logprob = text, avg_logprob


def _stub(results, log):
    """submit(temperature, seed, **kw) that completes at once with the next canned result"""
    it = iter(results)

    def submit(temperature, seed, **kw):
        log.append((temperature, seed, kw))
        f = Future()
        f.set_result(next(it))
        return f
    return submit


REPEAT = "la la la la " * 50
GOOD = "A quick brown fox jumps over the lazy dog."


def test_ladder_stops_at_the_first_pass():
    log = []
    tables = object()
    fut = decode_with_fallback(_stub([_Res(REPEAT, -0.2), _Res(GOOD, -1.5), _Res(GOOD, -0.3), _Res(GOOD, -0.1)], log), FallbackPolicy(), seed=77, tables=tables, prompt=[1, 2])
    res = fut.result(timeout=10)
    assert [l[0] for l in log] == [0.0, 0.2, 0.4]                             # ratio too high, then log-probability too low, then a pass
    assert res.attempts == 3 and res.temperature == 0.4 and res.text == GOOD and res.compression_ratio == compression_ratio(GOOD)
    for _, seed, kw in log:                                                    # the seed and the tables reach every attempt unchanged
        assert seed == 77 and kw["tables"] is tables and kw["prompt"] == [1, 2]


def test_ladder_returns_the_last_attempt_when_all_fail():
    log = []
    pol = FallbackPolicy()
    results = [_Res(REPEAT, -2.0 - k) for k in range(len(pol.temperatures))]
    res = decode_with_fallback(_stub(results, log), pol, seed=1).result(timeout=10)
    assert len(log) == 6 and res is results[-1] and res.attempts == 6 and res.temperature == 1.0 and res.compression_ratio > 2.4
    assert [l[0] for l in log] == [0.0, 0.2, 0.4, 0.6, 0.8, 1.0]


def test_ladder_ignores_thresholds_set_to_none():
    log = []
    res = decode_with_fallback(_stub([_Res(REPEAT, -0.5)], log), FallbackPolicy(compression_ratio_threshold=None), seed=0).result(timeout=10)
    assert res.attempts == 1 and len(log) == 1                                 # the ratio is not looked at
    log = []
    res = decode_with_fallback(_stub([_Res(GOOD, -9.0)], log), FallbackPolicy(logprob_threshold=None), seed=0).result(timeout=10)
    assert res.attempts == 1 and len(log) == 1                                 # nor the log-probability
    log = []
    res = decode_with_fallback(_stub([_Res(REPEAT, -9.0)], log), FallbackPolicy(compression_ratio_threshold=None, logprob_threshold=None), seed=0).result(timeout=10)
    assert res.attempts == 1 and res.temperature == 0.0
    assert not FallbackPolicy().failed(2.4, -1.0) and FallbackPolicy().failed(2.41, 0.0) and FallbackPolicy().failed(0.0, -1.01)      # strictly above / below
    assert not FallbackPolicy().failed(1.0, float("nan"))                     # nothing emitted: no average to judge


def test_ladder_errors_and_worker_thread():
    def boom(temperature, seed, **kw):
        raise RuntimeError("engine closed")
    with pytest.raises(RuntimeError, match="engine closed"):
        decode_with_fallback(boom, FallbackPolicy(), seed=0).result(timeout=10)

    def failing(temperature, seed, **kw):
        f = Future(); f.set_exception(ValueError("bad request")); return f
    with pytest.raises(ValueError, match="bad request"):
        decode_with_fallback(failing, FallbackPolicy(), seed=0).result(timeout=10)
    # with a Retrier the next attempt is submitted by its thread - not by the thread that completes the future, not by the caller
    r = fallback.Retrier("test-fallback")
    threads, pending = [], []

    second = threading.Event()

    def submit(temperature, seed, **kw):
        threads.append(threading.current_thread().name)
        f = Future(); pending.append(f)
        if len(pending) == 2:
            second.set()
        return f
    fut = decode_with_fallback(submit, FallbackPolicy((0.0, 0.5)), seed=3, retrier=r)
    assert len(pending) == 1 and not fut.done()                                # the caller was not held
    pending[0].set_result(_Res(REPEAT, -0.1))                                  # completes on THIS thread; the retry must not be submitted from it
    assert second.wait(30)
    assert len(pending) == 2 and threads == [threading.current_thread().name, "test-fallback"]
    pending[1].set_result(_Res(GOOD, -0.1))
    res = fut.result(timeout=10)
    assert res.attempts == 2 and res.temperature == 0.5
    r.close()


def test_range_refusals():
    for ok in (0, 0.0, 1e-3, 0.2, 1.0, 100.0):
        assert sampling.check_temperature(ok) == float(ok)
    for bad in (-0.1, 5e-4, 100.5, float("nan"), float("inf"), -float("inf"), "hot", None):
        with pytest.raises(ValueError, match="temperature"):
            sampling.check_temperature(bad)
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError, match="seed"):
            sampling.check_seed(bad)
    assert sampling.check_seed((1 << 64) - 1) == (1 << 64) - 1
    assert sampling.temperatures(0.4) == ((0.4,), False) and sampling.temperatures([0.0, 0.5]) == ((0.0, 0.5), True)
    with pytest.raises(ValueError, match="temperature"):
        sampling.temperatures([])
    with pytest.raises(ValueError, match="temperature"):
        FallbackPolicy((0.0, 200.0))
    t, s = engine.pack_request_sampling([None, (0.5, 7), (0.0, (1 << 64) - 1)])
    assert t.dtype == np.float32 and s.dtype == np.uint64 and t.tolist() == [0.0, 0.5, 0.0] and s.tolist() == [0, 7, (1 << 64) - 1]
    with pytest.raises(ValueError, match="temperature"):
        engine.pack_request_sampling([(1e-4, 0)])
    pol = FallbackPolicy()
    assert pol.temperatures == (0.0, 0.2, 0.4, 0.6, 0.8, 1.0) and pol.compression_ratio_threshold == 2.4 and pol.logprob_threshold == -1.0


def test_surface_and_model_refusals():
    from sonicscribe_amd import asr
    names = ("sonic_set_request_sampling", "sonic_dispatch_submit", "sonic_test_greedy_sample")
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    assert "int32_t sampled; float temperature; uint64_t seed;" in hdr                      # the dispatcher's way: fields of sonic_dispatch_request
    assert [f for f, _ in engine.DispatchRequest._fields_][14:17] == ["sampled", "temperature", "seed"]
    for n in names:
        assert re.search(r"SONIC_API int " + n + r"\(", hdr) and n in engine.EXPORTS
    assert all(hasattr(engine.Engine, m) for m in ("set_request_sampling", "test_greedy_sample"))
    m = asr.ASRModel.__new__(asr.ASRModel)                                     # no device: only the surface's own checks
    assert m._request_sampling() is None
    for kw in ({"temperature": 0.5}, {"seed": 3}, {"temperature": (0.0, 0.2)}):
        with pytest.raises(ValueError, match="sampling"):
            m._request_sampling(**kw)
    m.sampling, m._default_temperature, m._default_seed = True, 0.0, 5
    CS = sampling.CallSampling
    assert m._request_sampling() == CS((0.0,), False, 5, (0, 1.0, 0.0)) and m._request_sampling(0.3, 9) == CS((0.3,), False, 9, (0, 1.0, 0.0))
    assert m._request_sampling((0.0, 0.4)) == CS(temperatures=(0.0, 0.4), ladder=True, seed=5, cut=(0, 1.0, 0.0))
    with pytest.raises(ValueError, match="ladder"):
        m._request_sampling((0.0, 0.4), ladder_ok=False)
    with pytest.raises(ValueError, match="temperature"):
        m._request_sampling(-1.0)
    m.bulk = True
    with pytest.raises(ValueError, match="bulk"):
        m._request_sampling(0.5)
    t = asr.Transcription(REPEAT, [1, 2], [-0.5, -1.5], 0.6)
    assert t.temperature == 0.6 and t.attempts == 1 and t.compression_ratio == compression_ratio(REPEAT) and t.avg_logprob == -1.0


def test_dispatchers_carry_the_values_and_bulk_refuses():
    from sonicscribe_amd.dispatch import _BulkReplica, Request
    r = Request([np.zeros(16, np.int16)], [1], 4, sampling=(0.5, 7))
    assert r.sampling == (0.5, 7) and Request([np.zeros(16, np.int16)], [1], 4).sampling is None
    bulk = _BulkReplica.__new__(_BulkReplica)
    bulk.cv, bulk.stop, bulk.q = threading.Condition(), False, []
    with pytest.raises(ValueError, match="bulk"):
        bulk.put(r)
