"""top_k / top_p / min_p on the host: the numpy restatement in sonicscribe_amd/sampling.py against HF's own TopK / TopP / MinP warpers chained in
that order, its tie rules and edge rows, the range checks by name, the calls Engine makes for pairs and for 5-tuples (on a recording library), and the pinned
counts of the C ABI."""
import math

import numpy as np
import pytest

from concurrent.futures import Future

import abi_pins
from sonicscribe_amd import asr, engine, fallback, reqvalues, sampling, spec
from sonicscribe_amd.dispatch import Request, _BulkReplica

NEG = float("-inf")


# ------------------------------------------------------------------------------------------ the reference against HF
def _hf_kept(y, k, p, m):
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    s = torch.tensor(np.asarray(y, np.float64))[None]
    ids = torch.zeros((1, 1), dtype=torch.long)
    if k:
        s = lp.TopKLogitsWarper(top_k=int(k))(ids, s)
    if p < 1.0:
        s = lp.TopPLogitsWarper(top_p=float(p))(ids, s)
    if m > 0.0:
        s = lp.MinPLogitsWarper(min_p=float(m))(ids, s)
    return set(np.flatnonzero(np.isfinite(s[0].numpy())).tolist())


@pytest.mark.parametrize("V", [20, 1000])
@pytest.mark.parametrize("params", [(5, 1.0, 0.0), (0, 0.9, 0.0), (0, 1.0, 0.05), (50, 0.9, 0.05), (3, 0.5, 0.3), (0, 0.3, 0.0), (7, 0.999, 0.001)])
def test_reference_against_hf_warpers(V, params):
    """inputs with distinct values and no cumulative mass within 1e-4 of the top_p threshold (both asserted): the kept sets are equal"""
    k, p, m = params
    rng = np.random.default_rng(5 * V + int(1000 * p))
    for trial in range(6):
        s = (rng.standard_normal(V) * 3.0).astype(np.float32)
        t = (0.5, 1.0, 1.7)[trial % 3]
        y = sampling.quotient(s, t)
        assert len(np.unique(y)) == V
        n_k = sampling.truncation_counts(y, k, 1.0, 0.0)[0]
        ys = np.sort(y.astype(np.float64))[::-1][:n_k]
        w = np.exp(ys - ys[0])
        c = np.cumsum(w) / w.sum()
        assert p == 1.0 or np.abs(c - p).min() > 1e-4
        pm = np.exp(y.astype(np.float64) - float(y.max()))
        assert m == 0.0 or np.abs(pm / m - 1.0).min() > 1e-5      # (and no probability ratio within rounding of min_p, where the log-domain compare may differ)
        kept = sampling.truncation_kept(s, t, k, p, m)
        assert set(int(i) for i in kept) == _hf_kept(y, min(k, V), p, m), (V, params, trial)


def test_tie_rules_and_edge_rows():
    y = np.array([1.0, 3.0, 2.0, 2.0, 0.5, 2.0, NEG, NEG], np.float32)
    # top_k keeps the ties at the k-th value (HF's `scores < kth`)
    assert sampling.truncation_counts(y, 2, 1.0, 0.0)[0] == 4 and sampling.truncation_kept(y, 1.0, 2).tolist() == [1, 2, 3, 5]
    # k beyond the number of finite scores removes nothing (the k-th value is -inf, and nothing is below it); k equal to it drops what was -inf already
    assert sampling.truncation_counts(y, 6, 1.0, 0.0)[0] == 6 and sampling.truncation_counts(y, 7, 1.0, 0.0)[0] == 8 and sampling.truncation_counts(y, 100, 1.0, 0.0)[0] == 8
    # top_p: ties at the boundary go by the lower id.  masses 1, 3 x e^-1, ...: in front of the three ties 0.405, 0.554, 0.703 of the total 2.468
    assert sampling.truncation_kept(y, 1.0, 0, 0.6).tolist() == [1, 2, 3] and sampling.truncation_kept(y, 1.0, 0, 0.5).tolist() == [1, 2]
    # top_p so small that one id stays: rank 0 is always kept
    assert sampling.truncation_kept(y, 1.0, 0, 1e-6).tolist() == [1] and sampling.truncation_kept(y, 0.01, 0, 1e-30).tolist() == [1]
    # min_p = 1 keeps the maximum's ties; the threshold itself is kept
    assert sampling.truncation_kept(np.array([2.0, 1.0, 2.0], np.float32), 1.0, 0, 1.0, 1.0).tolist() == [0, 2]
    thr = np.float32(np.float32(3.0) + sampling.log_min_p(0.25))
    assert sampling.truncation_kept(np.array([3.0, thr, np.nextafter(thr, np.float32(-9))], np.float32), 1.0, 0, 1.0, 0.25).tolist() == [0, 1]
    # the shortest of the three prefixes; top_p runs over the top_k survivors (masses 1, 3 x e^-1 of 2.104: in front of the ties 0.475, 0.650), min_p over all
    assert sampling.truncation_counts(y, 2, 0.6, 0.5) == (4, 2, 1) and sampling.truncation_kept(y, 1.0, 2, 0.6, 0.5).tolist() == [1]
    assert sampling.truncation_kept(y, 1.0, 2, 0.6, 0.0).tolist() == [1, 2] and sampling.truncation_kept(y, 1.0, 0, 0.6, 0.3).tolist() == [1, 2, 3]
    # a row of -inf only keeps everything, and the token is 0
    inf = np.full(12, NEG, np.float32)
    assert sampling.truncation_counts(inf, 3, 0.5, 0.5) == (12, 12, 12) and sampling.sample_truncated(inf, 0.7, 1, 0, 3, 0.5, 0.5) == 0
    # t = 0 ignores the three parameters; all off is sample_reference
    s = np.random.default_rng(1).standard_normal(300).astype(np.float32)
    assert sampling.sample_truncated(s, 0.0, 9, 4, 1, 0.1, 0.9) == int(np.argmax(s))
    assert all(sampling.sample_truncated(s, 1.0, sd, 3) == sampling.sample_reference(s, 1.0, sd, 3) for sd in range(20))
    # a draw under top_k = 4 always lies among the 4 best, and is not always the best
    best = set(np.argsort(-s)[:4].tolist())
    draws = [sampling.sample_truncated(s, 1.5, sd, 0, 4) for sd in range(40)]
    assert set(draws) <= best and len(set(draws)) > 1
    # -0.0 counts as +0.0
    assert sampling.truncation_kept(np.array([-0.0, 0.0, -1.0], np.float32), 1.0, 1).tolist() == [0, 1]


def test_range_checks_by_name():
    for bad in (-1, 1.5, True, None, 2 ** 31, float("nan")):
        with pytest.raises(ValueError, match="top_k"):
            sampling.check_truncation(bad, 0.9, 0.0)
    for bad in (0.0, -0.1, 1.0001, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="top_p"):
            sampling.check_truncation(0, bad, 0.0)
    for bad in (-1e-9, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_p"):
            sampling.check_truncation(0, 0.9, bad)
    assert sampling.check_truncation() == (0, 1.0, 0.0) and sampling.check_truncation(50, 0.9, 0.05) == (50, 0.9, 0.05)
    assert sampling.pack_truncation([(50, 0.9, 0.05), (0, 1.0, 0.0)]).tolist() == [[50.0, np.float32(0.9), np.float32(0.05)], [0.0, 1.0, 0.0]]
    assert sampling.log_min_p(0.0) == NEG and sampling.log_min_p(1.0) == 0.0 and sampling.log_min_p(0.5) == np.float32(math.log(0.5))
    assert 2e-5 < sampling.EPS_MASS < 1e-4


# ------------------------------------------------------------------------------------------ Engine: what is armed, and when
class RecordingLib:
    """stands in for the ctypes library: every function records its name and arguments and returns 0"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


def _engine():
    e = engine.Engine.__new__(engine.Engine)
    e.lib, e.h, e.dims, e.owner, e._slots = RecordingLib(), 1, spec.TINY, None, []
    return e


def _names(e):
    return [(n, a[1]) if n in ("sonic_set_option", "sonic_load_tensor") else n for n, a in e.lib.calls]


def _consume(e, how, **kw):
    if how == "prefill":
        return e.prefill([[1, 2, 3], [1, 2]], [4, 4], [0, 1, 2], **kw)
    return e.transcribe_batch([np.zeros(1600, np.int16)] * 2, [[1, 2, 3], [1, 2]], [4, 4], req_win=[0, 1, 2], **kw)


ENTRY = {"host": "sonic_transcribe_batch", "prefill": "sonic_prefill"}
TRUNC = ("sonic_load_tensor", b"request_truncation")


@pytest.mark.parametrize("how", ["host", "prefill"])
def test_pairs_make_todays_calls_and_5_tuples_arm_the_tensor_right_ahead_of_the_consuming_call(how):
    e = _engine()
    try:
        _consume(e, how, request_sampling=[(0.5, 1), None])
        assert _names(e) == ["sonic_set_request_sampling", ENTRY[how]]                      # pairs: exactly today's calls
        e.lib.calls.clear()
        _consume(e, how, request_sampling=[(0.5, 1, 50, 0.9, 0.05), None])
        assert _names(e) == ["sonic_set_request_sampling", TRUNC, ENTRY[how]]               # ... directly ahead of the consuming call
        shape = e.lib.calls[1][1][4]
        assert (shape[0], shape[1]) == (2, 3) and e.lib.calls[1][1][3] == engine.DTYPE_F32 and e.lib.calls[1][1][5] == 2
        e.lib.calls.clear()
        _consume(e, how, request_sampling=[(0.5, 1, 50, 0.9, 0.05), (0.7, 2)], request_draft=[None, None])
        assert _names(e) == ["sonic_set_request_sampling", ("sonic_load_tensor", b"request_draft"), TRUNC, ENTRY[how]]
        for bad in ([(0.5, 1, 50, 1.5, 0.0), None], [(0.5, 1, -2, 0.9, 0.0), None], [(0.5, 1, 0, 0.9, float("nan")), None], [(0.5, 1, 3), None]):
            e.lib.calls.clear()
            with pytest.raises(ValueError):
                _consume(e, how, request_sampling=bad)
            assert e.lib.calls == []                                                        # validated before anything is armed
        # a per-row list of the wrong length under forks: nothing is armed
        e.lib.calls.clear()
        with pytest.raises(ValueError, match="request_sampling"):
            _consume(e, how, request_sampling=[(0.5, 1, 50, 0.9, 0.05), None], forks=[2, 1])
        assert e.lib.calls == []
        e.lib.calls.clear()
        e.max_batch = 8
        _consume(e, how, request_sampling=[(0.5, 1, 50, 0.9, 0.05), None, (0.5, 2)], forks=[2, 1])
        assert _names(e) == ["sonic_set_request_sampling", ("sonic_load_tensor", b"request_forks"), TRUNC, ENTRY[how]]
    finally:
        e.h = None


def test_set_request_sampling_passes_the_rows():
    e = _engine()
    try:
        e.set_request_sampling([(0.5, 1), None])
        assert _names(e) == ["sonic_set_request_sampling"]
        e.lib.calls.clear()
        e.set_request_sampling([(0.5, 1, 5, 0.5, 0.25), None, (0.0, 3, 0, 1.0, 0.0)])
        assert _names(e) == ["sonic_set_request_sampling", TRUNC]
        t, s = engine.pack_request_sampling([(0.5, 1), None])
        assert t.tolist() == [0.5, 0.0] and s.tolist() == [1, 0]
        packed = engine.pack_request_sampling([(0.5, 1, 5, 0.5, 0.25), None])
        assert len(packed) == 3 and packed[2].dtype == np.float32 and packed[2].tolist() == [[5.0, 0.5, 0.25], [0.0, 1.0, 0.0]]
    finally:
        e.h = None


# ------------------------------------------------------------------------------------------ ASRModel's policy on stub handles; the schedulers' requests
class StubDispatcher:
    """greedy and sampled attempts alike: ids [7, 8], log-probabilities -2 each (an average every threshold above -2 fails)"""
    def __init__(self):
        self.calls = []

    def home(self, session):
        return 0

    def submit(self, windows, prompt, max_new, **kw):
        self.calls.append(kw)
        f = Future()
        lp = np.asarray([-2.0, -2.0], np.float32)
        f.set_result((np.asarray([7, 8], np.int32), lp) if kw.get("want_logprobs") else np.asarray([7, 8], np.int32))
        return f


class StubForkEngine:
    """a forked run: the row of seed s emits [s % 1000] with log-probability -2"""
    def __init__(self):
        self.calls = []

    def transcribe_batch(self, segs, prompts, max_new, req_win=None, want_logprobs=False, request_sampling=None, forks=None, **kw):
        self.calls.append(list(request_sampling))
        return [np.asarray([v[1] % 1000], np.int32) for v in request_sampling], None, [np.asarray([-2.0], np.float32) for _ in request_sampling]


def _model(best_of=1, sampling_on=True, cut=(0, 1.0, 0.0)):
    m = asr.ASRModel.__new__(asr.ASRModel)                                 # no device: the policy alone
    m.best_of, m._max_batch, m.sampling = best_of, 8, sampling_on
    m._default_temperature, m._default_seed, m._default_cut = 0.0, 0, cut
    m.prompt = asr.SyntheticPrompt(spec.TINY)
    m.compression_ratio_threshold, m.logprob_threshold = None, -1.0
    m._dispatcher, m._retrier = StubDispatcher(), fallback._Inline
    m._fork_engines = [StubForkEngine()] if best_of > 1 else []
    m._fork_workers, m._fork_next = [fallback._Inline for _ in m._fork_engines], 0
    return m


WIN = [np.zeros(1600, np.int16)]


def test_model_resolves_the_call_over_the_defaults():
    m = _model(cut=(50, 0.9, 0.0))
    try:
        CS, values = sampling.CallSampling, lambda samp: reqvalues.CallValues(None, samp, None, None)
        assert m._request_sampling(0.7, 3) == CS((0.7,), False, 3, (50, 0.9, 0.0))                      # the constructor's defaults
        assert m._request_sampling(0.7, 3, cut=(None, 0.5, 0.1)) == CS((0.7,), False, 3, (50, 0.5, 0.1))  # a call overrides what it states
        assert m._request_sampling(0.7, 3, cut=(0, 1.0, None)) == CS((0.7,), False, 3, (0, 1.0, 0.0))    # all off: the cut that cuts nothing, and pairs downstream
        for bad, name in (((-1, None, None), "top_k"), ((None, 0.0, None), "top_p"), ((None, None, float("nan")), "min_p")):
            with pytest.raises(ValueError, match=name):
                m._request_sampling(0.7, 3, cut=bad)
        # what the schedulers are told: a pair at temperature 0 (greedy rows ignore the cut), the 5-tuple above it
        assert reqvalues.submit_keywords(values(m._request_sampling(0.7, 3))) == {"sampling": (0.7, 3, 50, 0.9, 0.0)}
        assert reqvalues.submit_keywords(values(m._request_sampling(0.0, 3))) == {"sampling": (0.0, 3)}
        assert reqvalues.submit_keywords(values(_model()._request_sampling(0.7, 3))) == {"sampling": (0.7, 3)}
    finally:
        m.__dict__.clear()


def test_every_rung_above_zero_and_every_fork_repeat_the_values():
    m = _model(cut=(50, 0.9, 0.05))
    try:
        tr = m._dispatch(WIN, [1, 2, 3], 4, True, reqvalues.CallValues(samp=m._request_sampling((0.0, 0.4, 0.8), 9))).result(timeout=5)      # every attempt averages -2: all three are tried
        assert [c["sampling"] for c in m._dispatcher.calls] == [(0.0, 9), (0.4, 9, 50, 0.9, 0.05), (0.8, 9, 50, 0.9, 0.05)]
        assert (tr.attempts, tr.temperature, tr.top_k, tr.top_p, tr.min_p) == (3, 0.8, 50, 0.9, 0.05)
        one = m._dispatch(WIN, [1, 2, 3], 4, True, reqvalues.CallValues(samp=m._request_sampling(0.0, 9))).result(timeout=5)
        assert (one.top_k, one.top_p, one.min_p) == (0, 1.0, 0.0)                                                      # temperature 0: the values were not used
    finally:
        m.__dict__.clear()
    m = _model(best_of=3, cut=(0, 1.0, 0.0))
    try:
        samp = m._request_sampling((0.0, 0.8), 41, cut=(5, None, None))
        tr = m._dispatch(WIN, [1, 2, 3], 4, True, reqvalues.CallValues(samp=samp, best_of=3)).result(timeout=5)
        assert m._dispatcher.calls[0]["sampling"] == (0.0, 41) and len(m._dispatcher.calls) == 1
        assert m._fork_engines[0].calls == [[(0.8, 41, 5, 1.0, 0.0), (0.8, 42, 5, 1.0, 0.0), (0.8, 43, 5, 1.0, 0.0)]]     # the forks differ in their seeds alone
        assert (tr.best_of, tr.top_k, tr.top_p, tr.min_p) == (3, 5, 1.0, 0.0)
    finally:
        m.__dict__.clear()


def test_refusals_name_sampling_and_bulk():
    with pytest.raises(ValueError, match="top_k / top_p / min_p need a model built with sampling=True"):      # ahead of any device
        asr.ASRModel("<none>", token_logprobs=True, top_k=50)
    with pytest.raises(ValueError, match="top_p"):
        asr.ASRModel("<none>", token_logprobs=True, sampling=True, top_p=0.0)
    plain = _model(sampling_on=False)
    try:
        for cut in ((5, None, None), (None, 0.9, None), (None, None, 0.1)):
            with pytest.raises(ValueError, match="sampling=True"):
                plain._request_sampling(None, None, cut=cut)
        assert plain._request_sampling(None, None, cut=(None, None, None)) is None
    finally:
        plain.__dict__.clear()
    m = _model()
    try:
        m.bulk = True
        with pytest.raises(ValueError, match="bulk"):
            m._request_sampling(0.5, 1, cut=(5, None, None))
    finally:
        m.__dict__.clear()
    # the schedulers' request keeps the five values, validated; the bulk replica refuses it by name
    r = Request(WIN, [1], 4, sampling=(0.5, 1, 50, 0.9, 0.05))
    assert r.sampling == (0.5, 1, 50, 0.9, 0.05) and Request(WIN, [1], 4, sampling=(0.5, 1)).sampling == (0.5, 1)
    for bad, name in (((0.5, 1, -1, 0.9, 0.0), "top_k"), ((0.5, 1, 0, 1.5, 0.0), "top_p"), ((0.5, 1, 0, 0.9, 2.0), "min_p"), ((0.5, 1, 3), "sampling")):
        with pytest.raises(ValueError, match=name):
            Request(WIN, [1], 4, sampling=bad)
    with pytest.raises(ValueError, match="bulk"):
        _BulkReplica.put(_BulkReplica.__new__(_BulkReplica), r)
    on = type("E", (), {"sampling": True})()
    assert reqvalues.keywords(on, [r, Request(WIN, [1], 4)]) == {"request_sampling": [(0.5, 1, 50, 0.9, 0.05), None]}      # the tuple passes through unchanged


# ------------------------------------------------------------------------------------------ the C ABI's pins
def test_abi_counts_hold():
    abi_pins.check_surface()
    assert "truncation" not in engine.MIRRORED_OPTIONS and len(engine.MIRRORED_OPTIONS) == 8
