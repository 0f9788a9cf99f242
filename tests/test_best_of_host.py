"""Row forks and best_of without a device: the seed rule, the ranker, the one statement of the row order, what Engine arms ahead of a forked call
(on the recording stand-in of tests/test_reqvalues_host.py), and ASRModel's policy - which attempts fork, who wins, what the result carries - on stub handles."""
from concurrent.futures import Future
from types import SimpleNamespace

import numpy as np
import pytest

from sonicscribe_amd import asr, engine, fallback, sampling, spec
from sonicscribe_amd.reqbias import RequestBias
from sonicscribe_amd.reqvalues import CallValues
from sonicscribe_amd.sampling import CallSampling

from test_dispatch import seg
from test_reqvalues_host import ENTRY, _consume, _engine, _names

FORKS_ARM = ("sonic_load_tensor", b"request_forks")


# ------------------------------------------------------------------------------------------ the rules
def test_fork_seed_wraps_at_2_64():
    assert [sampling.fork_seed(7, j) for j in range(3)] == [7, 8, 9]
    assert sampling.fork_seed(2 ** 64 - 1, 0) == 2 ** 64 - 1 and sampling.fork_seed(2 ** 64 - 1, 1) == 0 and sampling.fork_seed(2 ** 64 - 2, 5) == 3
    for bad in (-1, True, 1.0):
        with pytest.raises(ValueError, match="fork index"):
            sampling.fork_seed(0, bad)
    with pytest.raises(ValueError, match="seed"):
        sampling.fork_seed(2 ** 64, 0)


def test_pick_best_ties_and_order():
    assert fallback.pick_best([-1.0]) == 0
    assert fallback.pick_best([-2.0, -0.5, -1.0]) == 1 and fallback.pick_best([-0.5, -2.0, -1.0]) == 0 and fallback.pick_best([-3.0, -2.0, -1.0]) == 2
    assert fallback.pick_best([-1.0, -0.5, -0.5]) == 1 and fallback.pick_best([-0.5, -0.5, -0.5]) == 0      # ties: the lowest index
    assert fallback.pick_best([float("nan"), -9.0, float("nan")]) == 1 and fallback.pick_best([float("nan"), float("nan")]) == 0
    assert fallback.pick_best(np.asarray([-1.0, -0.25], np.float32)) == 1
    with pytest.raises(ValueError, match="no sample"):
        fallback.pick_best([])


def test_fork_rows_is_the_row_order():
    assert engine.Engine.fork_rows([3, 1, 2]) == [[0, 3, 4], [1], [2, 5]]
    assert engine.Engine.fork_rows([1, 1]) == [[0], [1]] and engine.Engine.fork_rows([4]) == [[0, 1, 2, 3]]
    assert engine.Engine.fork_rows([4, 4]) == [[0, 2, 3, 4], [1, 5, 6, 7]]
    rows = engine.Engine.fork_rows([2, 5, 1, 3])
    assert sorted(r for rr in rows for r in rr) == list(range(11)) and [rr[0] for rr in rows] == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------ Engine: what a forked call arms
@pytest.mark.parametrize("how", ["host", "ring", "prefill"])
def test_forks_are_armed_directly_ahead_of_the_consuming_call(how):
    e = _engine()
    e.max_batch = 8
    try:
        _consume(e, how, forks=[2])
        assert _names(e) == [FORKS_ARM, ENTRY[how]]
        name, args = e.lib.calls[0]
        assert args[3] == engine.DTYPE_I32 and list(args[4]) == [1] and args[5] == 1      # one row of int32 words, one per request
        A = e.lib.calls[1][1][{"host": 5, "ring": 8, "prefill": 2}[how]]
        assert A == 1                                                                    # the entry point's R stays the REQUEST count
        e.lib.calls.clear()
        g = SimpleNamespace(h=3, id=3, engine=e)
        _consume(e, how, forks=[2], request_bias=[RequestBias([[[5], 1.0]]), None], request_sampling=[(0.5, 1), (0.5, 2)], request_grammar=[g, None])
        assert _names(e) == ["sonic_set_request_bias", "sonic_set_request_sampling", ("sonic_set_option", b"request_grammar_begin"), ("sonic_set_option", b"request_grammar"),
                             FORKS_ARM, ENTRY[how]]
        assert e.lib.calls[1][1][-1] == 2                                                # the per-request stages count ROWS
        # validated before anything is armed: a per-row list of the wrong length, counts that do not fit, a draft
        for bad in (dict(forks=[2], request_sampling=[(0.5, 1)]), dict(forks=[2], request_bias=[None]), dict(forks=[2], request_grammar=[g, g, g]), dict(forks=[9]), dict(forks=[0]),
                    dict(forks=[1, 1]), dict(forks=[2], request_draft=[[5]])):
            e.lib.calls.clear()
            with pytest.raises(ValueError, match="forks"):
                _consume(e, how, **bad)
            assert e.lib.calls == []
        # a call without `forks` makes exactly the calls it made before
        e.lib.calls.clear()
        _consume(e, how, request_sampling=[(0.5, 1)])
        assert _names(e) == ["sonic_set_request_sampling", ENTRY[how]]
        e.lib.calls.clear()
        _consume(e, how)
        assert _names(e) == [ENTRY[how]]
    finally:
        e.h = None


def test_forked_results_have_one_entry_per_row():
    e = _engine()
    e.max_batch = 8
    try:
        ids, logits, lps = e.transcribe_batch([seg(1)], [[1, 2, 3]], [4], req_win=[0, 1], want_logits=True, want_logprobs=True, forks=[3])
        assert len(ids) == 3 and logits.shape == (4, 3, spec.TINY.vocab) and len(lps) == 3
    finally:
        e.h = None


# ------------------------------------------------------------------------------------------ ASRModel: the policy on stub handles
class StubDispatcher:
    """greedy attempts: ids [7, 8], log-probabilities -2 each"""
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
    """a forked run: the row of seed s emits [s % 1000] with log-probability LP[s]"""
    def __init__(self, lp_of_seed):
        self.calls, self.lp = [], lp_of_seed

    def transcribe_batch(self, segs, prompts, max_new, req_win=None, want_logprobs=False, request_sampling=None, forks=None, **kw):
        self.calls.append(dict(n_segs=len(segs), prompts=prompts, max_new=list(max_new), req_win=list(req_win), sampling=list(request_sampling), forks=list(forks), kw=kw))
        assert want_logprobs and len(request_sampling) == sum(forks)
        ids = [np.asarray([s % 1000], np.int32) for _, s in request_sampling]
        return ids, None, [np.asarray([self.lp[s]], np.float32) for _, s in request_sampling]


def _model(best_of=3, lp_of_seed=None, logprob_threshold=-1.0):
    m = asr.ASRModel.__new__(asr.ASRModel)                                 # no device: the policy alone
    m.best_of, m._max_batch, m.sampling = best_of, 8, True
    m.prompt = asr.SyntheticPrompt(spec.TINY)
    m.compression_ratio_threshold, m.logprob_threshold = None, logprob_threshold
    m._dispatcher, m._retrier = StubDispatcher(), fallback._Inline
    m._fork_engines = [StubForkEngine(lp_of_seed or {})] if best_of > 1 else []
    m._fork_workers, m._fork_next = [fallback._Inline for _ in m._fork_engines], 0
    return m


def test_temperature_zero_never_forks():
    m = _model(lp_of_seed={})
    try:
        tr = m._dispatch([seg(1)], [1, 2, 3], 4, True, CallValues(samp=CallSampling((0.0,), False, 5), best_of=3)).result(timeout=5)
        assert m._fork_engines[0].calls == [] and len(m._dispatcher.calls) == 1
        assert (tr.best_of, tr.fork_index) == (1, 0) and tr.fork_avg_logprobs.tolist() == [tr.avg_logprob] and tr.token_ids.tolist() == [7, 8]
        # ... nor does a call that asks for one sample
        m._dispatch([seg(1)], [1, 2, 3], 4, True, CallValues(samp=CallSampling((0.8,), False, 5), best_of=1)).result(timeout=5)
        assert m._fork_engines[0].calls == [] and m._dispatcher.calls[-1]["sampling"] == (0.8, 5)
    finally:
        m.__dict__.clear()


def test_a_sampled_attempt_is_one_forked_run_and_the_best_fork_wins():
    m = _model(lp_of_seed={41: -3.0, 42: -0.5, 43: -0.5})
    try:
        bias = RequestBias([[[5], 1.0]])
        tr = m._dispatch([seg(1), seg(2)], [1, 2, 3], 4, True, CallValues(bias, CallSampling((0.8,), False, 41), best_of=3)).result(timeout=5)
        assert m._dispatcher.calls == [] and len(m._fork_engines[0].calls) == 1
        c = m._fork_engines[0].calls[0]
        assert c["forks"] == [3] and c["sampling"] == [(0.8, 41), (0.8, 42), (0.8, 43)] and c["n_segs"] == 2 and c["req_win"] == [0, 2] and c["max_new"] == [4]
        assert c["kw"] == {"request_bias": [bias, bias, bias]}                          # the table is repeated on every fork; no grammar: no keyword
        assert (tr.best_of, tr.fork_index, tr.temperature) == (3, 1, 0.8) and tr.token_ids.tolist() == [42]      # the tie between forks 1 and 2 goes to the lower
        assert tr.fork_avg_logprobs.tolist() == [-3.0, -0.5, -0.5] and tr.avg_logprob == -0.5
        # the seeds wrap; the text alone when the caller asked for no details
        m._fork_engines[0].lp = {2 ** 64 - 1: -1.0, 0: -2.0}
        text = m._dispatch([seg(1)], [1, 2, 3], 4, False, CallValues(samp=CallSampling((0.5,), False, 2 ** 64 - 1), best_of=2)).result(timeout=5)
        assert m._fork_engines[0].calls[-1]["sampling"] == [(0.5, 2 ** 64 - 1), (0.5, 0)] and isinstance(text, str)
    finally:
        m.__dict__.clear()


def test_the_ladder_forks_only_its_sampled_rungs():
    m = _model(lp_of_seed={9: -0.25, 10: -0.125, 11: -4.0}, logprob_threshold=-1.0)      # the greedy attempt averages -2: it fails the threshold
    try:
        tr = m._dispatch([seg(1)], [1, 2, 3], 4, True, CallValues(samp=CallSampling((0.0, 0.8, 1.0), True, 9), best_of=3)).result(timeout=5)
        assert len(m._dispatcher.calls) == 1 and m._dispatcher.calls[0]["sampling"] == (0.0, 9)
        assert [c["sampling"] for c in m._fork_engines[0].calls] == [[(0.8, 9), (0.8, 10), (0.8, 11)]]      # the winner passed: no third rung
        assert (tr.attempts, tr.temperature, tr.best_of, tr.fork_index) == (2, 0.8, 3, 1) and tr.avg_logprob == -0.125
    finally:
        m.__dict__.clear()


def test_refusals_name_best_of():
    for bad in (0, 9, True, 2.0, "3"):
        with pytest.raises(ValueError, match="best_of must be an integer in 1 .. 8"):
            asr.check_best_of(bad, 8)
    assert asr.check_best_of(1, 8, sampling=False, bulk=True) == 1 and asr.check_best_of(8, 8) == 8
    with pytest.raises(ValueError, match="best_of > 1 needs sampling=True"):
        asr.check_best_of(2, 8, sampling=False)
    with pytest.raises(ValueError, match="best_of is not supported with bulk=True"):
        asr.check_best_of(2, 8, sampling=True, bulk=True)
    with pytest.raises(ValueError, match="best_of"):                                      # ... ahead of any device
        asr.ASRModel("<none>", token_logprobs=True, best_of=3)
    plain = _model(best_of=1)
    try:
        assert plain._request_best_of() == 1
        for n in (1, 3):
            with pytest.raises(ValueError, match="best_of= needs a model built with best_of > 1"):
                plain._request_best_of(n)
        plain.model, plain.token_logprobs = object(), True
        with pytest.raises(ValueError, match="best_of"):
            plain.submit(np.zeros(1600, np.float32), best_of=2)
    finally:
        plain.__dict__.clear()
    m = _model(best_of=3)
    try:
        assert m._request_best_of() == 3 and m._request_best_of(1) == 1 and m._request_best_of(8) == 8
        with pytest.raises(ValueError, match="best_of must be an integer"):
            m._request_best_of(9)
    finally:
        m.__dict__.clear()
