"""The per-request values between dispatch.Request and the engine call (sonicscribe_amd/reqvalues.py; no device): the list itself, the keywords the batch replica
states (whole batch and one-by-one retry), the setters the continuous replica calls ahead of a prefill, the refusals of the three replicas that refuse in put() - their
texts pinned here as literals -, Engine's one arming method in front of its three consuming calls (a recording stand-in for the library), and the table of the options
a handle mirrors.  Stub engines are those of tests/test_dispatch.py."""
import re
import threading
from types import SimpleNamespace

import numpy as np
import pytest

from sonicscribe_amd import dispatch, engine, reqvalues, spec
from sonicscribe_amd.dispatch import Dispatcher, Request
from sonicscribe_amd.reqbias import RequestBias
from sonicscribe_amd.sampling import CallSampling

from test_dispatch import StubEngine, StubPool, seg

OPTIONS = ("request_bias", "sampling", "grammar", "draft_verify")


# ------------------------------------------------------------------------------------------ the list
def test_the_list_names_what_the_sites_use():
    assert [v.attr for v in reqvalues.VALUES] == ["bias", "sampling", "grammar", "draft"]               # the order of arming and of the keywords
    assert tuple(v.option for v in reqvalues.VALUES) == OPTIONS
    assert [v.keyword for v in reqvalues.VALUES] == ["request_bias", "request_sampling", "request_grammar", "request_draft"]
    assert [v.setter for v in reqvalues.VALUES] == ["set_request_bias", "set_request_sampling", "set_request_grammar", "set_request_draft"]
    assert all(v.attr in Request.__slots__ and hasattr(engine.Engine, v.setter) for v in reqvalues.VALUES)
    src = open(reqvalues.__file__).read()
    assert not re.search(r"^\s*(from|import)\b.*\b(dispatch|engine)\b", src, re.M)                       # both import it
    assert dispatch.check_draft is reqvalues.check_draft


def test_submit_keywords_only_what_the_request_brings():
    g = object()
    CV, CS = reqvalues.CallValues, CallSampling
    assert reqvalues.submit_keywords(CV(None, None, None, None)) == {}
    assert reqvalues.submit_keywords(CV(RequestBias(), CS((0.0, 0.4), True, 3), None, [])) == {}              # an empty table, a ladder, an empty draft: nothing
    assert reqvalues.submit_keywords(CV("b", CS((0.3,), False, 9), g, [4, 5])) == {"bias": "b", "sampling": (0.3, 9), "grammar": g, "draft": [4, 5]}
    assert reqvalues.submit_keywords(CV(None, CS((0.0,), False, 0), None, None)) == {"sampling": (0.0, 0)}    # a greedy single temperature is still stated


# ------------------------------------------------------------------------------------------ the batch replica's keywords
class StubGrammar:
    """what a grammar.CompiledGrammar is to the dispatcher: on(engine) gives the handle that serves that engine"""
    def on(self, e):
        return ("device grammar", self, e)


class RecordingEngine(StubEngine):
    """the batch stub with the four options `on` or off: records every call's request count and keywords; fail_above: a call with more requests raises"""
    def __init__(self, on, max_batch=8, fail_above=None):
        super().__init__(max_batch)
        for o in OPTIONS:
            setattr(self, o, on)
        self.tok_cap, self.calls, self.fail_above, self.entered = 10 ** 6, [], fail_above, threading.Event()

    def transcribe_batch(self, segs, prompts, max_new, req_win=None, **kw):
        self.entered.set()
        self.calls.append((len(prompts), kw))
        if self.fail_above is not None and len(prompts) > self.fail_above:
            raise ValueError("not this batch")
        return super().transcribe_batch(segs, prompts, max_new, req_win=req_win)


BIAS, SAMPLING, GRAMMAR, DRAFT = RequestBias([[[5, 6], 1.0]]), (0.5, 7), StubGrammar(), [4, 5]
FOUR = ({"bias": BIAS}, {"sampling": SAMPLING}, {"grammar": GRAMMAR}, {"draft": DRAFT})


def _queue_behind_a_held_batch(e, requests):
    """the first batch waits inside the engine, so `requests` (keywords of Dispatcher.submit) queue up behind it and form one batch; returns their results"""
    e.gate = threading.Event()
    d = Dispatcher([e])
    try:
        first = d.submit([seg(0)], [1] * 3, 8)
        assert e.entered.wait(5)
        futs = [d.submit([seg(i + 1)], [1] * 3, 8, **kw) for i, kw in enumerate(requests)]
        e.gate.set()
        return [f.result(timeout=10) for f in [first] + futs]
    finally:
        e.gate.set()
        d.close()


def _one_of_four(i):
    """the four keywords of a one-request call for request i of FOUR: its own value, None for the other three"""
    def value(e, k):
        return [None if k != i else ("device grammar", GRAMMAR, e) if k == 2 else (BIAS, SAMPLING, GRAMMAR, DRAFT)[k]]
    return lambda e: {v.keyword: value(e, k) for k, v in enumerate(reqvalues.VALUES)}


def test_batch_keywords_in_batch_order():
    e = RecordingEngine(on=True)
    res = _queue_behind_a_held_batch(e, FOUR)
    assert len(res) == 5 and [n for n, _ in e.calls] == [1, 4]
    assert e.calls[0][1] == {"request_bias": [None], "request_sampling": [None], "request_grammar": [None], "request_draft": [None]}      # option on: always stated
    kw = e.calls[1][1]
    assert list(kw) == ["request_bias", "request_sampling", "request_grammar", "request_draft"]
    assert kw["request_bias"] == [BIAS, None, None, None] and kw["request_bias"][0] is BIAS
    assert kw["request_sampling"] == [None, SAMPLING, None, None]
    assert kw["request_grammar"] == [None, None, ("device grammar", GRAMMAR, e), None]              # what grammar.on(engine) returned for THIS engine
    assert kw["request_draft"] == [None, None, None, DRAFT]


def test_no_keyword_without_option_and_value():
    e = RecordingEngine(on=False)
    _queue_behind_a_held_batch(e, [{}, {}, {}])
    assert [n for n, _ in e.calls] == [1, 3] and all(kw == {} for _, kw in e.calls)
    plain = StubEngine(max_batch=4)                          # its transcribe_batch(segs, prompts, max_new, req_win=None) knows no keyword at all
    d = Dispatcher([plain])
    try:
        assert d.submit([seg(3)], [1, 2], 8).result(timeout=5).tolist() == [48, 2, 8]
    finally:
        d.close()
    # an engine without the options still hears of a value that a request brings (and refuses it itself): only those keywords
    assert reqvalues.keywords(plain, [Request([seg(0)], [1], 8, sampling=SAMPLING), Request([seg(1)], [1], 8)]) == {"request_sampling": [SAMPLING, None]}


def test_retry_states_each_requests_own_values():
    e = RecordingEngine(on=True, fail_above=1)
    res = _queue_behind_a_held_batch(e, FOUR)
    assert len(res) == 5 and all(r is not None for r in res)                                      # every future resolved
    assert [n for n, _ in e.calls] == [1, 4, 1, 1, 1, 1]
    for i, (_, kw) in enumerate(e.calls[2:]):
        assert kw == _one_of_four(i)(e), i


# ------------------------------------------------------------------------------------------ the continuous replica's setters
def _recording_pool(on):
    pool = StubPool(n_rows=4, prefill_batch=4)
    events = []
    for h in pool.prefills + [pool.decoder]:
        h.tok_cap = 10 ** 6
        for o in OPTIONS:
            setattr(h, o, on)
    for p in pool.prefills:
        for v in reqvalues.VALUES:
            setattr(p, v.setter, lambda values, name=v.setter: events.append((name, list(values))))
        orig = p.prefill
        p.prefill = lambda prompts, max_new, req_win=None, wait=True, orig=orig: (events.append(("prefill", len(prompts))), orig(prompts, max_new, req_win, wait))[1]
    return pool, events


def test_continuous_replica_arms_the_four_in_order_ahead_of_each_prefill():
    pool, events = _recording_pool(on=True)
    d = Dispatcher([pool.decoder], slots=[pool.prefills], continuous=True)
    try:
        for f in [d.submit([seg(i + 1)], [1, 2, 3], 9, **kw) for i, kw in enumerate(FOUR)]:
            f.result(timeout=10)
    finally:
        d.close()
    setters = [v.setter for v in reqvalues.VALUES]
    assert len(events) % 5 == 0
    told = {s: [] for s in setters}
    for k in range(0, len(events), 5):                       # per prefill batch: the four setters in the list's order, then the prefill, lists as long as the batch
        assert [n for n, _ in events[k:k + 5]] == setters + ["prefill"]
        assert all(len(values) == events[k + 4][1] for _, values in events[k:k + 4])
        for name, values in events[k:k + 4]:
            told[name] += values
    eng = pool.prefills[0]                                   # one prefill slot, a FIFO queue: the batches' lists in a row are the requests in submission order
    assert told == {"set_request_bias": [BIAS, None, None, None], "set_request_sampling": [None, SAMPLING, None, None],
                    "set_request_grammar": [None, None, ("device grammar", GRAMMAR, eng), None], "set_request_draft": [None, None, None, DRAFT]}


def test_continuous_replica_calls_no_setter_without_option_and_value():
    pool, events = _recording_pool(on=False)
    d = Dispatcher([pool.decoder], slots=[pool.prefills], continuous=True)
    try:
        for f in [d.submit([seg(i + 1)], [1, 2, 3], 9) for i in range(2)]:
            f.result(timeout=10)
    finally:
        d.close()
    assert events and all(n == "prefill" for n, _ in events)


# ------------------------------------------------------------------------------------------ the refusals, texts as the replicas have always worded them
NEEDS = {
    "bias": "a sequence bias needs the engine option request_bias on every handle (ASRModel(request_bias=True))",
    "sampling": "a temperature needs the engine option sampling on every handle (ASRModel(sampling=True))",
    "grammar": "a grammar needs the engine option grammar on every handle (ASRModel(token_logprobs=True, grammar=True))",
    "draft": "a draft needs the engine option draft_verify on every handle (ASRModel(draft_verify=True))",
}
BULK = {
    "bias": "a sequence bias is not supported with bulk=True (the bulk pipeline carries no per-request tables): use the continuous or the batch dispatcher",
    "sampling": "a temperature is not supported with bulk=True (the bulk pipeline carries no per-request values): use the continuous or the batch dispatcher",
    "grammar": "a grammar is not supported with bulk=True (the bulk pipeline carries no per-request grammar state): use the continuous or the batch dispatcher",
    "draft": "a draft is not supported with bulk=True (the bulk pipeline verifies no drafts): use the continuous or the batch dispatcher",
}
VALUE = {"bias": BIAS, "sampling": SAMPLING, "grammar": GRAMMAR, "draft": DRAFT}


def _replica(kind):
    """a replica of `kind` over handles without any option, as far as its put() reads it before it refuses: no thread, no library"""
    engines = [SimpleNamespace(max_batch=4), SimpleNamespace(max_batch=4)]
    if kind == "continuous":
        rep = dispatch._ContinuousReplica.__new__(dispatch._ContinuousReplica)
        rep.engine, rep.engines = engines[0], engines
    elif kind == "native":
        rep = dispatch._NativeContinuousReplica.__new__(dispatch._NativeContinuousReplica)
        rep.engine, rep.engines, rep.lp, rep.admits = engines[0], engines, False, reqvalues.supported(engines)
    else:
        rep = dispatch._BulkReplica.__new__(dispatch._BulkReplica)
    return rep


def _refusal(kind, **values):
    with pytest.raises(ValueError) as ex:
        _replica(kind).put(Request([seg(0)], [1], 8, **values))
    return str(ex.value)


@pytest.mark.parametrize("kind", ["continuous", "native", "bulk"])
@pytest.mark.parametrize("attr", ["bias", "sampling", "grammar", "draft"])
def test_refusal_texts(kind, attr):
    assert _refusal(kind, **{attr: VALUE[attr]}) == (BULK if kind == "bulk" else NEEDS)[attr]


@pytest.mark.parametrize("kind", ["continuous", "native", "bulk"])
def test_which_refusal_fires_first(kind):
    texts = BULK if kind == "bulk" else NEEDS
    assert _refusal(kind, bias=BIAS, grammar=GRAMMAR) == texts["bias"]
    assert _refusal(kind, grammar=GRAMMAR, draft=DRAFT) == texts["draft" if kind == "bulk" else "grammar"]      # the bulk replica asks bias, draft, grammar, sampling


def test_supported_flags_need_every_handle():
    on, off = SimpleNamespace(request_bias=True, sampling=True, grammar=True, draft_verify=True), SimpleNamespace(request_bias=True, grammar=True)
    assert reqvalues.supported([on, on]) == (True, True, True, True) and reqvalues.supported([on, off]) == (True, False, True, False)
    reqvalues.refuse_unsupported(Request([seg(0)], [1], 8, bias=BIAS, grammar=GRAMMAR), reqvalues.supported([on, off]))
    with pytest.raises(ValueError, match="a temperature needs the engine option sampling"):
        reqvalues.refuse_unsupported(Request([seg(0)], [1], 8, sampling=SAMPLING), reqvalues.supported([on, off]))


# ------------------------------------------------------------------------------------------ Engine: one arming method in front of three consuming calls
class RecordingLib:
    """stands in for the ctypes library: every function records its name and first arguments and returns 0"""
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


ARMS = ["sonic_set_request_bias", "sonic_set_request_sampling", ("sonic_set_option", b"request_grammar_begin"), ("sonic_set_option", b"request_grammar"),
        ("sonic_load_tensor", b"request_draft")]


def _consume(e, how, **kw):
    """one of the three consuming calls with a one-request batch; the per-request keywords are `kw`"""
    if how == "prefill":
        return e.prefill([[1, 2, 3]], [4], [0, 1], **kw)
    wins = [seg(1)] if how == "host" else [engine.RingSlice(SimpleNamespace(h=11, engine=e), 0, 16)]
    return e.transcribe_batch(wins, [[1, 2, 3]], [4], req_win=[0, 1], **kw)


ENTRY = {"host": "sonic_transcribe_batch", "ring": "sonic_transcribe_mixed", "prefill": "sonic_prefill"}


@pytest.mark.parametrize("how", ["host", "ring", "prefill"])
def test_engine_arms_in_order_right_ahead_of_the_consuming_call(how):
    e = _engine()
    try:
        g = SimpleNamespace(h=3, id=3, engine=e)
        _consume(e, how, request_bias=[BIAS], request_sampling=[SAMPLING], request_grammar=[g], request_draft=[DRAFT])
        assert _names(e) == ARMS + [ENTRY[how]]              # nothing ahead of the arms, nothing between them and the call, nothing behind it
        e.lib.calls.clear()
        _consume(e, how)
        assert _names(e) == [ENTRY[how]]                     # a caller that states nothing arms nothing
        e.lib.calls.clear()
        _consume(e, how, request_grammar=[None], request_draft=[None])
        assert _names(e) == [ARMS[2], ARMS[4], ENTRY[how]]   # (a free request: the begin option alone)
        for bad in ({"request_sampling": [(-1.0, 0)]}, {"request_draft": [[2 ** 31]]}):
            e.lib.calls.clear()
            with pytest.raises(ValueError):
                _consume(e, how, request_bias=[BIAS], request_grammar=[g], **bad)
            assert e.lib.calls == []                         # validated before anything is armed
    finally:
        e.h = None


def test_prefill_enqueue_is_armed_the_same_way():
    e = _engine()
    try:
        e.prefill([[1, 2, 3]], [4], [0, 1], wait=False, request_sampling=[SAMPLING], request_draft=[DRAFT])
        assert _names(e) == [ARMS[1], ARMS[4], "sonic_prefill_enqueue"]
    finally:
        e.h = None


def test_host_pcm_and_ring_slices_return_the_same_structure():
    got = {}
    for how in ("host", "ring"):
        e = _engine()
        try:
            plain = _consume(e, how)
            wide = e.transcribe_batch([seg(1)] if how == "host" else [engine.RingSlice(SimpleNamespace(h=11, engine=e), 0, 16)], [[1, 2, 3]], [4], req_win=[0, 1],
                                      want_logits=True, want_logprobs=True)
            assert _names(e)[-2:] == [ENTRY[how], "sonic_fetch_logprobs"]
        finally:
            e.h = None
        got[how] = (plain, wide)
    for plain, wide in got.values():
        assert len(plain) == 2 and plain[1] is None and len(wide) == 3
        assert [i.dtype for i in plain[0]] == [np.int32] and [i.shape for i in plain[0]] == [(0,)]      # (the stand-in writes no token)
        assert wide[1].shape == (4, 1, spec.TINY.vocab) and wide[1].dtype == np.float32
        assert len(wide[2]) == 1 and wide[2][0].shape == (0,)
    assert [type(x) for x in got["host"][0]] == [type(x) for x in got["ring"][0]] and [type(x) for x in got["host"][1]] == [type(x) for x in got["ring"][1]]


# ------------------------------------------------------------------------------------------ the options a handle mirrors
MIRRORED = {"token_logprobs": bool, "top_logprobs": int, "request_bias": bool, "sampling": bool, "grammar": bool, "forced_parallel": bool, "forced_align": bool,
            "draft_verify": bool}


def test_mirrored_options():
    assert engine.MIRRORED_OPTIONS == MIRRORED
    e = _engine()
    try:
        for name, kind in MIRRORED.items():
            assert not hasattr(e, name)
            e.set_option(name, 1)
            assert type(getattr(e, name)) is kind and getattr(e, name) == 1
        e.set_option("top_logprobs", 5)
        e.set_option("gemm_small_eff", 75)                   # not mirrored: the library alone keeps it
        assert not hasattr(e, "gemm_small_eff") and [a[1:] for _, a in e.lib.calls][-2:] == [(b"top_logprobs", 5), (b"gemm_small_eff", 75)]
        slot = SimpleNamespace()
        engine.copy_mirrored_options(e, slot)
        assert vars(slot) == {**{n: True for n in MIRRORED}, "top_logprobs": 5} and type(slot.top_logprobs) is int
        e.set_option("token_logprobs", 0)
        e.set_option("draft_verify", 0)
        engine.copy_mirrored_options(e, slot)                # a slot whose token_logprobs is off returns no records: their width is 0
        assert slot.token_logprobs is False and slot.top_logprobs == 0 and slot.draft_verify is False and slot.sampling is True
        bare = SimpleNamespace()
        engine.copy_mirrored_options(SimpleNamespace(), bare)            # an owner on which no option was ever set
        assert vars(bare) == {**{n: False for n in MIRRORED}, "top_logprobs": 0}
    finally:
        e.h = None
