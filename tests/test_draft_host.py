"""Draft-verified decoding on the host (no device): the packed words of "request_draft", ASRModel's cut rules and refusals,
draft_matched, batch fitting that counts draft tokens (with the stub engines of tests/test_dispatch.py), GatedSessions(cumulative_partials=True) with a stub
model, and the header: the feature adds no entry point and leaves the ABI version alone."""
import threading
from concurrent.futures import Future

import numpy as np
import pytest

import abi_pins
from sonicscribe_amd import asr, dispatch, engine, sessions, spec
from sonicscribe_amd.dispatch import Dispatcher, Request
from sonicscribe_amd.sampling import CallSampling
from sonicscribe_amd.sessions import DRAFT_HOLDBACK, PARTIAL_TOKENS, GatedSessions, committed_max_new_tokens

from test_dispatch import StubEngine, StubPool, seg
from test_sessions import StubModel, StubStream, energy_vad, loud


# ------------------------------------------------------------------------------------------ the words
def test_packed_words():
    w = engine.pack_request_draft([[5, 6, 7], None, [], [9]])
    assert w.dtype == np.int32 and w.tolist() == [4, 0, 3, 3, 3, 4, 5, 6, 7, 9]          # R | off[0 .. R] | ids
    assert engine.pack_request_draft([None]).tolist() == [1, 0, 0]
    assert engine.pack_request_draft([np.array([3, 4], np.int64)]).tolist() == [1, 0, 2, 3, 4]
    with pytest.raises(ValueError, match="no request"):
        engine.pack_request_draft([])
    with pytest.raises(ValueError, match="int32"):
        engine.pack_request_draft([[2 ** 31]])


def test_request_keeps_its_draft():
    assert Request([seg(0)], [1, 2], 8, draft=np.array([4, 5])).draft == [4, 5]
    assert Request([seg(0)], [1, 2], 8, draft=[]).draft is None and Request([seg(0)], [1, 2], 8).draft is None
    assert dispatch.request_tokens(Request([seg(0)], [1, 2, 3], 8, draft=[4, 5])) == 5


# ------------------------------------------------------------------------------------------ ASRModel: cut rules, refusals, draft_matched
def _model(draft_verify=True):
    m = asr.ASRModel.__new__(asr.ASRModel)                                 # no device: only the surface's own checks
    m.dims, m.prompt, m.draft_verify = spec.TINY, asr.SyntheticPrompt(spec.TINY), draft_verify
    return m


def test_cut_rules():
    eos = list(spec.TINY.eos_ids)
    assert asr.cut_draft([5, 6, eos[1], 7], eos, 100) == [5, 6]                              # in front of the first EOS id
    assert asr.cut_draft([5, 6, 7, 8], eos, 4) == [5, 6, 7]                                  # max_new - 1: the last token is the model's own
    assert asr.cut_draft([5, 6, 7, 8], eos, 1) == [] and asr.cut_draft([], eos, 10) == []
    m = _model()
    assert m._request_draft(np.array([5, 6, eos[0], 9]), 24) == [5, 6]
    assert m._request_draft([5, 6, 7], 3) == [5, 6]
    assert m._request_draft(None, 24) is None and m._request_draft([eos[0]], 24) is None     # nothing left: no draft
    with pytest.raises(ValueError, match="tokenizer"):                                       # a string goes through _candidate_ids, which needs one
        m._request_draft("some text", 24)


def test_asrmodel_refusals_by_name():
    with pytest.raises(ValueError, match="draft= needs a model built with draft_verify=True"):
        _model(False)._request_draft([5, 6], 24)
    m = _model()
    with pytest.raises(ValueError, match="draft= cannot be combined with bias values"):
        m._request_draft([5, 6], 24, bias=object())
    with pytest.raises(ValueError, match="draft= cannot be combined with a temperature ladder"):
        m._request_draft([5, 6], 24, samp=CallSampling((0.0, 0.4), True, 0))
    with pytest.raises(ValueError, match="temperature > 0"):
        m._request_draft([5, 6], 24, samp=CallSampling((0.7,), False, 0))
    assert m._request_draft([5, 6], 24, samp=CallSampling((0.0,), False, 0)) == [5, 6]                   # greedy is greedy
    with pytest.raises(ValueError, match="draft= cannot be combined with a grammar"):
        m._request_draft([5, 6], 24, gram=object())
    with pytest.raises(ValueError, match="draft_verify is not supported with mode='int8'"):
        asr.ASRModel("<none>", mode="int8", draft_verify=True)
    with pytest.raises(ValueError, match="draft_verify is not supported with bulk=True"):
        asr.ASRModel("<none>", bulk=True, draft_verify=True)


def test_draft_matched():
    assert asr.draft_matched([1, 2, 3, 4], [1, 2, 9, 4]) == 2
    assert asr.draft_matched([1, 2], [1, 2, 3]) == 2 and asr.draft_matched([], [1]) == 0 and asr.draft_matched([7], [8]) == 0
    inner = Future()
    out = asr._text_future(inner, lambda ids: "t", detailed=True, draft=[4, 5, 6])
    inner.set_result((np.array([4, 5, 9, 990], np.int32), np.zeros(4, np.float32)))
    tr = out.result(timeout=5)
    assert (tr.draft_len, tr.draft_matched) == (3, 2)
    plain = asr.Transcription("t", [1], [0.0])
    assert (plain.draft_len, plain.draft_matched) == (0, 0)


# ------------------------------------------------------------------------------------------ the schedulers
class DraftStubEngine(StubEngine):
    """the batch stub with option draft_verify: it records every batch's drafts and holds tok_cap tokens per prefill"""
    draft_verify = True

    def __init__(self, max_batch=4, tok_cap=40, delay=0.0):
        super().__init__(max_batch, delay)
        self.tok_cap, self.drafts = tok_cap, []

    def transcribe_batch(self, segs, prompts, max_new, req_win=None, request_draft=None):
        self.drafts.append(request_draft)
        assert sum(len(p) for p in prompts) + sum(len(d or ()) for d in request_draft) <= self.tok_cap or len(prompts) == 1
        return super().transcribe_batch(segs, prompts, max_new, req_win=req_win)


def test_batch_fitting_counts_draft_tokens():
    e = DraftStubEngine(max_batch=8, tok_cap=40)
    gate = threading.Event()
    orig = e.transcribe_batch

    def held(*a, **k):                                                     # the first batch waits, so the others queue up behind it and are batched together
        gate.wait(5)
        return orig(*a, **k)
    e.transcribe_batch = held
    d = Dispatcher([e])
    try:
        first = d.submit([seg(0)], [1] * 10, 8)
        import time
        time.sleep(0.05)
        futs = [d.submit([seg(i + 1)], [1] * 10, 8, draft=[7] * 6) for i in range(4)]      # 16 tokens each: two fit 40, three do not
        futs.append(d.submit([seg(9)], [1] * 10, 8, draft=[7] * 7))                           # (the same step class)
        gate.set()
        for f in [first] + futs:
            f.result(timeout=10)
    finally:
        d.close()
    sizes = [len(b) for b in e.drafts]
    assert sizes[0] == 1 and max(sizes[1:]) == 2 and sum(sizes) == 6, sizes
    assert e.drafts[0] == [None] and all(x == [7] * 6 or x == [7] * 7 for b in e.drafts[1:] for x in b)


def test_engines_without_the_option_batch_as_before_and_refuse_a_draft():
    e = StubEngine(max_batch=4)
    d = Dispatcher([e])
    try:
        with pytest.raises(ValueError, match="draft_verify"):
            d.submit([seg(0)], [1, 2], 8, draft=[5])
        assert d.submit([seg(0)], [1, 2], 8).result(timeout=5) is not None
    finally:
        d.close()
    with pytest.raises(ValueError, match="cannot be combined"):
        dispatch.check_draft(Request([seg(0)], [1], 8, sampling=(0.5, 1), draft=[5]), [DraftStubEngine()])
    dispatch.check_draft(Request([seg(0)], [1], 8, sampling=(0.0, 1), draft=[5]), [DraftStubEngine()])


def test_continuous_replica_hands_the_drafts_to_the_prefill():
    pool = StubPool(n_rows=4, prefill_batch=4)
    staged = []
    for p in pool.prefills:
        p.draft_verify, p.tok_cap = True, 1000
        p.set_request_draft = lambda drafts, p=p: staged.append(list(drafts))
    pool.decoder.draft_verify, pool.decoder.tok_cap = True, 1000
    d = Dispatcher([pool.decoder], slots=[pool.prefills], continuous=True)
    try:
        a = d.submit([seg(1)], [1, 2, 3], 9, draft=[4, 5])
        b = d.submit([seg(2)], [1, 2, 3], 9)
        a.result(timeout=10); b.result(timeout=10)
    finally:
        d.close()
    flat = [x for batch in staged for x in batch]
    assert sorted(flat, key=lambda x: x is None) == [[4, 5], None]


def test_bulk_replica_refuses_a_draft_by_name():
    src = open(dispatch.__file__).read()
    assert "a draft is not supported with bulk=True" in src
    from test_dispatch import StubNativePipeline  # noqa: F401  (the bulk replica's stub: its put() is what refuses)
    rep = dispatch._BulkReplica.__new__(dispatch._BulkReplica)
    with pytest.raises(ValueError, match="a draft is not supported with bulk=True"):
        rep.put(Request([seg(0)], [1], 8, draft=[5]))


# ------------------------------------------------------------------------------------------ cumulative partials
class Tr:
    def __init__(self, ids):
        self.token_ids = np.asarray(ids, np.int32)


class DraftStream(StubStream):
    """records every request with its draft; a partial's transcript: token 100 + k for every 1024 samples of audio, then an EOS id"""
    def submit_samples(self, first, n, max_new, hotwords=None, detailed=False, draft=None):
        self.sub.append((first, n, max_new, None if draft is None else list(draft), detailed))
        f = Future()
        ids = [100 + k for k in range(n // 1024)][:max_new - 1] + [spec.TINY.eos_ids[0]]
        f.set_result(Tr(ids) if detailed else f"{first}:{n}:{max_new}")
        return f


class DraftModel(StubModel):
    token_logprobs = draft_verify = True
    dims = spec.TINY

    def open_stream(self, s, buffer_seconds):
        return DraftStream()


def _drive(g, pattern, t0=100.0):
    ev = []
    for t, v in enumerate(pattern):
        for s in range(len(g.ids)):
            g.add_audio_chunk(s, loud(v), timestamp=t0 + 0.064 * (t + 1))
        ev.extend(g.tick(energy_vad, now=t0 + 0.064 * (t + 1)))
    return ev


PATTERN = [0] * 12 + [9000] * 60 + [0] * 40


def test_cumulative_partials_ranges_budgets_holdback_and_the_final():
    g = GatedSessions(DraftModel(), ["a"], cumulative_partials=True)
    ev = _drive(g, PATTERN)
    sub = g.streams[0].sub
    parts = [e for e in ev if e["type"] == "partial"]
    finals = [e for e in ev if e["type"] == "final"]
    start = [e for e in ev if e["type"] == "speech_start"][0]["start_chunk_id"]
    assert len(parts) >= 3 and len(finals) == 1 and len(sub) == len(parts) + 1
    prev = None
    for e, (first, n, max_new, draft, detailed) in zip(parts, sub):
        assert detailed and first == start * 1024 and e["start_chunk_id"] == start              # segment start -> newest chunk
        assert n == (e["end_chunk_id"] - start + 1) * 1024
        want = None
        if prev is not None:                                                                   # the previous partial: EOS and the last DRAFT_HOLDBACK tokens dropped
            ids = [t for t in prev if t not in spec.TINY.eos_ids]
            want = ids[:len(ids) - DRAFT_HOLDBACK] or None
        assert draft == want
        assert max_new == min(len(draft or ()) + PARTIAL_TOKENS, committed_max_new_tokens(n / 16000)) == e["max_new_tokens"]
        assert e["draft_len"] == len(draft or ())
        prev = e["future"].result().token_ids.tolist()
    assert [n for _, n, _, _, _ in sub[:len(parts)]] == sorted(n for _, n, _, _, _ in sub[:len(parts)]) and sub[len(parts) - 1][1] > sub[0][1]
    first, n, max_new, draft, detailed = sub[-1]                                               # the final takes the last partial's transcript
    ids = [t for t in prev if t not in spec.TINY.eos_ids]
    assert detailed and draft == ids[:len(ids) - DRAFT_HOLDBACK] and finals[0]["draft_len"] == len(draft)
    assert first == start * 1024 and max_new == committed_max_new_tokens(finals[0]["seconds"])
    assert isinstance(finals[0]["future"].result(), Tr)


def test_default_mode_issues_exactly_todays_requests():
    a = GatedSessions(StubModel(), ["a"])
    b = GatedSessions(DraftModel(), ["a"])                                                     # a draft_verify model, the mode left off
    ev_a, ev_b = _drive(a, PATTERN), _drive(b, PATTERN)
    assert [s for s in a.streams[0].sub] == [s[:3] for s in b.streams[0].sub]
    assert all(s[3] is None and s[4] is False for s in b.streams[0].sub)
    assert [(e["type"], e.get("n_samples")) for e in ev_a] == [(e["type"], e.get("n_samples")) for e in ev_b]
    assert any(s[1] == 20 * 1024 and s[2] == PARTIAL_TOKENS for s in a.streams[0].sub)           # the newest 1.28 s, 15 tokens


def test_cumulative_partials_refusals():
    with pytest.raises(ValueError, match="token_logprobs=True and draft_verify=True"):
        GatedSessions(StubModel(), ["a"], cumulative_partials=True)
    with pytest.raises(ValueError, match="cannot be combined with bias values or a temperature"):
        GatedSessions(DraftModel(), ["a"], cumulative_partials=True, hotword_boost=2.0)


# ------------------------------------------------------------------------------------------ the header
def test_no_new_entry_point_and_the_same_abi():
    abi_pins.check_surface(names=("sonic_dispatch_submit",), header_strings=("draft_verify", "request_draft", "const int32_t* draft_ids; int32_t n_draft;", "draft_accepted"))
    assert [f for f, _ in engine.DispatchRequest._fields_][-2:] == ["draft_ids", "n_draft"]
