"""Host side of the per-token log-probabilities (option token_logprobs), on CPU: the C ABI's five new entry points are declared, exported and
bound at version 12; the result object's mean covers every emitted token (EOS included) and is nan for none; the Python schedulers resolve a
`want_logprobs` request to (ids, log-probabilities) over stub engines and leave the other requests - and engines that never heard of the keyword -
alone; `detailed=True` on a model without the flag raises.  The GPU half is tests/test_gpu_logprobs.py."""
import math
import threading
from concurrent.futures import Future

import numpy as np
import pytest

import abi_pins
from sonicscribe_amd import asr
from sonicscribe_amd.dispatch import Dispatcher, Request

NEW = ["sonic_fetch_logprobs", "sonic_fetch_rows_lp", "sonic_dispatch_next_lp", "sonic_pipeline_submit_lp", "sonic_test_greedy_lp"]


def test_abi_header_exports_and_binding_agree():
    abi_pins.check_surface(names=NEW, header_strings=("connection_manager.py:159,274",))      # the reference interface the new entries stand in for


def test_transcription_object():
    t = asr.Transcription("7 8", [7, 8, 990], [-0.5, -1.5, -4.0])      # 990: the EOS that stopped the row counts
    assert t.text == "7 8" and t.token_ids.dtype == np.int32 and t.token_logprobs.dtype == np.float32
    assert t.avg_logprob == pytest.approx(-2.0) and len(t.token_logprobs) == 3
    e = asr.Transcription("", [], [])
    assert math.isnan(e.avg_logprob) and e.token_logprobs.shape == (0,) and e.token_ids.shape == (0,)


def test_text_future_detailed_and_errors():
    inner = Future()
    out = asr._text_future(inner, lambda ids: " ".join(str(int(i)) for i in ids if int(i) != 990), True)
    inner.set_result((np.array([5, 6, 990], np.int32), np.array([-1.0, -2.0, -3.0], np.float32)))
    r = out.result(timeout=1)
    assert r.text == "5 6" and r.token_ids.tolist() == [5, 6, 990] and r.avg_logprob == pytest.approx(-2.0)
    inner2 = Future()
    out2 = asr._text_future(inner2, str, True)
    inner2.set_exception(RuntimeError("boom"))
    with pytest.raises(RuntimeError):
        out2.result(timeout=1)


def test_detailed_needs_the_flag():
    m = asr.ASRModel.__new__(asr.ASRModel)                             # no device: only the surface's own check
    m.model = object(); m.token_logprobs = False
    with pytest.raises(ValueError, match="token_logprobs"):
        m.submit(np.zeros(1600, np.float32), detailed=True)
    with pytest.raises(ValueError, match="token_logprobs"):
        m._check_detailed(True)
    m._check_detailed(False)
    m.__dict__.clear()


# ------------------------------------------------------------------------------------------ schedulers over stub engines
def _ids(w, prompt, max_new):
    return np.asarray([int(sum(int(x.sum()) for x in w)) % 1000, len(prompt), max_new], np.int32)


def _lp(ids):
    return (-np.asarray(ids, np.float32) / 1000 - 0.25).astype(np.float32)


class PlainStub:
    """an engine that has never heard of log-probabilities (the stub of tests/test_dispatch.py)"""
    max_batch = 4

    def __init__(self):
        self.calls = []

    def transcribe_batch(self, segs, prompts, max_new, req_win=None):
        self.calls.append(False)
        return [_ids(segs[req_win[r]:req_win[r + 1]], prompts[r], max_new[r]) for r in range(len(prompts))], None


class LpStub(PlainStub):
    def transcribe_batch(self, segs, prompts, max_new, req_win=None, want_logprobs=False):
        self.calls.append(want_logprobs)
        ids = [_ids(segs[req_win[r]:req_win[r + 1]], prompts[r], max_new[r]) for r in range(len(prompts))]
        return (ids, None, [_lp(i) for i in ids]) if want_logprobs else (ids, None)


def seg(v, n=16):
    return np.full(n, v, np.int16)


def test_request_carries_the_flag():
    assert Request([seg(1)], [1], 4).want_logprobs is False and Request([seg(1)], [1], 4, True).want_logprobs is True


def test_batch_replica_resolves_ids_and_logprobs():
    e = LpStub()
    d = Dispatcher([e])
    f1 = d.submit([seg(3)], [1, 2], 15, want_logprobs=True)
    ids, lps = f1.result(timeout=5)
    assert ids.tolist() == [48, 2, 15] and lps.dtype == np.float32 and np.array_equal(lps, _lp(ids))
    plain = d.submit([seg(3)], [1, 2], 15).result(timeout=5)
    assert isinstance(plain, np.ndarray) and plain.tolist() == [48, 2, 15]
    assert e.calls == [True, False]                                    # the keyword reaches the engine only when somebody asked
    d.close()
    p = PlainStub()
    d2 = Dispatcher([p])
    assert d2.submit([seg(1)], [1], 15).result(timeout=5).tolist() == [16, 1, 15]
    d2.close()


class ContStub:
    """stub of a continuously decoding handle and its prefill slot: a row finishes at the first step after its splice"""
    max_batch = 4
    token_logprobs = True                                              # (what Engine.set_option("token_logprobs", 1) leaves on a handle and its slots)

    def __init__(self, shared=None):
        self.shared = shared if shared is not None else {"rows": {}, "seq": 0, "fetch_kw": []}
        self.batch = []

    def service_begin(self): pass
    def service_end(self): pass
    def set_option(self, k, v): pass

    def stage_pcm(self, segs, req_win=None):
        self.segs, self.req_win = segs, req_win

    def prefill(self, prompts, max_new, req_win=None):
        self.batch = [_ids(self.segs[req_win[r]:req_win[r + 1]], prompts[r], max_new[r]) for r in range(len(prompts))]

    def splice_rows(self, src, src_rows, dst_rows):
        for s, t in zip(src_rows, dst_rows):
            self.shared["rows"][t] = src.batch[s]
        return self.shared["seq"]

    def service_step(self, n, rows):
        self.shared["seq"] += 1
        fin, nn = np.ones(64, np.int32), np.zeros(64, np.int32)
        for r, ids in self.shared["rows"].items():
            nn[r] = len(ids)
        return fin, nn, self.shared["seq"], 0

    def fetch_row(self, row, n):
        self.shared["fetch_kw"].append(False)
        return self.shared["rows"].pop(row)[:n]

    def fetch_rows(self, rows, counts, want_logprobs=False):
        self.shared["fetch_kw"].append(want_logprobs)
        ids = [self.shared["rows"].pop(r)[:c] for r, c in zip(rows, counts)]
        return (ids, [_lp(i) for i in ids]) if want_logprobs else ids


def test_continuous_replica_resolves_ids_and_logprobs():
    dec = ContStub()
    pre = ContStub(dec.shared)
    d = Dispatcher([dec], slots=[[pre]], continuous=True, native=False)
    ids, lps = d.submit([seg(2)], [1, 2, 3], 15, want_logprobs=True).result(timeout=5)
    assert ids.tolist() == [32, 3, 15] and np.array_equal(lps, _lp(ids))
    plain = d.submit([seg(4)], [1], 15).result(timeout=5)
    assert isinstance(plain, np.ndarray) and plain.tolist() == [64, 1, 15]
    assert dec.shared["fetch_kw"] == [True, False]
    d.close()


class PipeStub:
    batches_in_flight = 2

    def __init__(self, decoders, prefills, block):
        self.kw, self.jobs, self.lock = [], {}, threading.Lock()

    def submit(self, prompts, max_new, segments=None, req_win=None, want_logprobs=False):
        ids = [_ids(segments[req_win[r]:req_win[r + 1]], prompts[r], max_new[r]) for r in range(len(prompts))]
        with self.lock:
            self.kw.append(want_logprobs)
            t = len(self.jobs) + 1
            self.jobs[t] = (ids, [_lp(i) for i in ids]) if want_logprobs else ids
        return t

    def wait(self, ticket):
        return self.jobs[ticket]

    def close(self): pass


def test_bulk_replica_resolves_ids_and_logprobs():
    e = PlainStub()
    pipes = []

    def factory(dec, pre, block):
        pipes.append(PipeStub(dec, pre, block))
        return pipes[-1]
    d = Dispatcher([e], slots=[[PlainStub(), PlainStub()]], bulk=True, decoders=1, pipeline_factory=factory)
    ids, lps = d.submit([seg(5)], [1, 2], 150, want_logprobs=True).result(timeout=5)
    assert ids.tolist() == [80, 2, 150] and np.array_equal(lps, _lp(ids))
    plain = d.submit([seg(6)], [1], 150).result(timeout=5)
    assert isinstance(plain, np.ndarray) and plain.tolist() == [96, 1, 150]
    assert pipes[0].kw == [True, False]
    d.close()


def test_native_replica_refuses_without_the_option():
    from sonicscribe_amd.dispatch import _NativeContinuousReplica
    r = _NativeContinuousReplica.__new__(_NativeContinuousReplica)     # no library: put()'s own check comes first
    r.lp = False
    with pytest.raises(ValueError, match="token_logprobs"):
        r.put(Request([seg(1)], [1], 4, True))


def test_continuous_replica_refuses_up_front_without_the_option():
    """stub handles that do not carry the option: the request is refused at put(), before a decode thread's fetch could fail its neighbours' rows"""
    dec = ContStub()
    pre = ContStub(dec.shared)
    dec.token_logprobs = True; pre.token_logprobs = False
    d = Dispatcher([dec], slots=[[pre]], continuous=True, native=False)
    with pytest.raises(ValueError, match="token_logprobs"):
        d.submit([seg(2)], [1, 2, 3], 15, want_logprobs=True)
    assert d.submit([seg(4)], [1], 15).result(timeout=5).tolist() == [64, 1, 15]
    d.close()


def test_python_pipeline_fetches_logprobs():
    """pipeline.ContinuousPipeline.run(want_logprobs=True): check() gets (ids, logprobs) of every row"""
    from sonicscribe_amd.pipeline import ContinuousPipeline
    dec = ContStub()
    pre = ContStub(dec.shared)
    pipe = ContinuousPipeline([dec], [pre], block=2)
    seen = []

    def prefill(slot):
        slot.stage_pcm([seg(1), seg(2)], [0, 1, 2]); slot.prefill([[1], [1, 2]], [3, 4], [0, 1, 2])

    def check(i, got):
        ids, lp = got
        seen.append(i)
        return np.array_equal(lp, _lp(ids)) and ids.tolist() == [16 * (i + 1), i + 1, 3 + i]
    res = pipe.run(2, prefill, check, want_logprobs=True)
    assert res["batches"] == 2 and res["wrong_rows"] == 0 and sorted(seen) == [0, 0, 1, 1]
    assert all(dec.shared["fetch_kw"])
    res = pipe.run(1, prefill, lambda i, ids: isinstance(ids, np.ndarray))
    assert res["wrong_rows"] == 0 and dec.shared["fetch_kw"][-1] is False
    pipe.close()
