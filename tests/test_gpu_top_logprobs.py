"""Option top_logprobs through the engine: the K best alternatives of every step ride in the tokens' log-probability records, from the prefill's first
token to the last one of the decode loop, on every scheduler.  TINY dimensions, 4 requests of unequal length, about 16 tokens.

Reference: NumPy's stable sort by -logit of the step logits the engine returns (want_step_logits; no processors: they ARE the scores the sum runs over); ids must
be equal, every log-probability within DESIGN.md 6.3's derived bound of float64 log_softmax (check_lp of test_gpu_request_bias.py).  Tokens and token_logprobs are
those of a K = 0 engine bit for bit, and a request's records are the same bits whichever way it is scheduled.  The kernel's own cases (ties, placed maxima, the six
families, the -1 / -inf fill) are tests/test_gpu_top_logprobs_kernel.py."""
import numpy as np
import pytest

from gpu_common import SEED, bits, check_lp, flags, make_engine, prompt_for
from sonicscribe_amd import spec, synth
from sonicscribe_amd.engine import TokenScores

pytestmark = pytest.mark.gpu
K = 8
D = spec.TINY
SEGS = [synth.synth_pcm(700 + i, n) for i, n in enumerate((48000, 200000, 80000, 64000))]
BUDGETS = [5, 17, 11, 16]
PROMPTS = [prompt_for(D, len(s)) for s in SEGS]


def make(k=K, max_batch=4):
    return make_engine(D, 0, max_batch, 1024, [("token_logprobs", 1)] + flags((k, "top_logprobs", k)))


def same(a: TokenScores, b: TokenScores):
    return np.array_equal(bits(a.lp), bits(b.lp)) and np.array_equal(bits(a.top_logprobs), bits(b.top_logprobs)) and np.array_equal(a.top_ids, b.top_ids)


@pytest.fixture(scope="module")
def eng():
    e = make(max_batch=8)
    yield e
    e.close()


@pytest.fixture(scope="module")
def solo(eng):
    """the four requests as one staged batch with step logits (sonic_run_staged, want_step_logits): (ids, logits [steps, R, V], TokenScores per request) -
    computed once, left unchanged"""
    R, ld = len(SEGS), max(BUDGETS)
    eng.stage_pcm(SEGS)
    eng.run_staged(PROMPTS, BUDGETS, want_logits=True)
    out, out_len, logits = np.zeros((R, ld), np.int32), np.zeros(R, np.int32), np.zeros((ld, R, D.vocab), np.float32)
    eng._check(eng.lib.sonic_fetch_tokens(eng.h, out.ctypes.data, ld, out_len.ctypes.data, logits.ctypes.data))
    assert out_len.tolist() == BUDGETS
    return [out[r, :out_len[r]].copy() for r in range(R)], logits, eng._fetch_logprobs(out_len, ld)


def test_every_step_against_numpy(eng, solo):
    """every step of every row, the prefill's first token included: ids = NumPy's top 8 of the step logits, log-probabilities within the bound; column 0 is the
    emitted token with its log-probability's bits"""
    ids, logits, sc = solo
    for r in range(len(SEGS)):
        s = sc[r]
        assert isinstance(s, TokenScores) and s.lp.shape == (BUDGETS[r],) and s.top_logprobs.shape == (BUDGETS[r], K) and s.top_ids.shape == (BUDGETS[r], K)
        assert s.top_ids.dtype == np.int32 and s.top_logprobs.dtype == np.float32 and len(ids[r]) == BUDGETS[r]
        for n in range(BUDGETS[r]):
            l = logits[n, r]
            want = np.argsort(-l.astype(np.float64), kind="stable")[:K]
            assert s.top_ids[n].tolist() == want.tolist(), (r, n, s.top_ids[n].tolist(), want.tolist())
            for k in range(K):
                check_lp((r, n, k), s.top_logprobs[n, k], l, want[k])
        assert np.array_equal(s.top_ids[:, 0], ids[r]) and np.array_equal(bits(s.top_logprobs[:, 0]), bits(s.lp)), r


def test_tokens_and_logprobs_keep_their_bits(solo):
    ids, _, sc = solo
    off = make(0, max_batch=8)
    try:
        ids0, _, lp0 = off.transcribe_batch(SEGS, PROMPTS, BUDGETS, want_logprobs=True)
        assert off.memory_info()[0] > 0
        for r in range(len(SEGS)):
            assert isinstance(lp0[r], np.ndarray) and np.array_equal(ids0[r], ids[r]) and np.array_equal(bits(lp0[r]), bits(sc[r].lp)), r
    finally:
        off.close()


def test_graph_loop_and_fetch_forms(eng, solo):
    """the hipGraph loop (no step logits) and the raw C fetch: same bits; records beyond a row's count are not written"""
    ids, _, sc = solo
    ids_g, lg, sc_g = eng.transcribe_batch(SEGS, PROMPTS, BUDGETS, want_logprobs=True)
    assert lg is None and all(np.array_equal(ids_g[r], ids[r]) and same(sc_g[r], sc[r]) for r in range(len(SEGS)))
    W, ld = 1 + 2 * K, 20 * (1 + 2 * K)
    buf = np.full((len(SEGS), ld), np.nan, np.float32)
    eng._check(eng.lib.sonic_fetch_logprobs(eng.h, buf.ctypes.data, ld))
    for r in range(len(SEGS)):
        rec = buf[r, :BUDGETS[r] * W].reshape(BUDGETS[r], W)
        assert np.array_equal(bits(rec[:, 0]), bits(sc[r].lp)) and np.array_equal(rec[:, 1 + K:].astype(np.int32), sc[r].top_ids) and np.all(np.isnan(buf[r, BUDGETS[r] * W:]))
    from sonicscribe_amd.engine import SonicError
    with pytest.raises(SonicError, match="out_ld"):
        small = np.zeros((len(SEGS), 20), np.float32)
        eng._check(eng.lib.sonic_fetch_logprobs(eng.h, small.ctypes.data, 20))      # 20 floats hold no 17 records


def test_continuous_scheduler_with_splice(eng, solo):
    """prefilled on a slot, spliced into neighbouring rows of a continuous loop (the first record comes from the prefill): the batch's bits"""
    ids, _, sc = solo
    pre = eng.slot()
    assert pre.top_logprobs == K
    eng.service_begin()
    try:
        pre.stage_pcm(SEGS); pre.prefill(PROMPTS, BUDGETS)
        rows = {2: 0, 3: 1, 4: 2, 5: 3}                                           # destination row -> request
        seq = eng.splice_rows(pre, [rows[r] for r in rows], list(rows))
        got = {}
        for _ in range(200):
            fin, nn, s_, _ = eng.service_step(1, 6)
            done = [r for r in rows if r not in got and s_ > seq and fin[r]]
            if done:
                a, b = eng.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                got.update({r: (x, y) for r, x, y in zip(done, a, b)})
            if len(got) == len(rows):
                break
        assert len(got) == len(rows)
        for row, req in rows.items():
            assert np.array_equal(got[row][0], ids[req]) and same(got[row][1], sc[req]), (row, req)
    finally:
        eng.service_end()
        pre.close()


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_dispatchers(solo, native):
    from sonicscribe_amd.dispatch import Dispatcher
    ids, _, sc = solo
    e = make(max_batch=8)
    try:
        slots = [e.slot(), e.slot()]
        disp = Dispatcher([e], slots=[slots], continuous=True, native=native)
        assert type(disp.replicas[0]).__name__ == ("_NativeContinuousReplica" if native else "_ContinuousReplica")
        futs = [disp.submit([SEGS[i]], PROMPTS[i], BUDGETS[i], want_logprobs=(i != 1)) for i in range(len(SEGS))]
        res = [f.result(timeout=60) for f in futs]
        disp.close()
        for i in (0, 2, 3):
            assert np.array_equal(res[i][0], ids[i]) and same(res[i][1], sc[i]), i
        assert isinstance(res[1], np.ndarray) and np.array_equal(res[1], ids[1])
    finally:
        e.close()


def test_refusals(eng):
    """the option's own rules, a splice between handles of different K, the bulk pipeline"""
    from sonicscribe_amd.engine import Engine, SonicError
    from sonicscribe_amd.pipeline import NativePipeline
    e = Engine(D, 0, 0, max_batch=32, max_ctx=1024)
    try:
        with pytest.raises(SonicError, match="token_logprobs"):
            e.set_option("top_logprobs", 3)                                        # not before token_logprobs
        e.set_option("token_logprobs", 1)
        for bad in (-1, 9):
            with pytest.raises(SonicError, match="0 .. 8"):
                e.set_option("top_logprobs", bad)
        a0 = e.memory_info()[0]
        e.set_option("top_logprobs", 3)
        assert e.memory_info()[0] > a0                                             # the wider buffer is counted
        with pytest.raises(SonicError, match="top_logprobs"):
            e.set_option("token_logprobs", 0)
        e.load_synthetic(SEED)
        slot3 = e.slot()
        e.set_option("top_logprobs", 5)                                            # the owner moves on, the slot keeps what it copied
        slot3.stage_pcm(SEGS[:1]); slot3.prefill(PROMPTS[:1], [4])
        e.service_begin()
        with pytest.raises(SonicError, match="top_logprobs"):
            e.splice_rows(slot3, [0], [0])
        with pytest.raises(SonicError):
            e.set_option("top_logprobs", 3)                                        # work in hand: the loop is running
        e.service_end()
        with pytest.raises(RuntimeError, match="top_logprobs"):
            NativePipeline([e], [slot3], 32)
        slot3.close()
    finally:
        e.close()


def test_asrmodel_surface():
    from sonicscribe_amd.asr import ASRModel, Transcription
    wav = synth.synth_pcm(31, 80000).astype(np.float32) / 32768.0
    m = ASRModel.from_synthetic(D, max_batch=4, max_ctx=1024, token_logprobs=True, top_logprobs=3)
    try:
        r = m.submit(wav, max_new_tokens=12, detailed=True).result(timeout=60)
        n = len(r.token_ids)
        assert isinstance(r, Transcription) and n >= 1 and r.top_token_ids.shape == (n, 3) and r.top_logprobs.shape == (n, 3)
        assert r.top_token_ids.dtype == np.int32 and np.array_equal(r.top_token_ids[:, 0], r.token_ids) and np.array_equal(bits(r.top_logprobs[:, 0]), bits(r.token_logprobs))
        info = m.transcribe(wav, max_new_tokens=12, return_debug_info=True)
        assert np.array_equal(info["top_token_ids"], r.top_token_ids) and np.array_equal(bits(info["top_logprobs"]), bits(r.top_logprobs))
    finally:
        m.close()
