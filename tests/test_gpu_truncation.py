"""top_k / top_p / min_p end to end on the GPU (option truncation, sonic_load_tensor "request_truncation", 5-tuples in `request_sampling`), on TINY
with max_batch 8 and `token_logprobs`, `sampling` and `truncation` on: ids and log-probability bits, no tolerances - a transcript is a pure function of (audio,
prompt, tables, t, seed, cut parameters) on every path; the eager path's dumped logits are replayed through the reference (sonicscribe_amd/sampling.py) under the
kernel test's rule 3."""
import numpy as np
import pytest

from gpu_common import flags, make_engine, same_bits, six
from sonicscribe_amd import sampling, spec, synth

pytestmark = pytest.mark.gpu
CUT = (5, 0.9, 0.05)


def make(mode=0, trunc=True, samp=True, max_batch=8):
    return make_engine(spec.TINY, mode, max_batch, 1024, [("token_logprobs", 1)] + flags((samp, "sampling", 1), (trunc, "truncation", 1)))


@pytest.fixture(scope="module")
def eng():
    e = make()
    yield e
    e.close()


@pytest.fixture(scope="module")
def solo(eng):
    """request 5 at (t, seed, CUT), alone: what every other path must reproduce; and the same request untruncated and greedy"""
    segs, prompts = six()
    ids, _, lp = eng.transcribe_batch([segs[5]], [prompts[5]], [15], want_logprobs=True, request_sampling=[(1.0, 77) + CUT])
    free, _, _ = eng.transcribe_batch([segs[5]], [prompts[5]], [15], want_logprobs=True, request_sampling=[(1.0, 77)])
    greedy, _, glp = eng.transcribe_batch([segs[5]], [prompts[5]], [15], want_logprobs=True)
    assert not np.array_equal(free[0], ids[0]), "the cut changed nothing at t = 1: the test shows nothing"
    return ids[0], lp[0], greedy[0], glp[0]


@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["bf16", "int8", "f16", "f32"])
def test_a_prefix_of_one_is_greedy(mode):
    """top_p = 1e-6 at t = 0.8 emits the greedy row's ids and log-probability bits: a prefix of one id is the first maximum; every kind goes through the same greedy_args"""
    segs, prompts = six()
    e = make(mode)
    try:
        g, _, glp = e.transcribe_batch(segs[:3], prompts[:3], [10, 10, 10], want_logprobs=True)
        ids, _, lp = e.transcribe_batch(segs[:3], prompts[:3], [10, 10, 10], want_logprobs=True, request_sampling=[(0.8, 5, 0, 1e-6, 0.0), (0.8, 6, 40, 1e-6, 0.0), (0.8, 7, 0, 1e-6, 0.3)])
        for r in range(3):
            assert np.array_equal(ids[r], g[r]) and same_bits(lp[r], glp[r]), (mode, r)
    finally:
        e.close()


def test_same_bits_on_the_graph_and_the_eager_path_and_the_replay(eng, solo):
    segs, prompts = six()
    want_ids, want_lp, _, _ = solo
    budgets = [5, 17, 11, 9, 13, 15]
    samp = [(0.7, 11, 50, 0.9, 0.0), (1.0, 12), (0.0, 13, 3, 0.5, 0.5), (0.3, 14, 0, 1.0, 0.2), None, (1.0, 77) + CUT]
    ids_b, _, lp_b = eng.transcribe_batch(segs, prompts, budgets, want_logprobs=True, request_sampling=samp)                         # row 5 of a batch, hipGraph chunks
    assert np.array_equal(ids_b[5], want_ids) and same_bits(lp_b[5], want_lp)
    ids_e, logits, lp_e = eng.transcribe_batch(segs, prompts, budgets, want_logits=True, want_logprobs=True, request_sampling=samp)   # ... and eager
    for r in range(6):
        assert np.array_equal(ids_e[r], ids_b[r]) and same_bits(lp_e[r], lp_b[r]), r
    # neighbouring rows keep their own values: row 1 (a pair) and row 4 (None) are the untruncated and the greedy run of their request
    one, _ = eng.transcribe_batch([segs[1]], [prompts[1]], [17], request_sampling=[(1.0, 12)])
    four, _ = eng.transcribe_batch([segs[4]], [prompts[4]], [13])
    assert np.array_equal(one[0], ids_b[1]) and np.array_equal(four[0], ids_b[4])
    # the replay: every emitted id of a truncated row lies inside the reference's prefix at top_p + EPS_MASS (rule 3's upper end); and, where the two ends agree,
    # it is the first maximum of the contract's y over that prefix up to the noise's EPS_G
    checked = 0
    for r in (0, 3, 5):
        t, seed, k, p, m = samp[r]
        for step in range(len(ids_e[r])):
            raw = logits[step, r]
            y = sampling.quotient(raw, t)
            order = sampling.truncation_order(y)
            lo = min(sampling.truncation_counts(y, k, p, m, -sampling.EPS_MASS if p < 1.0 else 0.0))
            hi = min(sampling.truncation_counts(y, k, p, m, sampling.EPS_MASS if p < 1.0 else 0.0))
            tok = int(ids_e[r][step])
            assert tok in order[:hi], (r, step, tok, lo, hi)
            if lo == hi:
                kept = np.sort(order[:lo])
                yy = sampling.perturbed(raw, t, seed, step)[kept]
                tol = 2 * sampling.EPS_G + float(np.spacing(np.float32(np.abs(yy[np.isfinite(yy)]).max())))
                assert yy[int(np.searchsorted(kept, tok))] >= yy.max() - tol, (r, step, tok)
                checked += 1
    assert checked >= 10, checked


def test_step_wise_spliced_and_forked(eng, solo):
    segs, prompts = six()
    want_ids, want_lp, _, _ = solo
    # prefill / decode_step / fetch_tokens
    eng.stage_pcm([segs[5]]); eng.prefill([prompts[5]], [15], request_sampling=[(1.0, 77) + CUT])
    eng.decode_step(100)
    ids, lp = eng.fetch_tokens(1, 15, want_logprobs=True)
    assert np.array_equal(ids[0], want_ids) and same_bits(lp[0], want_lp)
    # a prefill without staged words after one with them is untruncated
    free, _, flp = eng.transcribe_batch([segs[5]], [prompts[5]], [15], want_logprobs=True, request_sampling=[(1.0, 77)])
    assert not np.array_equal(free[0], want_ids)
    # spliced into scattered rows of a continuous loop: the words travel with the row
    pre = eng.slot()
    eng.service_begin()
    try:
        pre.stage_pcm([segs[0], segs[5]]); pre.prefill([prompts[0], prompts[5]], [5, 15], request_sampling=[(0.5, 3, 2, 1.0, 0.0), (1.0, 77) + CUT])
        seq = eng.splice_rows(pre, [1, 0], [6, 2])
        got = {}
        for _ in range(300):
            fin, nn, s_, _ = eng.service_step(1, 8)
            done = [r for r in (6, 2) if r not in got and s_ > seq and fin[r]]
            if done:
                a, b = eng.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                for r, x, y in zip(done, a, b):
                    got[r] = (x, y)
            if len(got) == 2:
                break
        assert len(got) == 2 and np.array_equal(got[6][0], want_ids) and same_bits(got[6][1], want_lp)
    finally:
        eng.service_end()
        pre.close()
    # forks [3, 1] with per-fork values: rows 0, 2, 3 are request 5's forks, row 1 is request 0
    rows = [(1.0, 77) + CUT, (0.5, 3, 2, 1.0, 0.0), (1.0, 77), (1.0, 78) + CUT]
    ids, _, lp = eng.transcribe_batch([segs[5], segs[0]], [prompts[5], prompts[0]], [15, 5], want_logprobs=True, request_sampling=rows, forks=[3, 1])
    assert np.array_equal(ids[0], want_ids) and same_bits(lp[0], want_lp)
    assert np.array_equal(ids[2], free[0]) and same_bits(lp[2], flp[0])
    other, _, olp = eng.transcribe_batch([segs[5]], [prompts[5]], [15], want_logprobs=True, request_sampling=[(1.0, 78) + CUT])
    assert np.array_equal(ids[3], other[0]) and same_bits(lp[3], olp[0])


def test_through_the_native_dispatcher_and_the_python_one(eng, solo):
    """the (t, seed, 5, 0.9, 0.05) request among pairs and greedy requests on both continuous schedulers: its solo run's ids and log-probability bits"""
    from sonicscribe_amd.dispatch import Dispatcher
    segs, prompts = six()
    want_ids, want_lp, _, _ = solo
    budgets = [5, 17, 11, 9, 13, 15]
    samp = [(0.7, 11, 50, 0.9, 0.0), (1.0, 12), None, (0.3, 14, 0, 1.0, 0.2), (0.0, 15, 3, 0.5, 0.5), (1.0, 77) + CUT]
    ids_b, _, lp_b = eng.transcribe_batch(segs, prompts, budgets, want_logprobs=True, request_sampling=samp)
    assert np.array_equal(ids_b[5], want_ids) and same_bits(lp_b[5], want_lp)
    for native in (False, True):
        slots = [eng.slot(), eng.slot()]
        disp = Dispatcher([eng], slots=[slots], continuous=True, native=native)
        try:
            assert type(disp.replicas[0]).__name__ == ("_NativeContinuousReplica" if native else "_ContinuousReplica")
            futs = [disp.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True, sampling=samp[i]) for i in range(6)]
            res = [f.result(timeout=120) for f in futs]
        finally:
            disp.close()
            for s in slots:
                s.close()
        for i in range(6):
            assert np.array_equal(res[i][0], ids_b[i]) and same_bits(res[i][1], lp_b[i]), (native, i)


def test_model_keywords_end_to_end():
    """ASRModel(top_k=, top_p=) as defaults and per call: a sampled transcript is the engine's own for (t, seed, cut), reported in the Transcription and the debug
    dictionary; refusals by name"""
    from sonicscribe_amd.asr import ASRModel
    wav = synth.synth_pcm(31, 80000).astype(np.float32) / 32768.0
    plain = ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, token_logprobs=True)
    try:
        with pytest.raises(ValueError, match="sampling"):
            plain.submit(wav, max_new_tokens=12, top_k=5)
    finally:
        plain.close()
    with pytest.raises(ValueError, match="bulk"):
        ASRModel.from_synthetic(spec.TINY, max_batch=32, max_ctx=1024, token_logprobs=True, sampling=True, top_k=5, bulk=True)
    m = ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, token_logprobs=True, sampling=True, top_k=5, top_p=0.9)
    try:
        free = m.submit(wav, max_new_tokens=12, detailed=True, temperature=1.0, seed=5, top_k=0, top_p=1.0).result(timeout=60)
        cut = m.submit(wav, max_new_tokens=12, detailed=True, temperature=1.0, seed=5).result(timeout=60)                        # the constructor's defaults
        same = m.submit(wav, max_new_tokens=12, detailed=True, temperature=1.0, seed=5, top_k=5, top_p=0.9, min_p=0.0).result(timeout=60)
        assert (free.top_k, free.top_p, free.min_p) == (0, 1.0, 0.0) and (cut.top_k, cut.top_p, cut.min_p) == (5, 0.9, 0.0)
        assert np.array_equal(cut.token_ids, same.token_ids) and same_bits(cut.token_logprobs, same.token_logprobs)
        assert not np.array_equal(cut.token_ids, free.token_ids), "the cut changed nothing at t = 1: the test shows nothing"
        one = m.submit(wav, max_new_tokens=12, detailed=True, temperature=1.0, seed=5, top_p=1e-6).result(timeout=60)             # a prefix of one: the greedy transcript
        greedy = m.submit(wav, max_new_tokens=12, detailed=True).result(timeout=60)
        assert np.array_equal(one.token_ids, greedy.token_ids) and same_bits(one.token_logprobs, greedy.token_logprobs) and (greedy.top_k, greedy.top_p) == (0, 1.0)
        assert m.transcribe_batch([wav], max_new_tokens=12, temperature=1.0, seed=5) == [cut.text]
        info = m.transcribe(wav, max_new_tokens=12, return_debug_info=True, temperature=1.0, seed=5, min_p=0.01)
        assert (info["top_k"], info["top_p"], info["min_p"]) == (5, 0.9, 0.01)
    finally:
        m.close()


def test_memory_and_refusals():
    from sonicscribe_amd.engine import DTYPE_F32, SonicError
    import ctypes as C
    segs, prompts = six()
    e = make(trunc=False, samp=False, max_batch=32)      # (32 rows: the bulk pipeline's block, for its refusal below)
    try:
        with pytest.raises(SonicError, match="sampling"):                     # refused by name unless sampling is on
            e.set_option("truncation", 1)
        e.set_option("sampling", 1)
        a0 = e.memory_info()[0]
        e.transcribe_batch(segs[:2], prompts[:2], [4, 4], request_sampling=[(0.5, 1), (0.5, 2)])
        assert e.memory_info()[0] == a0                                        # off is off: nothing is allocated without the option
        with pytest.raises(SonicError, match="truncation"):
            e.set_request_sampling([(0.5, 1, 5, 0.9, 0.0)])
        e.stage_pcm(segs[:1]); e.prefill(prompts[:1], [8])                     # (consumes the pair the refused call left)
        with pytest.raises(SonicError, match="running"):                       # refused while work is in hand
            e.set_option("truncation", 1)
        e.decode_step(100)
        e.set_option("truncation", 1)
        a1 = e.memory_info()[0]
        print(f"truncation: sonic_memory_info grows by {a1 - a0} bytes (64 rows x 3 words)")
        assert a1 - a0 == 64 * 3 * 4
        with pytest.raises(SonicError, match="truncation"):
            e.set_option("sampling", 0)
        for bad, name in (((0.5, 1, -1, 0.9, 0.0), "top_k"), ((0.5, 1, 0, 0.0, 0.0), "top_p"), ((0.5, 1, 0, float("nan"), 0.0), "top_p"), ((0.5, 1, 0, 1.5, 0.0), "top_p"),
                          ((0.5, 1, 0, 0.9, -0.5), "min_p"), ((0.5, 1, 0, 0.9, float("nan")), "min_p")):
            with pytest.raises(ValueError, match=name):                        # Python's check ...
                e.set_request_sampling([bad])
            row = np.array([bad[2:]], np.float32)                              # ... and the library's own behind it
            assert e.lib.sonic_load_tensor(e.h, b"request_truncation", row.ctypes.data_as(C.c_void_p), DTYPE_F32, (C.c_int64 * 2)(1, 3), 2) == 1
            assert name.encode() in e.lib.sonic_last_error(e.h)
        e.set_request_sampling([(0.5, 1, 5, 0.9, 0.0)])                        # values for one row, a batch of two: refused by name, and consumed
        with pytest.raises(SonicError, match="request_truncation|sonic_set_request_sampling"):
            e.transcribe_batch(segs[:2], prompts[:2], [4, 4])
        g0, _ = e.transcribe_batch(segs[:2], prompts[:2], [8, 8])
        g1, _ = e.transcribe_batch(segs[:2], prompts[:2], [8, 8])
        assert all(np.array_equal(g0[r], g1[r]) for r in range(2))
        # the bulk pipeline refuses the request by name, whatever the handles have
        from sonicscribe_amd.dispatch import Dispatcher
        slots = [e.slot(), e.slot()]
        bulk = Dispatcher([e], slots=[slots], bulk=True, decoders=1)
        with pytest.raises(ValueError, match="bulk"):
            bulk.submit([segs[0]], prompts[0], 4, sampling=(0.5, 1, 5, 0.9, 0.0))
        bulk.close()
        # a native scheduler over handles without the option refuses the cut by name
        for s_ in slots:
            s_.set_option("truncation", 0)
        e.set_option("truncation", 0)
        disp = Dispatcher([e], slots=[slots], continuous=True, native=True)
        with pytest.raises(ValueError, match="truncation"):
            disp.submit([segs[0]], prompts[0], 4, sampling=(0.5, 1, 5, 0.9, 0.0))
        disp.close()
        for s_ in slots:
            s_.close()
        e.set_option("truncation", 1)
        # a splice between handles whose options differ is refused by name
        pre = e.slot()
        pre.set_option("truncation", 0)
        e.service_begin()
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [4])
        with pytest.raises(SonicError, match="truncation"):
            e.splice_rows(pre, [0], [0])
        e.service_end()
        pre.decode_step(100)
        pre.close()
    finally:
        e.close()
