"""Row forks end to end on the GPU (sonic_load_tensor "request_forks", Engine.transcribe_batch / prefill `forks=`), on TINY with max_batch 8: every
row of a forked run is the solo run of its (audio, temperature, seed) - ids, log-probability bits and dumped logits - on the hipGraph and the eager path, under
guards, per-row bias tables and grammars, after a splice; the refusals by name; fork_kv_kernel's copy read back from the cache, element by element."""
import ctypes
import dataclasses
from functools import partial

import numpy as np
import pytest

import gpu_common
from gpu_common import SEED, flags, make_engine, same_bits, six
from sonicscribe_amd import spec, synth
from sonicscribe_amd.engine import Engine, SonicError
from sonicscribe_amd.grammar import Grammar
from sonicscribe_amd.reqbias import RequestBias

pytestmark = pytest.mark.gpu
D = spec.TINY
EOS = list(D.eos_ids)
FORKS = [3, 1, 2]
BUDGETS = [14, 20, 9]
# one (temperature, seed) per ROW, in the order of Engine.fork_rows(FORKS) = [[0, 3, 4], [1], [2, 5]]
SAMP = [(0.0, 1), (0.9, 12), (1.0, 0x123456789ABCDEF0), (0.8, 21), (1.2, 22), (0.7, 33)]
prompt_for = partial(gpu_common.prompt_for, D)      # (window lengths of one request)


def audios():
    """three requests from gpu_common.six, the second one of two windows: (windows per request, prompts, req_win)"""
    seg = six()[0]
    wins = [[seg[0]], [seg[2], seg[3]], [seg[4]]]
    return wins, [prompt_for([len(w) for w in ws]) for ws in wins]


def flat(wins):
    segs = [w for ws in wins for w in ws]
    rw = np.concatenate([[0], np.cumsum([len(ws) for ws in wins])]).tolist()
    return segs, rw


def make(bias=False, grammar=False, guards=None):
    return make_engine(D, 0, 8, 1024, [("token_logprobs", 1), ("sampling", 1)]
                       + flags((bias, "request_bias", 1), (grammar, "grammar", 1), (guards, "generation", guards)))


def row_source():
    """row -> request, from the one statement of the row order"""
    src = {}
    for a, rows in enumerate(Engine.fork_rows(FORKS)):
        for r in rows:
            src[r] = a
    return [src[r] for r in range(sum(FORKS))]


def solo_rows(e, samp, bias=None, grammar=None):
    """the reference: every row's (audio, t, seed, table, grammar) as a batch of its own, eager, with its logits"""
    wins, prompts = audios()
    out = []
    for r, a in enumerate(row_source()):
        kw = {}
        if bias is not None:
            kw["request_bias"] = [bias[r]]
        if grammar is not None:
            kw["request_grammar"] = [grammar[r]]
        ids, lg, lp = e.transcribe_batch(wins[a], [prompts[a]], [BUDGETS[a]], req_win=[0, len(wins[a])], want_logits=True, want_logprobs=True,
                                         request_sampling=[samp[r]], **kw)
        out.append((ids[0], lg[:len(ids[0]), 0].copy(), lp[0]))
    return out


def forked(e, samp, want_logits, **kw):
    wins, prompts = audios()
    segs, rw = flat(wins)
    return e.transcribe_batch(segs, prompts, BUDGETS, req_win=rw, want_logits=want_logits, want_logprobs=True, request_sampling=samp, forks=FORKS, **kw)


def check_rows(got_ids, got_lp, want, got_logits=None, what=""):
    assert len(got_ids) == len(want) == sum(FORKS)
    for r, (ids, lg, lp) in enumerate(want):
        assert np.array_equal(got_ids[r], ids), (what, r, got_ids[r].tolist(), ids.tolist())
        assert same_bits(got_lp[r], lp), (what, r)
        if got_logits is not None:
            assert same_bits(got_logits[:len(ids), r], lg), (what, r)


@pytest.fixture(scope="module")
def eng():
    e = make()
    yield e
    e.close()


@pytest.fixture(scope="module")
def solo(eng):
    return solo_rows(eng, SAMP)


# ------------------------------------------------------------------------------------------ 1. every row is its solo run
def test_rows_equal_their_solo_runs(eng, solo):
    wins, prompts = audios()
    greedy = [eng.transcribe_batch(wins[a], [prompts[a]], [BUDGETS[a]], req_win=[0, len(wins[a])])[0][0] for a in range(3)]
    src = row_source()
    assert np.array_equal(solo[0][0], greedy[0]), "row 0 decodes at t = 0"
    assert any(SAMP[r][0] > 0 and not np.array_equal(solo[r][0], greedy[src[r]]) for r in range(6)), "no sampled row left the greedy path: the test shows nothing"
    assert not np.array_equal(solo[3][0], solo[4][0]), "two forks of one audio with different seeds drew the same transcript"
    ids_g, none, lp_g = forked(eng, SAMP, False)                 # the hipGraph loop
    assert none is None
    check_rows(ids_g, lp_g, solo, what="graph")
    ids_e, lg_e, lp_e = forked(eng, SAMP, True)                  # eager, with the dumped logits
    assert lg_e.shape == (max(BUDGETS), 6, D.vocab)
    check_rows(ids_e, lp_e, solo, lg_e, what="eager")
    # the forks of one audio are drawn from the same first logits
    assert same_bits(lg_e[0, 0], lg_e[0, 3]) and same_bits(lg_e[0, 0], lg_e[0, 4]) and same_bits(lg_e[0, 2], lg_e[0, 5])


# ------------------------------------------------------------------------------------------ 2. guards, per-row bias tables, grammars
def test_guards_bias_and_grammars_per_row():
    guards = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[304, 10])
    e = make(bias=True, grammar=True, guards=guards)
    try:
        bias = [RequestBias([[[411], 6.0]]), None, RequestBias(bad_words_ids=[[500]]), RequestBias([[[205], 9.0], [[205, 206], 9.0]]), RequestBias(bad_words_ids=[[411], [412]]), None]
        want = solo_rows(e, SAMP, bias=bias)
        assert not np.array_equal(want[0][0], want[3][0]) or not np.array_equal(want[3][0], want[4][0])
        ids_g, _, lp_g = forked(e, SAMP, False, request_bias=bias)
        check_rows(ids_g, lp_g, want, what="graph")
        ids_e, lg_e, lp_e = forked(e, SAMP, True, request_bias=bias)
        check_rows(ids_e, lp_e, want, lg_e, what="eager")
        # two grammars on the two forks of one audio
        ga = Grammar.from_token_sequences([[205, 206, 207], [411, 412, 413, 414]], EOS, vocab=D.vocab, audio_token_id=D.audio_token_id)
        gb = Grammar.from_token_sequences([[600, 601], [600, 601, 602, 603], [620]], EOS, vocab=D.vocab, audio_token_id=D.audio_token_id)
        da, db = e.grammar_create(ga), e.grammar_create(gb)
        wins, prompts = audios()
        samp2 = [(0.0, 0), (0.9, 7)]
        ref = [e.transcribe_batch(wins[0], [prompts[0]], [12], want_logprobs=True, request_sampling=[samp2[j]], request_grammar=[g]) for j, g in enumerate((da, db))]
        ids, _, lps = e.transcribe_batch(wins[0], [prompts[0]], [12], want_logprobs=True, request_sampling=samp2, request_grammar=[da, db], forks=[2])
        for j, g in enumerate((ga, gb)):
            assert np.array_equal(ids[j], ref[j][0][0]) and same_bits(lps[j], ref[j][2][0]), j
            assert g.walk(ids[j]) == "accepted", (j, ids[j])
        da.close(); db.close()                                   # every row has ended and was fetched: nothing refers to the grammars
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 3. capacity and refusals
def _plain(e):
    wins, prompts = audios()
    return e.transcribe_batch(wins[0], [prompts[0]], [6], want_logprobs=True)


def test_capacity_and_refusals(eng):
    wins, prompts = audios()
    one = lambda **kw: eng.transcribe_batch(wins[0], [prompts[0]], [6], want_logprobs=True, **kw)
    base = _plain(eng)
    ids, _, lp = one(forks=[8])                                  # R' == max_batch
    assert len(ids) == 8 and all(np.array_equal(i, base[0][0]) for i in ids) and all(same_bits(x, base[2][0]) for x in lp)
    # the wrapper validates before anything is armed
    for bad, kw in (("9 rows", dict(forks=[9])), ("at least 1", dict(forks=[0])), ("2 counts", dict(forks=[1, 1])), ("request_sampling", dict(forks=[2], request_sampling=[(0.5, 1)])),
                    ("drafts", dict(forks=[2], request_draft=[[5]]))):
        with pytest.raises(ValueError, match="forks"):
            one(**kw)

    # ... and the library refuses each by name: the counts staged directly, then a plain consuming call
    def staged(counts, **kw):
        eng._arm_forks(np.ascontiguousarray(counts, dtype=np.int32))
        return one(**kw)
    for counts, text in (([9], "9 rows"), ([0], "fork count of 0"), ([-2], "fork count")):
        with pytest.raises(SonicError, match="request_forks.*" + text):
            eng._arm_forks(np.ascontiguousarray(counts, dtype=np.int32))
    with pytest.raises(SonicError, match="request_forks.*2 requests, the batch has 1"):
        staged([1, 2])
    with pytest.raises(SonicError, match="request_forks.*sonic_set_request_sampling gave values for 1 rows, the forked batch has 2"):
        staged([2], request_sampling=[(0.5, 1)])
    eng.set_forced_ids(np.full((1, 6), 5, np.int32))
    try:
        with pytest.raises(SonicError, match="request_forks.*forced ids"):
            staged([2])
    finally:
        eng.set_forced_ids(None)
    # a consuming call that fails leaves no counts behind: the next plain call is unforked
    eng._arm_forks(np.ascontiguousarray([3], dtype=np.int32))
    with pytest.raises(ValueError, match="do not match"):
        eng.transcribe_batch(wins[0], [prompts[0][:-8]], [6])
    again = _plain(eng)
    assert len(again[0]) == 1 and np.array_equal(again[0][0], base[0][0]) and same_bits(again[2][0], base[2][0])
    # the kinds and handles that have no forks
    for mode, text in ((1, "int8"), (3, "fp32")):
        k = Engine(D, 0, mode, max_batch=2, max_ctx=1024)
        try:
            k.load_synthetic(SEED)
            with pytest.raises(SonicError, match="request_forks.*" + text):
                k._arm_forks(np.ascontiguousarray([2], dtype=np.int32))
        finally:
            k.close()
    sc = eng.slot()
    try:
        sc.set_option("forced_parallel", 1)
        with pytest.raises(SonicError, match="request_forks.*forced_parallel"):
            sc._arm_forks(np.ascontiguousarray([2], dtype=np.int32))
    finally:
        sc.close()
    dv = Engine(D, 0, 0, max_batch=4, max_ctx=1024)
    try:
        dv.set_option("draft_verify", 1)
        dv.load_synthetic(SEED)
        dv.set_request_draft([[5, 6]])
        dv._arm_forks(np.ascontiguousarray([2], dtype=np.int32))
        with pytest.raises(SonicError, match="request_forks.*request_draft"):
            dv.transcribe_batch(wins[0], [prompts[0]], [6])
        assert len(dv.transcribe_batch(wins[0], [prompts[0]], [6])[0]) == 1      # both were consumed
    finally:
        dv.close()


# ------------------------------------------------------------------------------------------ 4. a forked prefill on a slot, spliced into a continuous loop
def test_forked_prefill_spliced(eng, solo):
    wins, prompts = audios()
    segs, rw = flat(wins)
    pre = eng.slot()
    eng.service_begin()
    try:
        pre.stage_pcm(segs, req_win=rw)
        pre.prefill(prompts, BUDGETS, req_win=rw, request_sampling=SAMP, forks=FORKS)
        src_rows, dst_rows = [0, 3, 4, 1, 2, 5], [6, 1, 4, 0, 7, 2]      # sources and forks, into scattered rows
        seq = eng.splice_rows(pre, src_rows, dst_rows)
        want = dict(zip(dst_rows, src_rows))
        got = {}
        for _ in range(300):
            fin, nn, s_, _ = eng.service_step(1, 8)
            done = [r for r in want if r not in got and s_ > seq and fin[r]]
            if done:
                a, b = eng.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                for r, x, y in zip(done, a, b):
                    got[r] = (x, y)
            if len(got) == len(want):
                break
        assert len(got) == len(want)
        for dst, src in want.items():
            assert np.array_equal(got[dst][0], solo[src][0]) and same_bits(got[dst][1], solo[src][2]), (dst, src)
    finally:
        eng.service_end()
        pre.close()


def test_forked_prefill_then_decode_steps(eng, solo):
    """the stage entry points: prefill(forks=), decode_step, fetch_tokens over R' rows"""
    wins, prompts = audios()
    segs, rw = flat(wins)
    eng.stage_pcm(segs, req_win=rw)
    eng.prefill(prompts, BUDGETS, req_win=rw, request_sampling=SAMP, forks=FORKS)
    first = eng.fetch_tokens(6, max(BUDGETS))
    assert [len(x) for x in first] == [1] * 6 and [int(x[0]) for x in first] == [int(s[0][0]) for s in solo]
    eng.decode_step(max(BUDGETS))
    ids, lp = eng.fetch_tokens(6, max(BUDGETS), want_logprobs=True)
    check_rows(ids, lp, solo, what="stages")


# ------------------------------------------------------------------------------------------ 5. the kernel, directly
def _cache(e, dims):
    n = e.max_batch * dims.dec_kv_heads * e.max_ctx * dims.dec_head_dim
    out = []
    for name in (b"kcache", b"vcache"):
        layers = []
        for l in range(dims.dec_layers):
            buf = np.empty(n, np.float32)
            e._check(e.lib.sonic_debug_read(e.h, name, l, buf.ctypes.data_as(ctypes.c_void_p), n))
            layers.append(buf.reshape(e.max_batch, dims.dec_kv_heads, e.max_ctx, dims.dec_head_dim))
        out.append(layers)
    return out


@pytest.mark.parametrize("kv_heads", [1, 2])
def test_fork_kv_kernel_copies_exactly(kv_heads):
    """all eight rows are first filled by an unforked batch of long segments; forks = [4, 4] over two shorter ones with budget 1 then leaves, in every layer and
    head, the sources' first P * head_dim elements in each fork's row, bit for bit (bf16 widened to fp32 is exact), and behind them what the first batch left"""
    dims = D if kv_heads == 1 else dataclasses.replace(D, dec_heads=4, dec_kv_heads=2)
    e = Engine(dims, 0, 0, max_batch=8, max_ctx=1024)
    try:
        e.load_synthetic(SEED)
        long_segs = [synth.synth_pcm(800 + i, 240000 + 16000 * i) for i in range(8)]
        e.transcribe_batch(long_segs, [prompt_for([len(s)]) for s in long_segs], [1] * 8)
        k0, v0 = _cache(e, dims)
        with pytest.raises(SonicError, match="index 2 out of range"):
            e._check(e.lib.sonic_debug_read(e.h, b"kcache", dims.dec_layers, np.empty(1, np.float32).ctypes.data_as(ctypes.c_void_p), 1))
        short = [synth.synth_pcm(900, 48000), synth.synth_pcm(901, 100000)]
        prompts = [prompt_for([len(s)]) for s in short]
        P = [len(p) for p in prompts]
        assert max(P) < min(len(prompt_for([len(s)])) for s in long_segs)      # behind the copies lies what the long batch wrote
        mem = e.memory_info()
        ids, _ = e.transcribe_batch(short, prompts, [1, 1], forks=[4, 4])
        assert len(ids) == 8 and e.memory_info() == mem
        k1, v1 = _cache(e, dims)
        rows = Engine.fork_rows([4, 4])
        assert rows == [[0, 2, 3, 4], [1, 5, 6, 7]]
        for name, c0, c1 in (("K", k0, k1), ("V", v0, v1)):
            for l in range(dims.dec_layers):
                a0, a1 = c0[l].view(np.uint32), c1[l].view(np.uint32)
                for a, rr in enumerate(rows):
                    assert not np.array_equal(a1[a, :, :P[a]], a0[a, :, :P[a]]), "the prefill wrote nothing new"
                    for r in rr[1:]:
                        assert np.array_equal(a1[r, :, :P[a]], a1[a, :, :P[a]]), (name, l, a, r)
                        assert np.array_equal(a1[r, :, P[a]:], a0[r, :, P[a]:]), (name, l, a, r, "written beyond kv_len")
                    assert np.array_equal(a1[a, :, P[a]:], a0[a, :, P[a]:])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 6. all counts 1; memory
def test_counts_of_one_are_no_counts(eng, solo):
    wins, prompts = audios()
    segs, rw = flat(wins)
    samp = [SAMP[0], SAMP[1], SAMP[2]]
    mem = eng.memory_info()
    a = eng.transcribe_batch(segs, prompts, BUDGETS, req_win=rw, want_logits=True, want_logprobs=True, request_sampling=samp)
    b = eng.transcribe_batch(segs, prompts, BUDGETS, req_win=rw, want_logits=True, want_logprobs=True, request_sampling=samp, forks=[1, 1, 1])
    for r in range(3):
        assert np.array_equal(a[0][r], b[0][r]) and same_bits(a[2][r], b[2][r]) and same_bits(a[1][:len(a[0][r]), r], b[1][:len(a[0][r]), r])
        assert np.array_equal(a[0][r], solo[r][0])
    forked(eng, SAMP, False)
    assert eng.memory_info() == mem
