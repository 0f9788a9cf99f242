"""Per-request sequence bias on the GPU (option request_bias, sonic_set_request_bias; greedy_kernel<T, LP, true, true>): HF's
SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor inside the greedy kernel, one table per row.  The reference is the numpy chain
`GenerationGuards.apply(RequestBias.apply(raw, history), history)`, which tests/test_request_bias_host.py holds bit for bit against HF's own classes: the emitted
token must be np.argmax (first maximum) of the chain over the raw logits the kernel dumped, exactly.  Log-probabilities are held to DESIGN.md 6.3's derived bound
(tests/gpu_common.py lp_bound, the same derivation: the bias adds no rounding to the sum, it changes the scores the sum is taken over), evaluated over
the processed scores."""
import numpy as np
import pytest

from gpu_common import check_lp, flags, load_golden, make_engine, prompt_for, same_bits, six, slabs
from sonicscribe_amd import spec, synth
from sonicscribe_amd.genconfig import GenerationGuards
from sonicscribe_amd.reqbias import RequestBias

pytestmark = pytest.mark.gpu
NEG = float("-inf")


def order_triple():
    """three fp32 values below 16 whose sum depends on the order (the same search as the host test)"""
    rng = np.random.default_rng(7)
    while True:
        a, b, c = rng.uniform(-16, 16, 3).astype(np.float32)
        if np.float32(np.float32(a + b) + c) != np.float32(np.float32(a + c) + b):
            return float(a), float(b), float(c)


def chain(raw, hist, bias, guards=None):
    s = bias.apply(raw, hist) if bias is not None else np.array(raw, np.float32)
    return (guards or GenerationGuards()).apply(s, hist)


def make(d=spec.TINY, mode=0, max_batch=4, max_ctx=1024, lp=False, bias=True, guards=None):
    return make_engine(d, mode, max_batch, max_ctx, flags((lp, "token_logprobs", 1), (bias, "request_bias", 1), (guards, "generation", guards)))


@pytest.fixture(scope="module")
def engines():
    es = {}

    def get(mode):
        if mode not in es:
            es[mode] = make(mode=mode, bias=False)        # the hook takes its tables as arguments: the option plays no part in it
        return es[mode]
    yield get
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    g, segs, prompts = load_golden(golden_dir, int_prompts=True)
    return g, segs, prompts, int(g["n_new"])


# ------------------------------------------------------------------------------------------ 1. the kernel hook, exact
def _edges(V):
    """the group and trip edges of the loop: first id, last id of the first f32x4 group, both sides of the first stride, the last id"""
    return sorted({0, 3, V - 1} | ({4095, 4096} if V > 4096 else set()))


def _histories(V, rng):
    """rows of 1, 40, 17 and 5 ids: none of them an edge id or the ids the tables' fillers use"""
    pool = [1, 2] if V == 8 else [5, 6, 7, 9, 77, V - 4, V - 5]
    hlen = np.array([1, 40, 17, 5], np.int32)
    hist = np.zeros((4, 40), np.int32)
    for b in range(4):
        h = [int(pool[i]) for i in rng.integers(0, len(pool), hlen[b])]
        if hlen[b] >= 2 and h[-1] == h[-2]:
            h[-1] = pool[0] if h[-2] != pool[0] else pool[1]      # the last two differ: a swapped prefix misses
        hist[b, :hlen[b]] = h
    return hist, hlen


def _big_table(V, h, winner, rng):
    """256 entries: a small length-1 bias on every edge id, a matching three-token entry that makes
    `winner` win, a swapped prefix that must miss although it carries the largest bias, a bad word on id 4 of the first group, fillers of 1 .. 8 ids"""
    ent = [[[p], 0.25] for p in _edges(V)]
    ent.append([[h[-2], h[-1], winner], 40.0])
    miss = 2 if V == 8 else V // 2
    ent.append([[h[-1], h[-2], miss], 100.0])
    seen = {tuple(e[0]) for e in ent}
    lo, hi = (4, 8) if V == 8 else (10, min(V, 2000))
    while len(ent) < 255:                                                  # (+ the bad word: 256 in all, at every V)
        L = int(rng.integers(1, 9))
        ids = tuple(int(t) for t in rng.integers(lo, hi, L))
        if ids in seen or (L > 1 and list(ids[:-1]) == h[len(h) - (L - 1):]) or (L == 1 and V == 8):      # (V = 8: single ids are the edges' and the bad word's)
            continue
        seen.add(ids)
        ent.append([list(ids), float(np.float32(rng.uniform(-3, 3)))])
    return RequestBias(ent, bad_words_ids=[[4]]), miss


def _run(eng, V, ks, rows, hist, hlen, tables, guards=None, want_lp=False, force=None, tag=""):
    s = slabs(rows, ks)
    B = len(rows)
    g = GenerationGuards(**(guards or {}))
    tok, raw, lp = eng.test_greedy_bias(s, B, hist[:B], hlen[:B], tables, force_ids=force, want_lp=want_lp, **(guards or {}))
    tok0, raw0 = eng.test_greedy(s, B, want_logits=True)
    assert np.array_equal(raw.view(np.uint32), raw0.view(np.uint32)), (tag, "the dump is the raw logits")
    worst = 0.0
    for b in range(B):
        proc = chain(raw[b], hist[b, :hlen[b]], tables[b], g)
        want = int(np.argmax(proc)) if force is None else int(force[b])
        assert int(tok[b]) == want, (tag, V, ks, b, int(tok[b]), want)
        if want_lp and not np.isneginf(proc).all():
            worst = max(worst, check_lp((tag, V, ks, b), lp[b], proc, tok[b]))
    return tok, tok0, worst


@pytest.mark.parametrize("mode", [0, 2, 3], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("V", [8, 1024, 16388, 59264])
def test_kernel_hook_exact(engines, V, mode):
    eng = engines(mode)
    rng = np.random.default_rng(V)
    hist, hlen = _histories(V, rng)
    a, b3, c = order_triple()
    T = 5 if V == 8 else V // 3
    h2 = [int(t) for t in hist[2, :hlen[2]]]
    triple = RequestBias([[[T], a], [[h2[-1], T], b3], [[h2[-2], h2[-1], T], c]])
    swapped = RequestBias([[[T], a], [[h2[-2], h2[-1], T], c], [[h2[-1], T], b3]])
    live = [6, 7] if V == 8 else [11, V // 5, V - 7]                         # row 3: the only finite scores, every one a bad word
    dead = RequestBias(bad_words_ids=[[t] for t in live])
    worst = 0.0
    for ks in (1, 2, 3):
        for winner in _edges(V)[ks - 1::3]:                                   # every edge id once, spread over the three slab counts
            rows = [rng.uniform(-2.0, 2.0, V).astype(np.float32) for _ in range(4)]
            big, miss = _big_table(V, [int(t) for t in hist[1, :40]], winner, rng)
            rows[1][4] = 9.0                                                   # the raw argmax of row 1 is its bad word
            rows[2][T] = 3.0                                                   # row 2: T + (a + b + c) in list order
            rows[3][:] = NEG; rows[3][live] = [1.0, 2.0, 3.0][:len(live)]
            tables = [None, big, triple, dead]
            for want_lp in (False, True):
                tok, tok0, w = _run(eng, V, ks, rows, hist, hlen, tables, want_lp=want_lp, tag=f"edge{winner}")
                worst = max(worst, w)
                assert int(tok[0]) == int(tok0[0]) and int(tok0[1]) == 4 and int(tok[1]) == winner and int(tok[3]) == 0, (V, ks, winner, tok.tolist())
                assert int(tok[1]) != miss
        # the order of the sum is the contract: the swapped table is another number, and the kernel follows the table it was given
        s_list = np.float32(np.float32(np.float32(np.float32(0.0) + np.float32(a)) + np.float32(b3)) + np.float32(c))
        s_swap = np.float32(np.float32(np.float32(np.float32(0.0) + np.float32(a)) + np.float32(c)) + np.float32(b3))
        assert s_list != s_swap
        rows = [np.full(V, -50.0, np.float32) for _ in range(4)]
        other = 6 if V == 8 else T + 4
        hi = max(s_list, s_swap)
        for r in rows:                                                         # raw 0.0 at both ids: 0.0 + s is s, in every dtype the logits are rounded to
            r[T] = 0.0; r[other] = 0.0
        for tab, s_mine in ((triple, s_list), (swapped, s_swap)):
            # `other` carries exactly the larger of the two sums as a length-1 bias: T wins (lower index, a tie) only where ITS sum is the larger one
            tabs = [None, None, RequestBias([[list(i), float(v)] for i, v in tab.entries] + [[[other], float(hi)]]), None]
            tok, _, w = _run(eng, V, ks, rows, hist, hlen, tabs, want_lp=True, tag="triple")
            assert int(tok[2]) == (T if s_mine == hi else other), (V, ks, float(s_list), float(s_swap))
            worst = max(worst, w)
        # L == len matches, L == len + 1 is ignored although its prefix would fit (row 0: one id, row 3: five); duplicates: the last bias wins; a bad word and a
        # positive bias on one token: -inf
        h0, h3 = [int(hist[0, 0])], [int(t) for t in hist[3, :5]]
        X, Y, Z = (4, 6, 7) if V == 8 else (20, 21, 22)
        rows = [rng.uniform(-2.0, 2.0, V).astype(np.float32) for _ in range(4)]
        tabs = [RequestBias([[h0 + [X], 30.0], [[Y], 20.0], [[Y], 10.0]]),                       # L == len + 1: ignored; Y: 10, not 20 and not 30
                RequestBias([[[Y], 25.0]], bad_words_ids=[[Y]]),                                 # -inf wins over +25
                RequestBias([[h2[-3:] + [Z], 30.0]]),                                            # a match reaching further back
                RequestBias([[h3 + [X], 30.0], [h3[1:] + [Z], 12.0]])]                           # L == len + 1 ignored, L == len matches
        tok, _, w = _run(eng, V, ks, rows, hist, hlen, tabs, want_lp=True, tag="edges of L")
        assert [int(t) for t in tok[[0, 2, 3]]] == [Y, Z, Z] and int(tok[1]) != Y
        worst = max(worst, w)
        # bias with all three guards, and a forced id whose score is recomputed with its bias in the tail
        S = 5 if V == 8 else V - 3
        g3 = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[S])
        rows = [rng.uniform(-2.0, 2.0, V).astype(np.float32) for _ in range(4)]
        for r in rows:
            r[S] = 9.0
        tabs = [RequestBias([[[int(hist[0, 0])], 6.0]]), big, triple, RequestBias([[[h3[-1], Z], 7.5]], bad_words_ids=[[X]])]
        _, _, w = _run(eng, V, ks, rows, hist, hlen, tabs, guards=g3, want_lp=True, tag="with guards")
        worst = max(worst, w)
        force = np.array([int(hist[0, 0]), _edges(V)[-1], T, Z], np.int32)
        _, _, w = _run(eng, V, ks, rows, hist, hlen, tabs, guards=g3, want_lp=True, force=force, tag="forced")
        worst = max(worst, w)
    print(f"bias hook V={V} mode={mode}: worst |lp - ref64| / bound = {worst:.3f}")


def test_neutral_guard_identity(engines):
    """an empty table and the neutral guard values: the GUARD = false kernel's tokens and, with LP, its bits (r * 1.0 and __fdiv_rn(r, 1.0) are exact)"""
    eng = engines(0)
    for V in (8, 1024, 16388):
        rng = np.random.default_rng(100 + V)
        hist, hlen = _histories(V, rng)
        for ks in (1, 2, 3):
            rows = [rng.uniform(-4.0, 4.0, V).astype(np.float32) for _ in range(4)]
            rows[1][V // 2] = -0.0
            s = slabs(rows, ks)
            tok, raw, lp = eng.test_greedy_bias(s, 4, hist, hlen, [None, RequestBias(), None, None], want_lp=True)
            tok0, raw0, lp0 = eng.test_greedy_lp(s, 4)
            assert np.array_equal(tok, tok0) and same_bits(raw, raw0) and same_bits(lp, lp0), (V, ks)


# ------------------------------------------------------------------------------------------ 2. end to end at TINY
def _identity(ids, logits, prompts, tables, n_new, guards=None, eos=spec.TINY.eos_ids):
    """every row, every step: argmax(chain(dumped raw logits, prompt + ids so far)) is the emitted id (the construction of test_end_to_end_eager)"""
    g = GenerationGuards(**(guards or {}))
    for si in range(len(ids)):
        n = len(ids[si])
        assert 1 <= n <= n_new and (n == n_new or int(ids[si][-1]) in eos)
        for s in range(n):
            proc = chain(logits[s, si], list(prompts[si]) + [int(t) for t in ids[si][:s]], tables[si], g)
            assert int(np.argmax(proc)) == int(ids[si][s]), (si, s)


def _fixture_tables(g):
    """per fixture row: a bias on the two-token sequence (its first id, NEW) that makes NEW the second token, and a bad word on the fixture's own second token"""
    out = []
    for si in range(2):
        ref = [int(t) for t in g[f"s{si}_new_ids"]]
        new = 200 + si
        assert new not in ref
        out.append((RequestBias([[[ref[0], new], 1000.0]]), RequestBias(bad_words_ids=[[ref[1]]]), new, ref))
    return out


@pytest.mark.parametrize("kind", ["sequence", "bad_word"])
def test_end_to_end(golden, kind):
    g, segs, prompts, n_new = golden
    ft = _fixture_tables(g)
    tables = [t[0] if kind == "sequence" else t[1] for t in ft]
    e = make()
    try:
        ids, logits = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True, request_bias=tables)
        _identity(ids, logits, prompts, tables, n_new)
        for si in range(2):
            _, _, new, ref = ft[si]
            if kind == "sequence":          # binds at step 1: the fixture's first id, then NEW
                assert int(ids[si][0]) == ref[0] and int(ids[si][1]) == new and ref[1] != new
            else:                           # binds at step 0 where the fixture's first two ids are equal, else at step 1
                assert ref[1] not in [int(t) for t in ids[si]] and [int(t) for t in ids[si]] != ref[:len(ids[si])]
        # consumed: the next batch on this handle starts without tables and gives the fixture's ids
        ids2, _ = e.transcribe_batch(segs, prompts, [n_new, n_new])
        for si in range(2):
            assert np.array_equal(ids2[si], g[f"s{si}_new_ids"][:len(ids2[si])])
    finally:
        e.close()


@pytest.mark.parametrize("mode", [1, 2, 3], ids=["int8", "f16", "f32"])
def test_modes_identity(mode, golden):
    g, segs, prompts, n_new = golden
    e = make(mode=mode)
    try:
        plain, _ = e.transcribe_batch(segs, prompts, [n_new, n_new])
        tables = [RequestBias([[[int(plain[si][0]), 200 + si], 1000.0]], bad_words_ids=[[int(plain[si][min(2, len(plain[si]) - 1)])]]) for si in range(2)]
        ids, logits = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True, request_bias=tables)
        _identity(ids, logits, prompts, tables, n_new)
        assert any(not np.array_equal(ids[si], plain[si]) for si in range(2))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 3. the same bits on every path
def _six():
    return six() + ([5, 17, 11, 9, 13, 7],)


def test_invariance_all_paths():
    from sonicscribe_amd.dispatch import Dispatcher
    segs, prompts, budgets = _six()
    e = make(max_batch=8, lp=True)
    try:
        plain = e.transcribe_batch(segs, prompts, budgets)[0]
        first = [int(p[0]) for p in plain]
        # three tables: both entries bind (a sequence after the first id, another after that one), one binds (the other names an id pair that never
        # occurs), none binds; requests 0, 3 / 1, 4 / 2, 5
        def two(i):
            return RequestBias([[[first[i], 210], 1000.0], [[210, 211], 1000.0]])
        def one(i):
            return RequestBias([[[first[i], 220], 1000.0], [[998, 997, 5], 1000.0]])
        none = lambda i: RequestBias([[[998, 997, 5], 1000.0]], bad_words_ids=[[996, 995]])
        tables = [two(0), one(1), none(2), two(3), one(4), None]
        ids_e, logits_e, lp_e = e.transcribe_batch(segs, prompts, budgets, want_logits=True, want_logprobs=True, request_bias=tables)      # one batch, eager
        for r in range(6):
            for s in range(len(ids_e[r])):
                proc = chain(logits_e[s, r], prompts[r] + [int(t) for t in ids_e[r][:s]], tables[r])
                assert int(np.argmax(proc)) == int(ids_e[r][s]), (r, s)
                check_lp(("paths", r, s), lp_e[r][s], proc, ids_e[r][s])
        for r in (0, 1, 3, 4):
            assert not np.array_equal(ids_e[r], plain[r]), r
        for r in (2, 5):
            assert np.array_equal(ids_e[r], plain[r]), r
        ids_g, _, lp_g = e.transcribe_batch(segs, prompts, budgets, want_logprobs=True, request_bias=tables)                               # one batch, hipGraph loop
        solo = [e.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]], want_logprobs=True, request_bias=[tables[i]]) for i in range(6)]  # solo runs
        for r in range(6):
            assert np.array_equal(ids_g[r], ids_e[r]) and same_bits(lp_g[r], lp_e[r]), r
            assert np.array_equal(solo[r][0][0], ids_e[r]) and same_bits(solo[r][2][0], lp_e[r]), r
        # prefill, then splice into a continuous handle: the table travels with the row (rows land in another order than they were prefilled in)
        pre = e.slot()
        e.service_begin()
        try:
            pre.stage_pcm(segs[:3]); pre.prefill(prompts[:3], budgets[:3], request_bias=tables[:3])
            seq1 = e.splice_rows(pre, [0, 1, 2], [5, 0, 3])
            for _ in range(2):
                e.service_step(1, 8)
            pre.stage_pcm(segs[3:]); pre.prefill(prompts[3:], budgets[3:], request_bias=tables[3:])
            seq = e.splice_rows(pre, [2, 0, 1], [1, 2, 4])
            rows, got = {5: 0, 0: 1, 3: 2, 1: 5, 2: 3, 4: 4}, {}
            for _ in range(300):
                fin, nn, s_, _ = e.service_step(1, 8)
                done = [r for r in rows if r not in got and s_ > max(seq, seq1) and fin[r]]
                if done:
                    a, b = e.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                    for r, x, y in zip(done, a, b):
                        got[r] = (x, y)
                if len(got) == 6:
                    break
            assert len(got) == 6
            for row, req in rows.items():
                assert np.array_equal(got[row][0], ids_e[req]) and same_bits(got[row][1], lp_e[req]), (row, req)
        finally:
            e.service_end()
            pre.close()
        # the Python dispatcher and the native one
        for native in (False, True):
            slots = [e.slot(), e.slot()]
            disp = Dispatcher([e], slots=[slots], continuous=True, native=native)
            assert type(disp.replicas[0]).__name__ == ("_NativeContinuousReplica" if native else "_ContinuousReplica")
            futs = [disp.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True, bias=tables[i]) for i in range(6)]
            res = [f.result(timeout=120) for f in futs]
            disp.close()
            for s in slots:
                s.close()
            for i in range(6):
                assert np.array_equal(res[i][0], ids_e[i]) and same_bits(res[i][1], lp_e[i]), (native, i)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 4. off is off; refusals; memory
def test_off_is_off_and_refusals(golden):
    import ctypes as C
    from sonicscribe_amd.dispatch import Dispatcher
    from sonicscribe_amd.engine import DispatchRequest, SonicError
    g, segs, prompts, n_new = golden
    off = make(lp=True, bias=False)
    try:
        a0 = off.memory_info()[0]
        got = off.transcribe_batch(segs, prompts, [n_new, n_new])
        for si in range(2):                                                    # the parent's fixture ids (the existing tests hold the logits against it)
            n = len(got[0][si])
            assert np.array_equal(got[0][si], g[f"s{si}_new_ids"][:n])
        t = RequestBias([[[5], 1.0]])
        with pytest.raises(SonicError, match="request_bias"):
            off.set_request_bias([t, None])
        slots = [off.slot(), off.slot()]
        disp = Dispatcher([off], slots=[slots], continuous=True, native=True)
        with pytest.raises(ValueError, match="request_bias"):
            disp.submit([segs[0]], prompts[0], 4, bias=t)
        rep = disp.replicas[0]                                                 # ... and the library's own answer, not only the Python check in front of it
        i, o, b = t.table()
        tk = C.c_int64(0)
        pcm = np.ascontiguousarray(segs[0], np.int16); offs = np.array([0, len(pcm)], np.int64); pr = np.ascontiguousarray(prompts[0], np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        rec = DispatchRequest(host_pcm=vp(pcm), host_off=vp(offs), W=1, prompt_ids=vp(pr), prompt_len=len(pr), max_new=4, seq_ids=vp(i), seq_off=vp(o), bias=vp(b), n_seq=1)
        rc = rep.lib.sonic_dispatch_submit(rep.h, C.byref(rec), C.byref(tk))
        assert rc == 1 and b"request_bias" in rep.lib.sonic_last_error(None)
        disp.close()
        for s in slots:
            s.close()
        # the option: memory from sonic_memory_info, refused while rows are running, copied by slots, a splice between differing handles refused either way
        off.stage_pcm(segs[:1]); off.prefill(prompts[:1], [8])
        with pytest.raises(SonicError, match="running"):
            off.set_option("request_bias", 1)
        off.decode_step(100)
        off.set_option("request_bias", 1)
        a1 = off.memory_info()[0]
        print(f"request_bias: sonic_memory_info grows by {a1 - a0} bytes (history {64 * 1024 * 4}, tables {(64 + 64 * 256 * 10) * 4})")
        assert a1 - a0 == 64 * 1024 * 4 + (64 + 64 * 256 * 10) * 4
        V = spec.TINY.vocab
        for bad in ([[[V], 1.0]], [[[1] * 9, 1.0]]):
            with pytest.raises((SonicError, ValueError)):
                off.set_request_bias([RequestBias(bad)])
        with pytest.raises(SonicError, match="sonic_set_request_bias"):       # the library's own cap, behind the Python one
            big = RequestBias([[[1 + k], 1.0] for k in range(256)]); big.entries.append(((300,), np.float32(1.0)))
            off.set_request_bias([big])
        off.set_request_bias([t])                                              # tables for one request, a batch of two: refused, and consumed
        with pytest.raises(SonicError, match="requests"):
            off.transcribe_batch(segs, prompts, [4, 4])
        ids, _ = off.transcribe_batch(segs, prompts, [n_new, n_new])
        for si in range(2):
            assert np.array_equal(ids[si], g[f"s{si}_new_ids"][:len(ids[si])])
        # two consecutive prefills on one handle, the second without tables: nothing leaks
        ban = [RequestBias(bad_words_ids=[[int(g[f"s{si}_new_ids"][0])]]) for si in range(2)]
        a, _ = off.transcribe_batch(segs, prompts, [n_new, n_new], request_bias=ban)
        b2, _ = off.transcribe_batch(segs, prompts, [n_new, n_new])
        for si in range(2):
            assert int(a[si][0]) != int(g[f"s{si}_new_ids"][0]) and np.array_equal(b2[si], g[f"s{si}_new_ids"][:len(b2[si])])
        # a batch with tables that fails in STAGING (more windows than rows) never reaches its prefill: its tables are dropped all the same, and the next batch of
        # the same R, given none, emits the unbiased ids - through the one call ...
        five = [segs[0]] * 5
        with pytest.raises(SonicError):
            off.transcribe_batch(five, prompts, [n_new, n_new], req_win=[0, 3, 5], request_bias=ban)
        c2, _ = off.transcribe_batch(segs, prompts, [n_new, n_new])
        # ... and through the stage entry points: tables set, the prefill refused for its arguments, then a prefill without tables
        off.stage_pcm(segs)
        off.set_request_bias(ban)
        with pytest.raises(SonicError):
            off.prefill(prompts, [n_new, 0])
        off.stage_pcm(segs); off.prefill(prompts, [n_new, n_new]); off.decode_step(100)
        d2 = off.fetch_tokens(2, n_new)
        for si in range(2):
            assert len(c2[si]) and np.array_equal(c2[si], g[f"s{si}_new_ids"][:len(c2[si])])
            assert len(d2[si]) and np.array_equal(d2[si], g[f"s{si}_new_ids"][:len(d2[si])])
        pre = off.slot()
        assert pre.request_bias
        # a splice between handles whose options differ is refused, the message naming the option: the source without it ...
        pre.set_option("request_bias", 0)
        off.service_begin()
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [4])
        with pytest.raises(SonicError, match="request_bias"):
            off.splice_rows(pre, [0], [0])
        with pytest.raises(SonicError, match="continuously"):                  # (and the option itself is refused on a handle that decodes continuously)
            off.set_option("request_bias", 0)
        off.service_end()
        pre.decode_step(100)
        # ... and the other way round: the destination without it
        pre.set_option("request_bias", 1)
        off.set_option("request_bias", 0)
        off.service_begin()
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [4], request_bias=[t])
        with pytest.raises(SonicError, match="request_bias"):
            off.splice_rows(pre, [0], [0])
        off.service_end()
        pre.decode_step(100)
        pre.close()
    finally:
        off.close()


def test_bulk_refuses():
    from sonicscribe_amd.dispatch import Dispatcher
    e = make(max_batch=32)                               # (a pipeline block holds 32 rows)
    try:
        slots = [e.slot(), e.slot()]
        bulk = Dispatcher([e], slots=[slots], bulk=True, decoders=1)
        with pytest.raises(ValueError, match="bulk"):
            bulk.submit([synth.synth_pcm(1, 48000)], prompt_for(spec.TINY, 48000), 4, bias=RequestBias([[[5], 1.0]]))
        bulk.close()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 5. live HF
def test_live_hf_generate_with_sequence_bias_vs_fp32_engine_through_checkpoint(tmp_path):
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    from tests import hf_helpers as G
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.engine import MODE_F32
    d = spec.TINY
    n_new = 24
    model, _ = G.build_tiny(torch.float32)
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    pcm = synth.synth_pcm(10, 80000)
    feats, mask = G.mel_case(G.feature_extractor(), pcm)
    ids = G.PROMPT_PREFIX + [d.audio_token_id] * spec.audio_token_count(int(mask.sum())) + G.PROMPT_SUFFIX
    input_ids = torch.tensor([ids], dtype=torch.long)
    kw = dict(input_ids=input_ids, input_features=torch.from_numpy(feats)[None], input_features_mask=torch.from_numpy(mask)[None].long(),
              attention_mask=torch.ones_like(input_ids), max_new_tokens=n_new, do_sample=False, return_dict_in_generate=True, output_scores=True)
    with torch.no_grad():
        base = model.generate(**kw).sequences[0, len(ids):].tolist()
    # chosen on the CPU: unbiased, HF emits 304 at every step; with these entries 304, 205 (the first sequence binds at step 1), 206 (the second, step 2), then the bad
    # word (206, 304) turns step 3 away from 304; every step's top-1 / top-2 margin of HF's processed scores is > 0.2 on this input
    sb = [[[base[0], 205], 30.0], [[205, 206], 30.0], [[207], 0.5]]
    bw = [[206, base[0]], [206, 208]]
    with torch.no_grad():
        gen = model.generate(**kw, sequence_bias=sb, bad_words_ids=bw)
    ref_ids = gen.sequences[0, len(ids):].numpy().astype(np.int32)
    scores = torch.stack([s[0] for s in gen.scores]).numpy()
    m = ASRModel(str(tmp_path), max_batch=2, max_ctx=1024, slots=1, continuous=False, _allow_synthetic_prompt=True, _engine_mode=MODE_F32, request_bias=True)
    try:
        table = m._request_bias(None, sb, bw)
        got, _ = m.model.transcribe_batch([pcm], [ids], [n_new], request_bias=[table])
        srt = np.sort(scores, axis=1)
        margin = srt[:, -1] - srt[:, -2]
        clear = len(margin) if (margin > 1e-3).all() else int(np.argmin(margin > 1e-3))
        print(f"live HF with sequence_bias: {len(ref_ids)} steps, {clear} with margin > 1e-3; HF {ref_ids.tolist()} (unbiased {base})")
        assert clear == len(ref_ids) and ref_ids[:3].tolist() == [base[0], 205, 206] and int(ref_ids[3]) != base[0]
        assert np.array_equal(got[0], ref_ids), (got[0].tolist(), ref_ids.tolist())
        assert m.prompt.decode(got[0]) == m.prompt.decode(ref_ids)                                # the transcripts are equal
    finally:
        m.close()
