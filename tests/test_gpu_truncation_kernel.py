"""top_k / top_p / min_p in the greedy kernel (greedy_kernel<T, true, GUARD, BIAS, true, TOPK, GRAMMAR, true>; truncsel.h), through
sonic_test_greedy_sample with a truncation armed on the handle (sonic_load_tensor "truncation.hook"), in the handle's own type: bf16, fp16 and the fp32 kind.  The
reference is sonicscribe_amd/sampling.py (truncation_order / truncation_counts) over the processed scores `GenerationGuards.apply(RequestBias.apply(raw, history),
history)`, `raw` being the logits the kernel dumps (rounded to the handle's type: any fp32 input will do).

Every row is held to five rules (check_row):
  1. structure, bit for bit   the record (bits of the last kept y, its id, n) names position n - 1 of the (y descending, id ascending) order of the numpy y
  2. top_k / min_p, exact     a row without top_p has n = the reference's n, tie rows included
  3. top_p                    n_ref(p - EPS_MASS) <= n <= n_ref(p + EPS_MASS), no row excluded; the two ends agree on at least 90 % of the rows of a test
  4. token, bit for bit       the emitted token is the first maximum of float32(y + noise_out) over the first n ids of the order
  5. log-probability          out_lp is within the existing lp_bound of log_softmax(s)[tok] over the untruncated scores
Logit scales: Zipf-like rows s = -1.5 ln(rank) (+ jitter), for which the id at the 0.9 boundary carries about 1e-3 of the mass - forty times EPS_MASS - so the
reference alone is unambiguous on almost every row; and rows with a few dominant ids whose cut is unambiguous by a wide margin."""
import numpy as np
import pytest

from gpu_common import lp_bound, make_engine, ref_logprob, same_bits, slabs
from sonicscribe_amd import sampling
from sonicscribe_amd.genconfig import GenerationGuards
from sonicscribe_amd.grammar import Grammar
from sonicscribe_amd.reqbias import RequestBias

pytestmark = pytest.mark.gpu
NEG = float("-inf")
MODES = pytest.mark.parametrize("mode", [0, 2, 3], ids=["bf16", "f16", "f32"])
OFF = (0, 1.0, 0.0)


def check_lp(tag, lp, processed, tok):
    ref = ref_logprob(processed, tok)
    ratio = abs(float(lp) - ref) / lp_bound(len(processed), ref)
    assert np.isfinite(lp) and ratio <= 1.0, (tag, float(lp), ref, ratio)


@pytest.fixture(scope="module")
def engines():
    es = {}

    def get(mode):
        if mode not in es:
            es[mode] = make_engine(mode=mode)                              # the hook takes everything as arguments: no option plays a part in it
        return es[mode]
    yield get
    for e in es.values():
        e.close()


def zipf_row(V, rng, a=1.5, jitter=0.02):
    s = (-a * np.log(np.arange(1, V + 1)) + rng.uniform(-jitter, jitter, V)).astype(np.float32)
    return s[rng.permutation(V)]


def dominant_row(V, rng, vals):
    """a few dominant ids at scattered places over a floor 15 below them"""
    s = rng.uniform(-6.0, -5.0, V).astype(np.float32)
    at = [7 % V, V // 2, V - 3, V // 3, 1][: len(vals)]
    s[at] = vals
    return s


def histories(V, B, rng):
    hlen = np.array([1, 40, 17, 5][:B], np.int32)
    pool = [5, 6, 7, 9, 11, V - 4, V - 5]
    hist = np.zeros((B, 40), np.int32)
    for b in range(B):
        hist[b, :hlen[b]] = rng.choice(pool, hlen[b])
    return hist, hlen


def check_row(tag, s, t, trunc, tok, lp, noise, rec, stats):
    """the five rules on one row.  s: the processed scores; rec: (y bits, id, n) of the row"""
    V = len(s)
    k, p, m = trunc
    y = sampling.quotient(s, t)
    order = sampling.truncation_order(y)
    ybits, cid, n = int(rec[0]), int(rec[1]), int(rec[2])
    n_k, n_p, n_m = sampling.truncation_counts(y, k, p, m)
    if not np.isfinite(y.max()) or (k == 0 and p == 1.0 and m == 0.0):
        assert (ybits, cid, n) == (0, -1, V), (tag, ybits, cid, n)      # the branch around the select
    else:
        assert 1 <= n <= V, (tag, n)
        assert int(order[n - 1]) == cid and int(y[cid:cid + 1].view(np.uint32)[0]) == ybits, (tag, "structure", n, cid, int(order[n - 1]), hex(ybits))      # rule 1
        if p == 1.0:
            assert n == min(n_k, n_m), (tag, "top_k / min_p", n, n_k, n_m)                                                                                   # rule 2
        else:
            lo = min(sampling.truncation_counts(y, k, p, m, -sampling.EPS_MASS))
            hi = min(sampling.truncation_counts(y, k, min(p, 1.0), m, sampling.EPS_MASS))
            stats.append(lo == hi)
            print(f"  {tag}: n {n} in [{lo}, {hi}] (n_k {n_k} n_p {n_p} n_m {n_m})")
            assert lo <= n <= hi, (tag, "top_p", n, lo, hi)                                                                                                  # rule 3
    kept = np.sort(order[:n])
    yy = (y[kept] + np.asarray(noise, np.float32)[kept]).astype(np.float32)
    want = int(kept[int(np.argmax(yy))]) if np.isfinite(y.max()) else 0
    assert int(tok) == want, (tag, "token", int(tok), want, n)                                                                                               # rule 4
    if np.isfinite(np.asarray(s, np.float32).max()):
        check_lp(tag, lp, s, tok)                                                                                                                            # rule 5


def chain(raw, hist, table, guards):
    s = table.apply(raw, hist) if table is not None else np.array(raw, np.float32)
    return guards.apply(s, hist)


def _family(V, family, rng):
    hist, hlen = histories(V, 4, rng)
    guards, tables = {}, None
    if family in ("guard", "bias"):
        guards = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[V - 3])
    if family == "bias":
        h1 = [int(t) for t in hist[1, :40]]
        tables = [RequestBias([[[3], 1.5], [[V - 1], 0.75]]), RequestBias([[[h1[-2], h1[-1], V // 3], 2.0]], bad_words_ids=[[4]]), None, RequestBias([[[int(hist[3, 4]), 9], 1.25]])]
    return hist, hlen, guards, tables


def _launch(eng, family, s, B, t, seeds, steps, trunc, hist, hlen, guards, tables):
    kw = {} if family == "plain" else dict(hist=hist[:B], hist_len=hlen[:B], tables=tables[:B] if family == "bias" else None, **guards)
    if trunc is None:
        return eng.test_greedy_sample(s, B, t, seeds, steps, **kw) + (None,)
    return eng.test_greedy_truncation(s, B, t, seeds, steps, trunc, **kw)


# ------------------------------------------------------------------------------------------ 1. the five rules, every family, every size
@MODES
@pytest.mark.parametrize("family", ["plain", "guard", "bias"])
@pytest.mark.parametrize("V", [20, 4100, 16388, 59264])
def test_rules(engines, V, family, mode):
    """V = 20 (fewer ids than k = 50), 4100 (one partial trip of the 16 384-id loop), 16388 (one group left in the second trip), 59264.  Launch A: Zipf rows under
    top_k, top_p, min_p alone and all three; launch B: the same rows under other values, top_p so small that one id stays among them"""
    eng = engines(mode)
    rng = np.random.default_rng(100 + V)
    hist, hlen, guards, tables = _family(V, family, rng)
    g = GenerationGuards(**guards)
    rows = [zipf_row(V, rng) for _ in range(4)]
    t, seeds, steps = [0.7, 1.0, 1.3, 0.9], [3, 0x123456789ABCDEF0, 17, 1], [0, 7, 1000, 2]
    sets = ([(50, 1.0, 0.0), (0, 0.9, 0.0), (0, 1.0, 0.05), (50, 0.9, 0.05)], [(5, 0.95, 0.0), (0, 0.5, 0.001), (3, 1.0, 0.5), (0, 1e-6, 0.0)])
    stats = []
    for ks in (1, 2):
        for trunc in sets:
            tok, raw, lp, noise, rec = _launch(eng, family, slabs(rows, ks), 4, t, seeds, steps, trunc, hist, hlen, guards, tables)
            for b in range(4):
                s = raw[b] if family == "plain" else chain(raw[b], hist[b, :hlen[b]], tables[b] if tables else None, g)
                check_row((V, family, mode, ks, trunc[b]), s, t[b], trunc[b], tok[b], lp[b], noise[b], (rec[0][b], rec[1][b], rec[2][b]), stats)
            if trunc[3][1] == 1e-6:
                assert int(rec[2][3]) == 1                      # one id stays: the first maximum of y
    assert len(stats) >= 10 and np.mean(stats) >= 0.9, (len(stats), float(np.mean(stats)))


# ------------------------------------------------------------------------------------------ 2. ties built on purpose, dominant ids, rows of -inf
@MODES
@pytest.mark.parametrize("V", [20, 16388])
def test_ties_and_dominant_rows(engines, V, mode):
    eng = engines(mode)
    rng = np.random.default_rng(7)
    r0 = dominant_row(V, rng, [3.0, 2.0, 2.0, 2.0, 1.0])      # top_k = 2: the 2nd value is held by three ids, all kept (HF's `scores < kth`): n = 4
    r1 = dominant_row(V, rng, [3.0, 3.0, 1.0])                 # min_p = 1: the threshold is the maximum, held by two ids: n = 2
    r2 = dominant_row(V, rng, [10.0, 8.0, 8.0, 8.0])           # top_p = 0.85: mass in front of the ties' three ids 0.711, 0.807, 0.903 of the four: the two lower ids stay
    r3 = dominant_row(V, rng, [10.0, 9.0, 8.0])                # top_p = 0.9: 0.665, 0.910: two ids stay, by a wide margin
    trunc = [(2, 1.0, 0.0), (0, 1.0, 1.0), (0, 0.85, 0.0), (0, 0.9, 0.0)]
    want_n = [4, 2, 3, 2]
    t, seeds, steps = [1.0] * 4, [5, 6, 7, 8], [0, 1, 2, 3]
    stats = []
    for ks in (1, 2):
        tok, raw, lp, noise, rec = eng.test_greedy_truncation(slabs([r0, r1, r2, r3], ks), 4, t, seeds, steps, trunc)
        for b in range(4):
            check_row((V, mode, ks, b), raw[b], t[b], trunc[b], tok[b], lp[b], noise[b], (rec[0][b], rec[1][b], rec[2][b]), stats)
            assert int(rec[2][b]) == want_n[b], (b, int(rec[2][b]))
        assert int(rec[1][2]) == V // 2                        # the ties at the boundary go by the lower id: V // 3 and V // 2 stay, V - 3 does not
    assert all(stats)
    # a row of -inf only, and a row whose finite scores are fewer than k
    a = np.full(V, NEG, np.float32)
    c = np.full(V, NEG, np.float32)
    c[[2, V // 2, V - 1]] = [1.0, 2.0, 0.5]
    trunc = [(5, 0.9, 0.1), (5, 1.0, 0.0), (0, 0.9, 0.0), (2, 0.9, 0.5)]
    tok, raw, lp, noise, rec = eng.test_greedy_truncation(slabs([a, c, c, c], 1), 4, t, seeds, steps, trunc)
    for b in range(4):
        check_row((V, mode, "inf", b), raw[b], t[b], trunc[b], tok[b], lp[b], noise[b], (rec[0][b], rec[1][b], rec[2][b]), stats)
    assert int(tok[0]) == 0 and int(rec[2][1]) == V             # k >= the number of finite scores: nothing is removed
    assert all(int(x) in (2, V // 2, V - 1) for x in tok[1:])


# ------------------------------------------------------------------------------------------ 3. a grammar row
@MODES
def test_grammar_row(engines, mode):
    eng = engines(mode)
    V = 16388
    rng = np.random.default_rng(9)
    allowed = sorted(int(x) for x in rng.choice(np.arange(10, V - 10), 200, replace=False))
    gr = Grammar.from_token_sequences([[a] for a in allowed], [V - 1], vocab=V, audio_token_id=V - 2)
    rows = [zipf_row(V, rng) for _ in range(2)]
    hist, hlen = histories(V, 2, rng)
    t, seeds, steps = [0.8, 1.0], [11, 12], [0, 4]
    trunc = [(20, 0.9, 0.01), (0, 0.8, 0.0)]
    eng.arm_truncation_hook(sampling.pack_truncation(trunc))
    tok, raw, lp, noise, state = eng.test_greedy_grammar(slabs(rows, 1), 2, gr, [0, -1], eos_ids=[V - 1], hist=hist, hist_len=hlen, samp=(t, seeds, steps))
    rec = eng.read_truncation_hook(2)
    stats = []
    for b in range(2):
        s = GenerationGuards().apply(raw[b], hist[b, :hlen[b]])
        if b == 0:
            s = gr.apply(s, 0, [V - 1])
        check_row((mode, "grammar", b), s, t[b], trunc[b], tok[b], lp[b], noise[b], (rec[0][b], rec[1][b], rec[2][b]), stats)
    assert int(tok[0]) in allowed and int(rec[2][0]) <= 20


# ------------------------------------------------------------------------------------------ 4. across rows
@MODES
@pytest.mark.parametrize("family", ["plain", "bias"])
def test_rows_off_and_row_independence(engines, family, mode):
    """t = 0 rows and rows with all three parameters off carry the bits of the parent SAMPLE launch; the same launch twice gives the same records and tokens; a row
    gives the same record and token as row 0 of one batch and as row 3 of another"""
    eng = engines(mode)
    V = 16388
    rng = np.random.default_rng(21)
    hist, hlen, guards, tables = _family(V, family, rng)
    rows = [zipf_row(V, rng) for _ in range(4)]
    t, seeds, steps = [0.0, 1.0, 0.8, 0.6], [5, 6, 7, 8], [0, 3, 9, 1]
    trunc = [(5, 0.9, 0.1), OFF, (40, 0.9, 0.02), OFF]
    for ks in (1, 2):
        s = slabs(rows, ks)
        tok0, _, lp0, noise0, _ = _launch(eng, family, s, 4, t, seeds, steps, None, hist, hlen, guards, tables)
        tok, _, lp, noise, rec = _launch(eng, family, s, 4, t, seeds, steps, trunc, hist, hlen, guards, tables)
        tok2, _, lp2, noise2, rec2 = _launch(eng, family, s, 4, t, seeds, steps, trunc, hist, hlen, guards, tables)
        for b in (0, 1, 3):
            assert int(tok[b]) == int(tok0[b]) and same_bits(lp[b], lp0[b]), (family, ks, b)
            assert (int(rec[0][b]), int(rec[1][b]), int(rec[2][b])) == (0, -1, V)
        assert same_bits(noise, noise0) and not noise[0].any()
        assert np.array_equal(tok, tok2) and same_bits(lp, lp2) and all(np.array_equal(rec[i], rec2[i]) for i in range(3))
        assert 1 <= int(rec[2][2]) <= 40
    if family == "plain":
        # row 2 of the batch above as row 0 of one batch and as row 3 of another
        ta, _, la, _, ra = eng.test_greedy_truncation(slabs([rows[2]], 1), 1, [t[2]], [seeds[2]], [steps[2]], [trunc[2]])
        other = [rows[0], rows[1], rows[3], rows[2]]
        tb, _, lb, _, rb = eng.test_greedy_truncation(slabs(other, 1), 4, [0.5, 0.0, 1.0, t[2]], [1, 2, 3, seeds[2]], [4, 5, 6, steps[2]], [(3, 0.5, 0.0), OFF, (0, 0.7, 0.3), trunc[2]])
        for tt, ll, rr, b in ((ta, la, ra, 0), (tb, lb, rb, 3)):
            assert int(tt[b]) == int(tok[2]) and same_bits(ll[b], lp[2]) and all(int(rr[i][b]) == int(rec[i][2]) for i in range(3)), b


# ------------------------------------------------------------------------------------------ 5. the TOPK twins
@MODES
@pytest.mark.parametrize("family", ["plain", "bias"])
def test_with_top_logprobs(family, mode):
    """option top_logprobs = 8 on the handle: the hooks launch the TRUNC x TOPK instantiations.  The alternatives and out_lp carry the bits of the untruncated
    launch (the cut changes the draw, never the record), and the token obeys rule 4"""
    eng = make_engine(mode=mode, options=(("token_logprobs", 1), ("top_logprobs", 8)))
    try:
        V = 16388
        rng = np.random.default_rng(33)
        hist, hlen, guards, tables = _family(V, family, rng)
        g = GenerationGuards(**guards)
        rows = [zipf_row(V, rng) for _ in range(4)]
        t, seeds, steps = [0.7, 1.0, 0.0, 1.3], [3, 4, 5, 6], [0, 7, 2, 1]
        trunc = [(10, 1.0, 0.0), (0, 0.9, 0.0), (5, 0.5, 0.5), (40, 0.95, 0.01)]
        s = slabs(rows, 2)
        tok0, _, sc0, _, _ = _launch(eng, family, s, 4, t, seeds, steps, None, hist, hlen, guards, tables)
        tok, raw, sc, noise, rec = _launch(eng, family, s, 4, t, seeds, steps, trunc, hist, hlen, guards, tables)
        assert same_bits(sc.top_logprobs, sc0.top_logprobs) and np.array_equal(sc.top_ids, sc0.top_ids)
        stats = []
        for b in range(4):
            p = raw[b] if family == "plain" else chain(raw[b], hist[b, :hlen[b]], tables[b] if tables else None, g)
            check_row((family, mode, "topk", b), p, t[b] if t[b] > 0 else 1.0, trunc[b] if t[b] > 0 else OFF, tok[b], sc.lp[b], noise[b], (rec[0][b], rec[1][b], rec[2][b]), stats)
            if int(tok[b]) == int(tok0[b]):
                assert same_bits(sc.lp[b], sc0.lp[b])
            assert np.array_equal(sc.top_ids[b], np.argsort(-np.asarray(p, np.float64), kind="stable")[:8])      # the alternatives: the 8 best of the untruncated scores
        assert int(tok[2]) == int(tok0[2])                          # the t = 0 row
    finally:
        eng.close()


def test_refusals_by_name(engines):
    from sonicscribe_amd.engine import SonicError
    eng = engines(0)
    for bad, name in (((-1.0, 0.9, 0.0), "top_k"), ((2.5, 0.9, 0.0), "top_k"), ((0, 0.0, 0.0), "top_p"), ((0, 1.5, 0.0), "top_p"), ((0, float("nan"), 0.0), "top_p"),
                      ((0, 0.9, -0.1), "min_p"), ((0, 0.9, 1.5), "min_p"), ((0, 0.9, float("nan")), "min_p")):
        with pytest.raises(SonicError, match=name):
            eng.arm_truncation_hook(np.array([bad], np.float32))
