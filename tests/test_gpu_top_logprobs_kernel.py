"""The TOPK instantiations of the greedy kernel (csrc/greedy.hip, option top_logprobs), through the four hooks that return log-probabilities, on a
handle with the option set: all six families that have LP - lp, guard_lp, bias_lp, sample, sample_guard, sample_bias.

Contract: with s the fully processed scores (bias, penalty, bans), the K alternatives are the first K ids of the order (s descending, id ascending) among the
ids with s > -inf, each with log_softmax(s)[id] formed from the emitted token's maximum and sum; places beyond the finite scores hold (-1, -inf).  Forcing and
sampling change the emitted token, never the alternatives.

Reference: NumPy forms the processed scores (reqbias.RequestBias.apply, genconfig.GenerationGuards.apply - what the families' own tests check the kernel
against) and sorts stably by -s, so equal values keep ascending ids.  Ids must be equal; every log-probability lies within DESIGN.md 6.3's derived bound
(check_lp of test_gpu_request_bias.py) of float64 log_softmax.  Everything else is bit for bit.

Shapes: 4 rows, K = 8, V = 8 (two f32x4 groups: fewer ids than threads), 16388 (one group in the last, partial trip of the 4 x 4096 loop), 59264 (the production
vocabulary), 1 and 2 slabs.  Rows are uniform(-4, 4) cut to bf16 precision: about a thousand distinct values, so at 59264 the top 8 hold ties."""
import numpy as np
import pytest

from gpu_common import SEED, check_lp, make_engine, same_bits, slabs
from sonicscribe_amd.genconfig import GenerationGuards
from sonicscribe_amd.reqbias import RequestBias
from test_gpu_request_bias import _histories  # noqa: E402
from test_gpu_sampling_kernel import bf16_exact  # noqa: E402

pytestmark = pytest.mark.gpu
B = 4
K = 8
NEG = np.float32("-inf")
SHAPES = pytest.mark.parametrize("V,ks", [(V, ks) for V in (8, 16388, 59264) for ks in (1, 2)])
FAMILIES = ("lp", "guard_lp", "bias_lp", "sample", "sample_guard", "sample_bias")      # (GUARD, BIAS, SAMPLE) below
FLAGS = {"lp": (0, 0, 0), "guard_lp": (1, 0, 0), "bias_lp": (1, 1, 0), "sample": (0, 0, 1), "sample_guard": (1, 0, 1), "sample_bias": (1, 1, 1)}
GUARDS = GenerationGuards(repetition_penalty=1.3, no_repeat_ngram_size=2)


@pytest.fixture(scope="module")
def eng():
    """one bf16 handle; the option is switched between launches (the hooks leave no work in hand)"""
    e = make_engine(max_batch=B)
    e.set_option("token_logprobs", 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases():
    """(rows, slabs, hist, hlen) per shape, computed once and left unchanged"""
    memo = {}

    def get(V, ks):
        if (V, ks) not in memo:
            rng = np.random.default_rng(SEED + V)
            rows = [bf16_exact(rng.uniform(-4.0, 4.0, V)) for _ in range(B)]
            hist, hlen = _histories(V, rng)
            memo[V, ks] = (rows, slabs(rows, ks), hist, hlen)
        return memo[V, ks]
    return get


def tables_for(rows):
    """a boost on every row's lowest id (it becomes alternative 0) and a bad word on its second-highest (it leaves the list)"""
    return [RequestBias([[[int(np.argmin(r))], 100.0]], [[int(np.argsort(-r, kind="stable")[1])]], []) for r in rows]


def processed(family, rows, hist, hlen, tables, suppress):
    guard, bias, _ = FLAGS[family]
    out = []
    for b, r in enumerate(rows):
        h = hist[b, :hlen[b]]
        s = tables[b].apply(r, h) if bias else np.array(r, np.float32)
        if guard:
            s = GenerationGuards(GUARDS.repetition_penalty, GUARDS.no_repeat_ngram_size, list(suppress)).apply(s, h)
        out.append(np.asarray(s, np.float32))
    return out


def launch(eng, family, k, s, hist, hlen, tables, suppress=(), temperature=None, force_ids=None):
    """one launch of `family` with option top_logprobs = k -> (tokens, raw logits, lp [B], top_lp [B, k], top_ids [B, k])"""
    eng.set_option("top_logprobs", k)
    guard, bias, sample = FLAGS[family]
    g = dict(repetition_penalty=GUARDS.repetition_penalty, no_repeat_ngram_size=GUARDS.no_repeat_ngram_size, suppress_tokens=suppress)
    if sample:
        t = [0.0] * B if temperature is None else temperature
        kw = dict(hist=hist, hist_len=hlen, tables=tables if bias else None, **g) if guard else {}
        tok, raw, lp, _ = eng.test_greedy_sample(s, B, t, list(range(B)), [0] * B, force_ids=force_ids, want_noise=False, **kw)
    elif bias:
        tok, raw, lp = eng.test_greedy_bias(s, B, hist, hlen, tables, force_ids=force_ids, want_lp=True, **g)
    elif guard:
        tok, raw, lp = eng.test_greedy_guard(s, B, hist, hlen, force_ids=force_ids, want_lp=True, **g)
    else:
        tok, raw, lp = eng.test_greedy_lp(s, B, force_ids=force_ids)
    if k == 0:
        return tok, raw, lp, np.zeros((B, 0), np.float32), np.zeros((B, 0), np.int32)
    return (tok, raw) + tuple(lp)


def reference(s, k):
    """the first k ids of (s descending, id ascending) among the finite scores, -1 beyond them"""
    order = np.argsort(-np.asarray(s, np.float64), kind="stable")[:k]
    ids = np.array([int(i) if s[i] > NEG else -1 for i in order] + [-1] * (k - len(order)), np.int32)
    return ids


def check_alternatives(tag, s, top_lp, top_ids, k=K):
    want = reference(s, k)
    assert top_ids.dtype == np.int32 and top_ids.tolist() == want.tolist(), (tag, top_ids.tolist(), want.tolist())
    for j in range(k):
        if want[j] < 0:
            assert np.isneginf(top_lp[j]), (tag, j, top_lp[j])
        else:
            check_lp(tag + (j,), top_lp[j], s, want[j])
    live = top_lp[want >= 0]
    assert np.all(live[:-1] >= live[1:]) or len(live) < 2, (tag, "descending")


@SHAPES
@pytest.mark.parametrize("family", FAMILIES)
def test_families_against_numpy(eng, cases, family, V, ks):
    """every family at every shape: ids equal NumPy's, log-probabilities within the bound; tokens, raw dump and lp are the K = 0 launch's bits; on these
    greedy, unforced rows alternative 0 is (tok, lp) bit for bit.  At V = 59264 the top 8 hold equal values: the lowest-id rule decides"""
    rows, s, hist, hlen = cases(V, ks)
    tables = tables_for(rows) if V > 8 else [RequestBias([[[7], 0.5]]) for _ in rows]
    sup = sorted({int(np.argmax(r)) for r in rows}) if FLAGS[family][0] else ()
    tok0, raw0, lp0, _, _ = launch(eng, family, 0, s, hist, hlen, tables, sup)
    tok, raw, lp, top_lp, top_ids = launch(eng, family, K, s, hist, hlen, tables, sup)
    assert np.array_equal(tok, tok0) and same_bits(raw, raw0) and same_bits(lp, lp0), (family, V, ks)
    proc = processed(family, rows, hist, hlen, tables, sup)
    ties = 0
    for b in range(B):
        check_alternatives((family, V, ks, b), proc[b], top_lp[b], top_ids[b])
        assert int(top_ids[b, 0]) == int(tok[b]) and same_bits(top_lp[b, 0], lp[b]), (family, V, ks, b, "alternative 0 is the emitted token")
        v = proc[b][top_ids[b][top_ids[b] >= 0]]
        ties += int(np.sum(v[:-1] == v[1:]))
    if V == 59264:
        assert ties >= 1, "bf16-exact rows of 59264 values: the top 8 were expected to hold equal values"


def placed(V, where, rng):
    """rows whose eight largest values sit at chosen ids: thread t owns ids 4t .. 4t + 3 of every 4096-id stride"""
    spots = {"one_thread": [0, 1, 2, 3, 4096, 4097, 8192, 16384],                       # thread 0's ids, over all four strides and the partial trip
             "eight_lanes": [4 * lane + 1 for lane in (0, 5, 9, 17, 30, 41, 50, 63)],      # eight lanes of wave 0
             "eight_waves": [256 * w + 4 * (w + 1) for w in (0, 2, 3, 5, 8, 11, 13, 15)],  # one lane in each of eight waves
             "last_trip": [16384, 16385, 16386, 16387, 16386, 16385, 16384, 16387]}[where]
    rows = []
    for b in range(B):
        r = bf16_exact(rng.uniform(-4.0, 3.0, V))
        ids = spots if where != "last_trip" else spots[:4]
        vals = bf16_exact(4.0 + 0.25 * rng.permutation(len(ids)))                         # distinct, above everything else, in no id order
        if b == 1:
            vals[:] = vals[0]                                                             # all equal: ids ascending
        r[ids] = vals
        rows.append(r)
    return rows


@pytest.mark.parametrize("where", ["one_thread", "eight_lanes", "eight_waves", "last_trip"])
def test_placed_maxima(eng, where):
    """V = 16388: the eight largest values in one thread's list, in eight lanes of one wave, in eight waves, in the last partial trip (four ids: the other
    four alternatives come from the rest) - what each stage of the merge has to get right on its own"""
    V = 16388
    rng = np.random.default_rng(SEED + 99)
    rows = placed(V, where, rng)
    hist, hlen = _histories(V, rng)
    for ks in (1, 2):
        tok, raw, lp, top_lp, top_ids = launch(eng, "lp", K, slabs(rows, ks), hist, hlen, None)
        for b in range(B):
            check_alternatives((where, ks, b), rows[b], top_lp[b], top_ids[b])
            assert int(top_ids[b, 0]) == int(tok[b]) and same_bits(top_lp[b, 0], lp[b])


def test_prefixes(eng, cases):
    """K = 1, 3 and 8 on the same slabs: each is a prefix of the next, bit for bit"""
    rows, s, hist, hlen = cases(16388, 2)
    got = {k: launch(eng, "guard_lp", k, s, hist, hlen, None) for k in (1, 3, 8)}
    for k in (1, 3):
        assert got[k][3].shape == (B, k) and np.array_equal(got[k][4], got[8][4][:, :k]) and same_bits(got[k][3], got[8][3][:, :k]), k
        assert same_bits(got[k][2], got[8][2]) and np.array_equal(got[k][0], got[8][0])


def test_few_finite_scores(eng):
    """guard family, V = 8: all but three ids suppressed - three entries, then five x (-1, -inf); a row whose every id is banned - eight x (-1, -inf)"""
    rng = np.random.default_rng(SEED + 8)
    rows = [bf16_exact(rng.uniform(-4.0, 4.0, 8)) for _ in range(B)]
    hist, hlen = np.zeros((B, 2), np.int32), np.zeros(B, np.int32)
    eng.set_option("top_logprobs", K)
    tok, raw, lp = eng.test_greedy_guard(slabs(rows, 1), B, hist, hlen, suppress_tokens=[0, 2, 3, 5, 7], want_lp=True)
    for b in range(B):
        s = np.array(rows[b], np.float32)
        s[[0, 2, 3, 5, 7]] = NEG
        check_alternatives(("three", b), s, lp.top_logprobs[b], lp.top_ids[b])
        assert lp.top_ids[b, 3:].tolist() == [-1] * 5 and np.all(np.isneginf(lp.top_logprobs[b, 3:])) and sorted(lp.top_ids[b, :3].tolist()) == [1, 4, 6]
    tok, raw, lp = eng.test_greedy_guard(slabs(rows, 1), B, hist, hlen, suppress_tokens=list(range(8)), want_lp=True)
    assert lp.top_ids.tolist() == [[-1] * K] * B and np.all(np.isneginf(lp.top_logprobs)) and tok.tolist() == [0] * B


def test_forcing_and_sampling_leave_the_alternatives(eng, cases):
    """a forced id outside the top 8, and rows sampling at t = 1: the alternatives are the greedy launch's, bit for bit; the emitted token's lp is the K = 0
    launch's; an emitted token that is among the alternatives carries lp's bits"""
    rows, s, hist, hlen = cases(16388, 1)
    _, _, _, alt_lp, alt_ids = launch(eng, "lp", K, s, hist, hlen, None)
    force = np.array([int(np.argsort(-r, kind="stable")[100 + b]) for b, r in enumerate(rows)], np.int32)
    tok0, _, lp0, _, _ = launch(eng, "lp", 0, s, hist, hlen, None, force_ids=force)
    tok, _, lp, top_lp, top_ids = launch(eng, "lp", K, s, hist, hlen, None, force_ids=force)
    assert tok.tolist() == force.tolist() == tok0.tolist() and same_bits(lp, lp0)
    assert np.array_equal(top_ids, alt_ids) and same_bits(top_lp, alt_lp) and not any(int(force[b]) in top_ids[b] for b in range(B))
    _, _, _, g_lp, g_ids = launch(eng, "sample", K, s, hist, hlen, None)                 # t = 0: greedy rows of the sampling family
    assert np.array_equal(g_ids, alt_ids) and same_bits(g_lp, alt_lp)
    t = [1.0] * B
    tok0, _, lp0, _, _ = launch(eng, "sample", 0, s, hist, hlen, None, temperature=t)
    tok, _, lp, top_lp, top_ids = launch(eng, "sample", K, s, hist, hlen, None, temperature=t)
    assert np.array_equal(tok, tok0) and same_bits(lp, lp0) and any(int(tok[b]) != int(alt_ids[b, 0]) for b in range(B)), "t = 1 draws away from the maximum"
    assert np.array_equal(top_ids, alt_ids) and same_bits(top_lp, alt_lp)
    for b in range(B):
        hit = np.nonzero(top_ids[b] == tok[b])[0]
        if len(hit):
            assert same_bits(top_lp[b, hit[0]], lp[b]), (b, "an emitted token among the alternatives carries out_lp's bits")
