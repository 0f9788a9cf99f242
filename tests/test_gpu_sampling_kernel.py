"""Temperature sampling in the greedy kernel (greedy_kernel<T, true, GUARD, BIAS, true>), through sonic_test_greedy_sample, in the handle's own type:
bf16, fp16 and the fp32 kind.  The reference is sonicscribe_amd/sampling.py (the noise definition) over `GenerationGuards.apply(RequestBias.apply(raw, history),
history)` (the processed scores, held bit for bit against HF by the host tests).

Inputs are bf16-exact values of moderate size, so the rounding to the handle's type changes none of them: the existing hooks (which launch the bf16 kernels whatever
the handle) see the same scores as the sampling hook does."""
import numpy as np
import pytest

from gpu_common import lp_bound, make_engine, ref_logprob, same_bits, slabs
from sonicscribe_amd import sampling
from sonicscribe_amd.genconfig import GenerationGuards
from sonicscribe_amd.reqbias import RequestBias

pytestmark = pytest.mark.gpu
NEG = float("-inf")
MODES = pytest.mark.parametrize("mode", [0, 2, 3], ids=["bf16", "f16", "f32"])
SEEDS = (0, 1, 0x123456789ABCDEF0)
STEPS = (0, 7, 1000)


def check_lp(tag, lp, processed, tok):
    ref = ref_logprob(processed, tok)
    ratio = abs(float(lp) - ref) / lp_bound(len(processed), ref)
    print(f"  lp {tag}: kernel {float(lp):.7f} ref {ref:.7f} |d|/bound {ratio:.3f}")
    assert np.isfinite(lp) and ratio <= 1.0, (tag, float(lp), ref, ratio)


def bf16_exact(x):
    """fp32 values cut to bf16 precision, magnitudes in [2^-6, 4): exact in bf16, fp16 and fp32 alike"""
    x = np.asarray(x, np.float32)
    x = np.where(np.abs(x) < 2.0 ** -6, np.float32(2.0 ** -6), x).astype(np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def chain(raw, hist, table, guards):
    s = table.apply(raw, hist) if table is not None else np.array(raw, np.float32)
    return guards.apply(s, hist)


def select(s, t, noise):
    """the contract's selection in fp32 on the noise the kernel reports: first maximum of float32(s / t) + g"""
    with np.errstate(invalid="ignore"):
        y = (np.asarray(s, np.float32) / np.float32(t)).astype(np.float32) + np.asarray(noise, np.float32)
    assert y.dtype == np.float32
    return int(np.argmax(y)), y


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


def histories(V, B, rng):
    hlen = np.array([1, 40, 17, 5][:B], np.int32)
    pool = [5, 6, 7, 9, 77, V - 4, V - 5]
    hist = np.zeros((B, 40), np.int32)
    for b in range(B):
        hist[b, :hlen[b]] = rng.choice(pool, hlen[b])
    return hist, hlen


# ------------------------------------------------------------------------------------------ 1. the noise
@MODES
@pytest.mark.parametrize("V", [4, 16388, 59264])
def test_noise(engines, V, mode):
    """noise_out against gumbel_noise at every id: V = 4 (one group), 16388 (one group left in the second trip), 59264; seeds x steps as nine rows of one launch"""
    eng = engines(mode)
    pairs = [(sd, st) for sd in SEEDS for st in STEPS]
    B = len(pairs)
    rows = [np.zeros(V, np.float32) for _ in range(B)]
    tok, raw, lp, noise = eng.test_greedy_sample(slabs(rows, 1), B, [1.0] * B, [p[0] for p in pairs], [p[1] for p in pairs])
    worst = 0.0
    for b, (sd, st) in enumerate(pairs):
        g = sampling.gumbel_noise(sd, st, V)
        err = np.abs(noise[b].astype(np.float64) - g).max()
        worst = max(worst, err)
        assert err <= sampling.EPS_G, (V, hex(sd), st, err, int(np.argmax(np.abs(noise[b] - g))))
        # zero scores: the token is the first maximum of the noise itself
        assert int(tok[b]) == int(np.argmax(noise[b])), (V, b)
    print(f"noise V={V} mode={mode}: worst |g - g64| = {worst:.3e} (eps_g = {sampling.EPS_G:.3e})")


# ------------------------------------------------------------------------------------------ 2. the selection, bit for bit; 3. rows with t = 0
def _family_inputs(V, family, rng):
    B = 4
    rows = [bf16_exact(rng.uniform(-2.0, 2.0, V)) for _ in range(B)]
    hist, hlen = histories(V, B, rng)
    guards, tables = {}, None
    if family in ("guard", "bias"):
        guards = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[V - 3])
    if family == "bias":
        h1 = [int(t) for t in hist[1, :40]]
        tables = [RequestBias([[[3], 1.5], [[V - 1], 0.75]]), RequestBias([[[h1[-2], h1[-1], V // 3], 2.0]], bad_words_ids=[[4]]), None,
                  RequestBias([[[int(hist[3, 4]), 9], 1.25]])]
    return rows, hist, hlen, guards, tables


def _sample(eng, family, s, B, t, seeds, steps, hist, hlen, guards, tables, force=None):
    if family == "plain":
        return eng.test_greedy_sample(s, B, t, seeds, steps, force_ids=force)
    return eng.test_greedy_sample(s, B, t, seeds, steps, hist=hist, hist_len=hlen, tables=tables if family == "bias" else None, force_ids=force, **guards)


@MODES
@pytest.mark.parametrize("family", ["plain", "guard", "bias"])
def test_selection_bit_for_bit(engines, family, mode):
    eng = engines(mode)
    V = 16388
    rng = np.random.default_rng(11)
    rows, hist, hlen, guards, tables = _family_inputs(V, family, rng)
    g = GenerationGuards(**guards)
    t = [0.7, 1.0, 0.2, 2.0]
    seeds = [3, 0x123456789ABCDEF0, 17, 1]
    steps = [0, 7, 1000, 2]
    for ks in (1, 2):
        tok, raw, lp, noise = _sample(eng, family, slabs(rows, ks), 4, t, seeds, steps, hist, hlen, guards, tables)
        for b in range(4):
            assert same_bits(raw[b], rows[b]), "the dump is the raw logits"
            s = chain(raw[b], hist[b, :hlen[b]], tables[b] if tables else None, g) if family != "plain" else raw[b]
            want, y = select(s, t[b], noise[b])
            assert int(tok[b]) == want, (family, ks, b, int(tok[b]), want)
            assert np.abs(noise[b].astype(np.float64) - sampling.gumbel_noise(seeds[b], steps[b], V)).max() <= sampling.EPS_G
            check_lp((family, mode, ks, b), lp[b], s, tok[b])
    # the draw is rarely the argmax of s at these temperatures: the recomputed score of the token is really exercised
    assert any(int(tok[b]) != int(np.argmax(rows[b])) for b in range(4))


@MODES
@pytest.mark.parametrize("family", ["plain", "guard", "bias"])
def test_rows_with_t_zero(engines, family, mode):
    """t = 0 rows among t > 0 rows: token and out_lp bits of the LP kernels on the same inputs"""
    eng = engines(mode)
    V = 16388
    rng = np.random.default_rng(12)
    rows, hist, hlen, guards, tables = _family_inputs(V, family, rng)
    t = [0.0, 1.0, 0.0, 0.6]
    for ks in (1, 2):
        s = slabs(rows, ks)
        tok, raw, lp, noise = _sample(eng, family, s, 4, t, [5, 6, 7, 8], [0, 3, 9, 1], hist, hlen, guards, tables)
        if family == "plain":
            tok0, _, lp0 = eng.test_greedy_lp(s, 4)
        elif family == "guard":
            tok0, _, lp0 = eng.test_greedy_guard(s, 4, hist, hlen, want_lp=True, **guards)
        else:
            tok0, _, lp0 = eng.test_greedy_bias(s, 4, hist, hlen, tables, want_lp=True, **guards)
        for b in (0, 2):
            assert int(tok[b]) == int(tok0[b]) and same_bits(lp[b], lp0[b]), (family, ks, b, int(tok[b]), int(tok0[b]), float(lp[b]), float(lp0[b]))
            assert not noise[b].any()                                              # no noise was drawn for them
        assert noise[1].any() and noise[3].any()


# ------------------------------------------------------------------------------------------ 4. bans
@MODES
def test_bans_and_forced(engines, mode):
    eng = engines(mode)
    V = 16388
    rng = np.random.default_rng(13)
    rows = [bf16_exact(rng.uniform(-2.0, 2.0, V)) for _ in range(4)]
    rows[3][:] = NEG
    rows[3][[11, V // 5, V - 7]] = [1.0, 2.0, 3.0]
    hist, hlen = histories(V, 4, rng)
    t, seeds, steps = [1.0, 0.5, 2.0, 1.0], [21, 22, 23, 24], [0, 1, 2, 3]
    s = slabs(rows, 1)
    tok, raw, lp, noise = eng.test_greedy_sample(s, 4, t, seeds, steps, hist=hist, hist_len=hlen)
    # the 32 highest ids of y of rows 0 .. 2 are suppressed (one list for the launch), and row 3's three finite ids with them: none is emitted
    banned = set()
    for b in range(3):
        _, y = select(GenerationGuards().apply(raw[b], hist[b, :hlen[b]]), t[b], noise[b])
        banned |= {int(i) for i in np.argsort(-y, kind="stable")[:32]}
        assert int(tok[b]) in banned
    banned |= {11, V // 5, V - 7}
    sup = sorted(banned)
    assert len(sup) <= 256
    g = GenerationGuards(suppress_tokens=sup)
    tok2, raw2, lp2, noise2 = eng.test_greedy_sample(s, 4, t, seeds, steps, hist=hist, hist_len=hlen, suppress_tokens=sup)
    assert same_bits(noise2, noise)
    for b in range(3):
        sc = g.apply(raw2[b], hist[b, :hlen[b]])
        want, _ = select(sc, t[b], noise2[b])
        assert int(tok2[b]) == want and int(tok2[b]) not in banned, (b, int(tok2[b]))
        check_lp(("banned", mode, b), lp2[b], sc, tok2[b])
    assert int(tok2[3]) == 0                                                       # every score -inf: the first of equal values
    # a forced id wins over the draw, and its log-probability is that id's
    force = np.array([V - 1, 0, 4097, 11], np.int32)
    tok3, raw3, lp3, _ = eng.test_greedy_sample(s, 4, t, seeds, steps, hist=hist, hist_len=hlen, force_ids=force)
    assert tok3.tolist() == force.tolist()
    for b in range(4):
        check_lp(("forced", mode, b), lp3[b], GenerationGuards().apply(raw3[b], hist[b, :hlen[b]]), force[b])


# ------------------------------------------------------------------------------------------ 5. the distribution
@MODES
def test_distribution(engines, mode):
    """V = 16, s_i = 0.5 i - 4, t = 2: 4096 draws (64 rows x 64 launches, seeds 0 .. 4095) against softmax(s / 2); Pearson chi-square, 15 degrees of freedom, below
    the 1e-4 quantile 44.3.  The definition alone gives 15.99 (step 0) and 12.35 (step 7); the seeds are fixed, so nothing here can flake."""
    eng = engines(mode)
    V, B = 16, 64
    sc = (0.5 * np.arange(V) - 4).astype(np.float32)
    s = slabs([sc] * B, 1, mpad=B)
    p = np.exp(sc.astype(np.float64) / 2)
    p /= p.sum()
    e = p * 4096
    assert e.min() > 21.7
    for step in (0, 7):
        cnt = np.zeros(V)
        for k in range(64):
            tok, _, _, _ = eng.test_greedy_sample(s, B, [2.0] * B, list(range(64 * k, 64 * k + 64)), [step] * B, want_noise=False)
            cnt += np.bincount(tok, minlength=V)
        chi2 = float(((cnt - e) ** 2 / e).sum())
        print(f"distribution mode={mode} step={step}: chi-square = {chi2:.2f} (15 dof; bound 44.3)")
        assert cnt.sum() == 4096 and chi2 < 44.3, (step, chi2, cnt.tolist())
