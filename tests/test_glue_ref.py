"""tests/glue_ref.py against float64 and against its own claims (no GPU): the references stay within the element type's u of the real-number result, the
integer constructions of tests/test_gpu_decode_glue.py are exact, and the random cases used there keep their ambiguous share under the caps."""
import numpy as np
import pytest

import glue_ref as G
from attn_ref import U, rounder, rope_table
from gpu_common import load_oracle

KINDS = ["bf16", "f16"]
F = np.float32


def representable(a, kind):
    a = np.asarray(a, F)
    return np.array_equal(rounder(kind)(a), a)


@pytest.mark.parametrize("kind", KINDS)
def test_norm_reference_against_float64(kind):
    """y_lo / y_hi sit within (2 u + u^2) |y64| of the real-number RMSNorm (two roundings), and differ from each other in few places"""
    u = U[kind]
    for rows, d, ks in G.NORM_RANDOM_CASES:
        x, slabs, w = G.norm_random(rows, d, ks, kind, G.NORM_SEED)
        xn = G.residual_add(x, G.slab_sum(slabs), kind)
        v64 = slabs.astype(np.float64).sum(axis=0); x64 = x.astype(np.float64) + v64
        assert np.all(np.abs(xn - x64) <= 1.01 * u * (np.abs(v64) + np.abs(x64)) + 2.0 ** -22)      # rt(v), then rt(x + .)
        lo, hi = G.norm_lo_hi(xn, w, 1e-5, kind)
        y64 = w * xn.astype(np.float64) / np.sqrt((xn.astype(np.float64) ** 2).mean(axis=1, keepdims=True) + float(F(1e-5)))
        for y in (lo, hi):
            assert np.all(np.abs(y - y64) <= (2 * u + u * u + 2.0 ** -17) * np.abs(y64) + 2.0 ** -24)
        ok, share = G.in_pair(lo, lo, hi)
        assert ok and share <= G.AMBIGUOUS_CAP[kind], (rows, d, share)
        assert share > 0 or d < 512                                    # the interval is not empty either: some elements do sit on a boundary


@pytest.mark.parametrize("kind", KINDS)
def test_o_chain_random_caps(kind):
    for M, K, D, ff in G.O_RANDOM_CASES:
        att, Wo, resid, w, _, _ = G.o_random(M, K, D, 16, kind, G.O_SEED)
        assert representable(att, kind) and representable(Wo, kind) and representable(resid, kind)
        assert np.abs(Wo).min() >= 2.0 ** -14                           # normal numbers in fp16 too
        lo, hi = G.o_resid_lo_hi(att, Wo, resid, kind)
        ok, share = G.in_pair(lo, lo, hi)
        assert ok and share <= G.AMBIGUOUS_CAP[kind], (M, K, D, share)
        for xn in (lo, hi):
            a, b = G.norm_lo_hi(xn, w, 1e-5, kind)
            assert G.in_pair(a, a, b)[1] <= G.AMBIGUOUS_CAP[kind]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,D", [(256, 256), (2048, 2048)])
def test_o_chain_exact_construction(kind, K, D):
    att, Wo, resid = G.o_chain_exact(64, K, D, 66, K + D)
    assert representable(att, kind) and representable(Wo, kind) and representable(resid[:64], kind)
    n = np.arange(D)
    assert np.all(n % K != (7 * n + 3) % K) and np.all((Wo != 0).sum(axis=1) == 2)
    v = att.astype(np.float64) @ Wo.T.astype(np.float64)
    assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 4
    assert np.array_equal(v, att[:, n % K] - att[:, (7 * n + 3) % K])
    xn = resid[:64] + v
    assert np.abs(xn).max() <= 12 and representable(xn, kind) and np.array_equal(G.residual_add(resid[:64], v, kind), xn)
    assert np.abs(att).sum(axis=1).max() * 2 < 2 ** 24 and D * 144 < 2 ** 24          # any partial sum of products / of squares is an exact fp32 integer
    assert np.all(np.abs(resid[64:]) == 1e4)                               # the sentinel rows (compared after the upload rounding)


@pytest.mark.parametrize("kind", KINDS)
def test_split_ints_and_add_rmsnorm_exact(kind):
    rng = np.random.default_rng(7)
    for d in (64, 264, 2048):
        v = rng.integers(-4, 5, size=(3, d)).astype(F); x = rng.integers(-8, 9, size=(3, d)).astype(F)
        for ks in (1, 3, 8):
            s = G.split_ints(rng, v, ks)
            assert np.array_equal(s, np.rint(s)) and np.abs(s).sum(axis=0).max() < 2 ** 24
            assert np.array_equal(G.slab_sum(s), v) and np.array_equal(G.slab_sum(s[::-1]), v)
            xn, y = G.add_rmsnorm(x, s, np.ones(d, F), 1e-5, kind)
            assert np.array_equal(xn, x + v)
            lo, hi = G.norm_lo_hi(xn, np.ones(d, F), 1e-5, kind)
            assert G.in_pair(y, lo, hi)[0]                               # the exact-scale result lies inside the random tests' acceptance set


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gu8", [0, 1])
def test_swiglu_exact_construction(kind, gu8):
    rt = rounder(kind)
    for ff, rows, ks in [(32, 1, 1), (2048, 17, 4), (2048, 1, 1)]:
        slabs, want = G.swiglu_exact(ff, rows, ks, gu8, kind, 5)
        assert representable(want, kind) and np.all(np.isfinite(want)) and np.abs(want).min() >= (2.0 ** -14 if kind == "f16" else 2.0 ** -126)   # normal numbers
        for r in range(rows):
            assert len(np.unique(want[r])) == ff                          # every output column of a row has its own value
        gi, ui = G.swiglu_maps(ff, gu8)
        assert sorted(np.concatenate([gi, ui]).tolist()) == list(range(2 * ff))   # the two maps tile the interleaved projection
        p64 = slabs[:, :rows].astype(np.float64).sum(axis=0)
        assert np.array_equal(G.slab_sum(slabs[:, :rows]).astype(np.float64), p64)    # the slab sums are exact
        g = p64[:, gi]
        assert np.array_equal(g, np.broadcast_to(16 + np.arange(ff) % 16, g.shape))
        assert np.array_equal(rt((g / (1.0 + np.exp(-g))).astype(F)), g)   # silu(g) rounds to g
        assert np.array_equal(G.swiglu(slabs, rows, gu8, kind), want)
    # the reference on random data against float64: three roundings
    rng = np.random.default_rng(11)
    slabs = rng.standard_normal((3, 4, 128)).astype(F)
    got = G.swiglu(slabs, 4, gu8, kind)
    p = slabs.astype(np.float64).sum(axis=0); gi, ui = G.swiglu_maps(64, gu8)
    ref = p[:, gi] / (1.0 + np.exp(-p[:, gi])) * p[:, ui]
    assert np.all(np.abs(got - ref) <= 4.5 * U[kind] * np.abs(ref) + 2.0 ** -24)


def test_quant_row_reference():
    for K in (64, 2048, 8192):
        X = G.quant_rows_data(K, K)
        assert representable(X[np.isfinite(X)], "f16") and X.shape[0] == 7
        n_out = []
        for y in X:
            codes, sca, cols, vals = G.quant_row(y)
            with np.errstate(invalid="ignore"):
                out = ~(np.abs(y) < 6.0)
            assert np.array_equal(cols, np.flatnonzero(out)) and np.all(np.diff(cols) > 0) and np.array_equal(vals, y[cols], equal_nan=True)
            assert np.all(codes[out] == 0)
            if (~out).any() and np.abs(y[~out]).max() > 0:
                a = np.abs(y[~out]).max()
                assert sca == a and np.abs(codes).max() == 127
                assert np.all(np.abs(codes[~out] - y[~out].astype(np.float64) * 127.0 / a) <= 0.5 + 1e-4)
            else:
                assert np.all(codes == 0)
            n_out.append(len(cols))
        assert n_out[0] == 0 and n_out[1] == len({c for c in G.OUTLIER_COLS if c < K - 1} | {K - 1}) and n_out[2] == 2
        assert n_out[3] == min(70, K - 4) and (K == 64 or n_out[3] > G.OUTL_CAP) and n_out[4] == 0 and n_out[5] == K and n_out[6] == 1
        assert G.quant_row(X[4])[1] == 0.0
        assert G.quant_row(X[5])[1] == -G.FLT_MIN                         # nothing below the threshold: amax keeps its initial value, as in the oracle's linear_int8
        assert 5.99609375 in X[2] and 6.0 in X[2] and -6.0 in X[2]


def test_norm_quant_rows_are_what_they_claim():
    xp, w, eps = G.norm_quant_data(2048, 2048)
    assert representable(xp, "f16") and representable(w, "f16")
    _, y = G.add_rmsnorm(np.zeros_like(xp), xp[None], w, eps, "f16")
    cnt = [len(G.quant_row(r)[2]) for r in y]
    assert cnt[0] == 0 and cnt[1] == 6 and cnt[2] == 6 and cnt[3] >= 65 and cnt[4] == 0
    assert np.array_equal(G.quant_row(y[1])[2], sorted(list(G.OUTLIER_COLS) + [2047]))
    assert set(np.abs(y[2][list(G.OUTLIER_COLS)])) == {6.0} and abs(y[2][100]) == 5.99609375 and np.all(y[4] == 0)
    assert (y[2][list(G.OUTLIER_COLS) + [2047]] > 0).any() and (y[2][list(G.OUTLIER_COLS) + [2047]] < 0).any()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rd,hd", [(128, 128), (64, 64), (32, 64)])
def test_rope_reference(kind, rd, hd):
    rng = np.random.default_rng(rd)
    T = 9
    x = rounder(kind)(rng.standard_normal((T, 3, hd)))
    cs = rope_table(T, hd=rd)
    got = G.rope(x, cs[:, None, :], rd, kind)
    assert np.array_equal(got[..., rd:], x[..., rd:])
    h = rd // 2
    c, s = cs[:, None, :h].astype(np.float64), cs[:, None, h:].astype(np.float64)
    x1, x2 = x[..., :h].astype(np.float64), x[..., h:rd].astype(np.float64)
    ref = np.concatenate([x1 * c - x2 * s, x2 * c + x1 * s], axis=-1)
    mag = np.concatenate([np.abs(x1 * c) + np.abs(x2 * s), np.abs(x2 * c) + np.abs(x1 * s)], axis=-1)
    assert np.all(np.abs(got[..., :rd] - ref) <= U[kind] * (mag + np.abs(ref)) * 1.01 + 2.0 ** -24)
    assert np.array_equal(got[0], x[0])                                 # position 0: cos 1, sin 0
    if rd == 128:                                                       # the same statement as the fused decode prologue's
        from attn_ref import fused_prologue
        q, k, v = fused_prologue(x.reshape(1, T, 3 * 128), cs, 1, 1, kind)
        assert np.array_equal(q[:, 0], got[:, 0]) and np.array_equal(k[:, 0], got[:, 1]) and np.array_equal(v[:, 0], x[:, 2])


# ------------------------------------------------------------------------------------------ the int8 token step's references (tests/test_gpu_int8_decode_glue.py)
@pytest.fixture(scope="module")
def orc():
    return load_oracle()


def oracle_rows(orc, X, W):
    """the Linear's spec: one reference call per row"""
    cb, scb = orc.quantize_rows(W)
    return np.concatenate([orc.linear_int8(X[i:i + 1], cb, scb) for i in range(X.shape[0])]), cb, scb


def test_i8_rows_are_what_they_claim():
    for K in (256, 768, 2048):
        X, n = G.i8_rows(K, 64, K)
        assert representable(X, "f16") and list(n[:13]) == [K if c < 0 else min(c, K) for c in G.I8_COUNTS]
        for i, y in enumerate(X):
            cols = G.quant_row(y)[2]
            assert len(cols) == n[i], (K, i)
            if n[i] >= 4:
                assert {0, 63, 64, K - 1} <= set(cols.tolist())
            if n[i]:
                assert y[0] == (6.0 if i % 2 == 0 else -6.0)                   # exactly the threshold: an outlier
            if n[i] < K and abs(y[(i % 4) * (K // 4) + 1]) < 6:
                assert abs(y[(i % 4) * (K // 4) + 1]) == G.F16_BELOW_6         # the largest fp16 below it: not one
            if 4 < n[i] < K:
                assert (y[cols] > 0).any() and (y[cols] < 0).any()
        am, big = G.i8_partials(X)
        assert np.array_equal(big.sum(axis=1), n) and set(am.argmax(axis=1)[n < K].tolist()) == {0, 1, 2, 3}
        for i, y in enumerate(X):                                               # the maximum of the partials is the row's scale (0 for -FLT_MIN: no element below 6)
            a = G.quant_row(y)[1]
            assert am[i].max() == (a if a > 0 else 0.0)


def test_int8_product_and_dequant_against_the_oracle(orc):
    """glue_ref.int8_product equals the plain int64 product, and on rows without outliers its dequantisation IS oracle.linear_int8, bit for bit"""
    rng = np.random.default_rng(3)
    a = rng.integers(-127, 128, size=(5, 512)).astype(np.int8); b = rng.integers(-127, 128, size=(48, 512)).astype(np.int8)
    assert np.array_equal(G.int8_product(a, b), np.einsum("mk,nk->mn", a.astype(np.int64), b.astype(np.int64)))
    full = np.full((1, 8192), 127, np.int8)
    assert G.int8_product(full, -full)[0, 0] == -8192 * 127 * 127
    for N, K in [(256, 256), (256, 1024), (1024, 768)]:
        X, n = G.i8_rows(K, 64, N + K)
        W = G.i8_weights(N, K, N * K)
        X = X[n == 0]
        assert X.shape[0] >= 4
        lin, cb, scb = oracle_rows(orc, X, W)
        P = G.int8_product(G.i8_codes(X), cb)
        for i in range(X.shape[0]):
            got = G.i8_dequant(P[i], G.quant_row(X[i])[1], scb)
            assert np.array_equal(got.view(np.uint32), lin[i].view(np.uint32)), (N, K, i)


def test_i8_norm_cases_keep_the_ambiguity_cap(orc):
    """the norm consumer's reference alone - the oracle's rows, the residual add, norm_lo_hi - stays under the fp16 cap for the data and every row count the GPU
    test uses; the partials of the on-the-fly form put their maximum into each of the four slots"""
    for N, K, _, _, forms, Ms in G.I8_NORM_CASES:
        X, n, W, x, w = G.i8_norm_data(N, K)
        M = max(Ms)
        lin, _, _ = oracle_rows(orc, X[:M], W)
        assert np.all(np.isfinite(lin)) and representable(lin, "f16")
        xn = G.residual_add(x[:M], lin, "f16")
        lo, hi = G.norm_lo_hi(xn, w, 1e-5, "f16")
        for m in Ms:
            ok, share = G.in_pair(lo[:m], lo[:m], hi[:m])
            assert ok and share <= G.AMBIGUOUS_CAP["f16"], (N, K, m, share)
        if 1 in forms and M >= 4:
            assert set(G.i8_partials(X[:M])[0].argmax(axis=1)[n[:M] < K].tolist()) == {0, 1, 2, 3}


def test_head_partials():
    out = np.zeros((2, 4, 128), F)
    out[0, 0, 5] = -5.5; out[0, 1, 7] = 6.0; out[0, 1, 8] = 3.0; out[0, 3, 0] = np.float32(-7.25); out[1, 2, 127] = G.F16_BELOW_6
    am, big = G.head_partials(out, 2)
    assert am.tolist() == [[5.5, 0.0], [0.0, float(G.F16_BELOW_6)]] and big.tolist() == [[1, 1], [0, 0]]
    am, big = G.head_partials(out, 4)
    assert am.tolist() == [[5.5, 3.0, 0.0, 0.0], [0.0, 0.0, float(G.F16_BELOW_6), 0.0]] and big.tolist() == [[0, 1, 0, 1], [0, 0, 0, 0]]


def test_i8_attn_data_keeps_the_bounds_premise(orc):
    """the int8 attention cases, from the reference alone: fp16 probabilities that leave the normal range cost at most a quarter of the c = 1 bound (attn_ref's
    docstring; the data keeps q and k near N(0, 1.2) and gives the rows with many outliers one key), and the outputs put heads on both sides of 6.0"""
    from attn_ref import attention, fused_prologue
    scale = 1.0 / np.sqrt(128.0)
    for Hq, Hkv, D, _, _, Bs in G.I8_ATTN_CASES:
        B = max(Bs)
        d = G.i8_attn_data(Hq, Hkv, D, B)
        assert representable(d["X"], "f16") and representable(d["W"], "f16") and np.abs(d["W"][d["W"] != 0]).min() >= 2.0 ** -24
        assert set(d["kv_len"].tolist()) >= {1, 128, G.I8_ATTN_CTX - 1} and np.all(d["kv_len"][d["n"] >= 63] == 1)
        lin, _, _ = oracle_rows(orc, d["X"], d["W"])
        pos = d["kv_len"] - 1
        q, k_new, v_new = fused_prologue(lin[None], d["cs"][pos], Hq, Hkv, "f16")
        kc, vc = d["kc"].copy(), d["vc"].copy()
        assert np.all(np.abs(kc[np.arange(B), :, pos]) == 1e4) and np.all(np.abs(vc[np.arange(B), :, pos]) == 1e4)      # poison where the kernel appends, and behind
        kc[np.arange(B), :, pos] = k_new; vc[np.arange(B), :, pos] = v_new
        out = np.zeros((B, Hq, 128), F)
        for b in range(B):
            for h in range(Hq):
                g = h // (Hq // Hkv)
                assert G.f16_subnormal_share(q[b, h], kc[b, g], vc[b, g], int(d["kv_len"][b]), scale) <= 0.25, (Hq, D, b, h)
                out[b, h] = rounder("f16")(attention(q[b, h][None], kc[b, g], vc[b, g], [d["kv_len"][b]], scale)[0][0])
        am, big = G.head_partials(out, Hkv)
        assert (big > 0).any() and (big == 0).any() and ((big > 0) & (am > 0)).any()
