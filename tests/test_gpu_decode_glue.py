"""The kernels between the decode step's GEMMs, and the prefill's RoPE / KV append, each launched the way decode_step() / run_prefill() launch it on
caller-made data (the sonic_test_* hooks of csrc/engine_hooks.cpp) and compared with tests/glue_ref.py, which restates every kernel's rounding points.

Two kinds of check:
  * exact data, bit for bit (np.array_equal): small integers and powers of two, for which every sum is exact in fp32 in ANY order, so the result does not
    depend on a reduction tree and one wrong element, lane map or slab index shows;
  * random data against the reference with a derived acceptance set (glue_ref's docstring): the only free quantity of a norm kernel is the RMSNorm scale,
    within r64 (1 -+ 2^-18); every element must equal one of the two values that interval allows, the residual rows stay bit-exact.

Buffers are larger than the kernels may touch and hold finite poison / sentinels there (+-1e4), which must come back as they went in.
"""
import numpy as np
import pytest

import glue_ref as G
from gpu_common import bits, make_engine
from sonicscribe_amd.engine import MODE_F16

pytestmark = pytest.mark.gpu

KINDS = ["bf16", "f16"]
F = np.float32
EPS = 1e-5


@pytest.fixture(scope="module")
def eng():
    e = make_engine(max_ctx=256)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng16():
    e = make_engine(mode=MODE_F16, max_ctx=256)
    yield e
    e.close()


@pytest.fixture
def E(eng, eng16):
    """kind -> engine, with the decode-step knobs back at their defaults afterwards"""
    engines = {"bf16": eng, "f16": eng16}
    yield lambda kind: engines[kind]
    for e in engines.values():
        e.set_option("gu64_two_pass", 0); e.set_option("o64_16rows", 0)


def same(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (what, len(bad), "first at", bad[0].tolist(), float(got[tuple(bad[0])]), float(want[tuple(bad[0])]))


def poison(shape, kind, flip=False):
    n = int(np.prod(shape))
    return G.rounder(kind)(np.where((np.arange(n) % 2 == 0) != flip, 1e4, -1e4).astype(F)).reshape(shape)


# ------------------------------------------------------------------------------------------ o_proj -> norm -> gate/up
@pytest.fixture(scope="module")
def gu_weights():
    """one gate/up matrix per D for the exact tests (they compare forms with each other: any weights do)"""
    rng = np.random.default_rng(99)
    out = {}
    for D in (256, 2048):
        out[D] = G.interleave16(G.rounder("bf16")(rng.standard_normal((2048, D)) * 0.05), G.rounder("bf16")(rng.standard_normal((2048, D)) * 0.05))
    return out


@pytest.mark.parametrize("M", [1, 5, 16, 17, 32, 33, 47, 64])
@pytest.mark.parametrize("K,D", [(256, 256), (2048, 2048)])
@pytest.mark.parametrize("kind", KINDS)
def test_o_chain_exact(E, gu_weights, kind, K, D, M):
    """integer data (glue_ref.o_chain_exact): resid_out, the row totals of SS and hn_out equal the fp32 emulation bit for bit in forms 0, 1, 2; act_out has the
    same bits in every form, also under gu64_two_pass and o64_16rows; the sentinel rows behind M come back untouched"""
    e = E(kind)
    rt = G.rounder(kind)
    rows_alloc = M + 3
    att, Wo, resid = G.o_chain_exact(M, K, D, rows_alloc, 1000 * M + D)
    w = np.random.default_rng(M).uniform(0.5, 1.5, size=D).astype(F)
    v = att[:, np.arange(D) % K] - att[:, (7 * np.arange(D) + 3) % K]
    want_resid = np.concatenate([G.residual_add(resid[:M], v, kind), rt(resid[M:])])
    tot = G.sumsq_exact(want_resid[:M])
    want_hn = G.norm_apply(want_resid[:M], w, G.scale32(tot.astype(F), D, EPS), kind)

    def check(tag):
        r = {f: e.test_decode_o_gu(att, Wo, resid, w, EPS, gu_weights[D], f, want_ss=f < 2) for f in (0, 1, 2)}
        for f in (0, 1, 2):
            same(r[f]["resid"], want_resid, (tag, "resid_out, form", f))
        for f in (0, 1):
            ss = r[f]["ss"]                                                  # [region][D / 64][32][4] -> per row: all partials of region row // 32, slot row % 32
            got_tot = np.asarray([ss[m >> 5, :, m & 31, :].astype(np.float64).sum() for m in range(M)])
            assert np.array_equal(got_tot, tot), (tag, "SS row totals, form", f, np.flatnonzero(got_tot != tot)[:4].tolist())
        same(r[1]["hn"], want_hn, (tag, "hn_out of rmsnorm_ss"))
        same(r[2]["hn"], want_hn, (tag, "hn_out of add_rmsnorm"))
        assert np.all(np.isfinite(r[0]["act"]))
        same(r[1]["act"], r[0]["act"], (tag, "act_out, form 1 against form 0"))
        same(r[2]["act"], r[0]["act"], (tag, "act_out, form 2 against form 0"))
        return r[0]["act"]

    act = check("default")
    if M > 32:                                                               # the knobs only change the 33 .. 64 row launches
        for key in ("gu64_two_pass", "o64_16rows"):
            e.set_option(key, 1)
            same(check(key), act, (key, "act_out against the default launch"))
            e.set_option(key, 0)


@pytest.mark.parametrize("M,K,D,ff", G.O_RANDOM_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_o_chain_random(E, kind, M, K, D, ff):
    """random data without cancellation in the o_proj sum: resid_out within the two values v64 (1 -+ 2^-17) allows, hn_out within the two values
    r64 (1 -+ 2^-18) allows (computed from the kernel's own residual rows), act_out against float64 within test_skinny_fused_gate_up's bound"""
    e = E(kind)
    rt = G.rounder(kind)
    att, Wo, resid, w, Wg, Wu = G.o_random(M, K, D, ff, kind, G.O_SEED)
    Wi = G.interleave16(Wg, Wu)
    lo, hi = G.o_resid_lo_hi(att, Wo, resid, kind)
    r = {f: e.test_decode_o_gu(att, Wo, resid, w, EPS, Wi, f) for f in (0, 1, 2)}
    same(r[1]["resid"], r[0]["resid"], "resid_out, form 1 against form 0")
    worst_gu = 0.0
    for f in (0, 1, 2):
        ok, share = G.in_pair(r[f]["resid"], lo, hi)
        print(f"{kind} M={M} K={K} D={D} form {f}: resid_out ambiguous share {share:.5f} (cap {G.AMBIGUOUS_CAP[kind]})")
        assert share <= G.AMBIGUOUS_CAP[kind]
        assert ok, ("resid_out outside the acceptance set, form", f, int(np.sum((bits(r[f]["resid"]) != bits(lo)) & (bits(r[f]["resid"]) != bits(hi)))))
        hn = r[f]["hn"] if f else r[1]["hn"]                                  # form 0 never materialises hn: its act is checked against form 1's (same bits as form 0's input)
        if f:
            ylo, yhi = G.norm_lo_hi(r[f]["resid"], w, EPS, kind)
            ok, share = G.in_pair(hn, ylo, yhi)
            print(f"{kind} M={M} K={K} D={D} form {f}: hn_out ambiguous share {share:.5f}")
            assert share <= G.AMBIGUOUS_CAP[kind]
            assert ok, ("hn_out outside the acceptance set, form", f)
        gg = rt((hn.astype(np.float64) @ Wg.T.astype(np.float64)).astype(F)); uu = rt((hn.astype(np.float64) @ Wu.T.astype(np.float64)).astype(F))
        ref = rt(rt(gg / (1.0 + np.exp(-gg))) * uu)
        tol = 4 * np.maximum(np.abs(ref), 1e-2) * 2.0 ** -8 + 1e-3           # test_gpu_parity.py::test_skinny_fused_gate_up: ulp_tol(ref, 4) + 1e-3
        sh = float((np.abs(r[f]["act"] - ref) / tol).max())
        worst_gu = max(worst_gu, sh)
        assert sh <= 1.0, ("act_out, form", f, sh)
    same(r[1]["act"], r[0]["act"], "act_out, form 1 against form 0")
    print(f"{kind} M={M} K={K} D={D}: worst share of the gate/up bound {worst_gu:.3f}")


# ------------------------------------------------------------------------------------------ add_rmsnorm
@pytest.mark.parametrize("d", [64, 264, 2048])                              # 264: 33 active threads, a partial wave
@pytest.mark.parametrize("kind", KINDS)
def test_add_rmsnorm_exact(E, kind, d):
    e = E(kind)
    rt = G.rounder(kind)
    rng = np.random.default_rng(d)
    w = rng.uniform(0.5, 1.5, size=d).astype(F)
    for rows in (1, 3, 64):
        for ks in (1, 3, 8):
            rows_alloc, mpad = rows + 2, (rows + 15) // 16 * 16 + 16
            x = poison((rows_alloc, d), kind); x[:rows] = rng.integers(-8, 9, size=(rows, d))
            v = rng.integers(-4, 5, size=(rows, d)).astype(F)
            slabs = np.full((ks, mpad, d), 1e4, F); slabs[:, :rows] = G.split_ints(rng, v, ks)
            y0 = poison((rows_alloc, d), kind, flip=True)
            xo, yo = e.test_add_rmsnorm(x, slabs, w, EPS, rows, y_init=y0)
            xn, y = G.add_rmsnorm(x[:rows], slabs[:, :rows], w, EPS, kind)
            assert np.array_equal(xn, x[:rows] + v)
            same(xo, np.concatenate([xn, x[rows:]]), ("x_out", rows, ks))
            same(yo, np.concatenate([y, y0[rows:]]), ("y_out", rows, ks))


@pytest.mark.parametrize("rows,d,ks", G.NORM_RANDOM_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_add_rmsnorm_random(E, kind, rows, d, ks):
    e = E(kind)
    x, slabs, w = G.norm_random(rows, d, ks, kind, G.NORM_SEED)
    xo, yo = e.test_add_rmsnorm(x, slabs, w, EPS, rows)
    xn = G.residual_add(x, G.slab_sum(slabs), kind)
    same(xo, xn, "x_out (fixed ascending slab order: exact)")
    lo, hi = G.norm_lo_hi(xn, w, EPS, kind)
    ok, share = G.in_pair(yo, lo, hi)
    print(f"{kind} rows={rows} d={d} ksplit={ks}: y_out ambiguous share {share:.5f} (cap {G.AMBIGUOUS_CAP[kind]})")
    assert share <= G.AMBIGUOUS_CAP[kind]
    assert ok, ("y_out outside the acceptance set", int(np.sum((bits(yo) != bits(lo)) & (bits(yo) != bits(hi)))))


# ------------------------------------------------------------------------------------------ SwiGLU of the slabs
@pytest.mark.parametrize("gu8", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_swiglu_slab_exact(E, kind, gu8):
    e = E(kind)
    for ff in (32, 2048):
        for rows in (1, 17):
            for ks in (1, 4):
                slabs, want = G.swiglu_exact(ff, rows, ks, gu8, kind, ff + rows)
                got = e.test_swiglu_slab(slabs, rows, gu8)
                same(got, want, ("act", ff, rows, ks))
                same(got, G.swiglu(slabs, rows, gu8, kind), ("act against the reference", ff, rows, ks))


# ------------------------------------------------------------------------------------------ the row quantiser (fp16 engines)
def check_quant(qb, Y, what):
    q, sca, cnt, lst, val = qb
    for i, y in enumerate(Y):
        codes, a, cols, vals = G.quant_row(y)
        n = len(cols)
        assert cnt[i] == n, (what, "row", i, "oc_cnt", int(cnt[i]), n)
        assert bits(sca[i:i + 1])[0] == bits(np.asarray([a]))[0], (what, "row", i, "sca", float(sca[i]), float(a))
        assert np.array_equal(q[i], codes), (what, "row", i, "codes differ at", np.flatnonzero(q[i] != codes)[:8].tolist())
        assert np.array_equal(lst[i, :n], cols), (what, "row", i, "oc_list", lst[i, :n][:8].tolist(), cols[:8].tolist())
        assert np.all(lst[i, n:] == -1) and np.all(val[i, n:] == 0), (what, "row", i, "written behind the list's end")
        assert np.array_equal(val[i, :n], vals, equal_nan=True), (what, "row", i, "oc_val")


@pytest.mark.parametrize("K", [64, 2048, 8192])
def test_quant_rows_exact(eng16, K):
    """no outlier; outliers across thread and wave boundaries; +-6.0 and 5.996; a list longer than OUTL_CAP; all zero (sca 0); all outliers (amax keeps its initial
    value: sca is -FLT_MIN = -1.17549435e-38, as oracle/sonic_oracle.c linear_int8 leaves it; the codes are 0 either way); a NaN (an outlier)"""
    Y = G.quant_rows_data(K, K)
    ld = K + 24
    X = np.full((Y.shape[0], ld), 7.0, F); X[:, :K] = Y                     # the pad holds outliers: a kernel that ran past K would list them
    check_quant(eng16.test_quant_rows(X, K), Y, ("quant_rows", K))
    check_quant(eng16.test_quant_rows(Y), Y, ("quant_rows, ld == K", K))


def test_add_rmsnorm_quant_exact(eng16):
    """add_rmsnorm + QuantOut at d = 2048: the normalised rows of glue_ref.norm_quant_data, and a row with a NaN (every element of y is NaN: all outliers)"""
    d = 2048
    xp, w, eps = G.norm_quant_data(d, d)
    rows = xp.shape[0] + 1
    x = np.zeros((rows, d), F); x[-1, 5] = np.nan
    rng = np.random.default_rng(3)
    slabs = np.full((3, rows + 16, d), 1e4, F)
    slabs[:, :rows] = G.split_ints(rng, np.concatenate([xp, 2 * np.ones((1, d), F)]), 3, spread=20)
    xo, yo, qb = eng16.test_add_rmsnorm(x, slabs, w, eps, rows, quant=True)
    xn, y = G.add_rmsnorm(x, slabs[:, :rows], w, eps, "f16")
    assert np.array_equal(xn[:-1], xp) and np.isnan(y[-1]).all()
    assert np.array_equal(xo, xn, equal_nan=True) and np.array_equal(bits(yo[:-1]), bits(y[:-1])) and np.isnan(yo[-1]).all()
    check_quant(qb, y, "add_rmsnorm + QuantOut")
    assert qb[2][-1] == d and bits(qb[1][-1:])[0] == bits(np.asarray([-G.FLT_MIN]))[0]


# ------------------------------------------------------------------------------------------ prefill RoPE + KV append
@pytest.mark.parametrize("vt_ld", [64, 68])                                 # 68: not a multiple of 8 - the scalar V^T path
@pytest.mark.parametrize("tiled", [1, 0])
@pytest.mark.parametrize("kind", KINDS)
def test_rope_append(E, kind, tiled, vt_ld):
    e = E(kind)
    rt = G.rounder(kind)
    rng = np.random.default_rng(37)
    B, Hq, Hkv, ctx = 3, 4, 2, 64
    q_len = np.asarray([1, 16, 37]); order = [2, 0, 1]                      # packed in shuffled sequence order
    q_off = np.zeros(B, np.int64); at = 0
    for b in order:
        q_off[b] = at; at += q_len[b]
    n_tok = at
    tok_seq = np.zeros(n_tok, np.int32); tok_pos = np.zeros(n_tok, np.int32)
    for b in range(B):
        tok_seq[q_off[b]:q_off[b] + q_len[b]] = b; tok_pos[q_off[b]:q_off[b] + q_len[b]] = np.arange(q_len[b])
    qkv = rt(rng.standard_normal((n_tok, Hq + 2 * Hkv, 128)))
    cs = G.rope_table(ctx)
    kc0 = poison((B, Hkv, ctx, 128), kind); vc0 = poison((B, Hkv, ctx, 128), kind, flip=True); vt0 = poison((B, Hkv, 128, vt_ld), kind)
    roped = G.rope(qkv[:, :Hq + Hkv], cs[tok_pos][:, None, :], 128, kind)
    want_k, want_v, want_vt = kc0.copy(), vc0.copy(), vt0.copy()
    for t in range(n_tok):
        b, p = tok_seq[t], tok_pos[t]
        want_k[b, :, p] = roped[t, Hq:]; want_v[b, :, p] = qkv[t, Hq + Hkv:]
        want_vt[b, :, :, p] = qkv[t, Hq + Hkv:]
    q, kc, vc, vt = e.test_rope_append(qkv.reshape(n_tok, -1), cs, tok_seq, tok_pos, q_off, q_len, Hq, kc0, vc0, vt0, bool(tiled))
    same(q, roped[:, :Hq], "q_out")
    same(kc, want_k, "K cache [b, kv head, position, dim]")
    same(vc, want_v, "V cache [b, kv head, position, dim]")
    same(vt, want_vt, "V^T [b, kv head, dim, position]")
    for b in range(B):                                                       # (stated on its own: V^T is the transpose of what the V cache received)
        assert np.array_equal(vt[b, :, :, :q_len[b]], np.swapaxes(vc[b, :, :q_len[b]], 1, 2))


def test_rope_append_refuses_what_the_tile_kernel_assumes(eng):
    """the tile kernel takes a tile's first position from its first token: the hook refuses plans whose positions are not 0 .. q_len - 1 in packing order"""
    from sonicscribe_amd.engine import SonicError
    z = np.zeros((1, 1, 64, 128), F)
    args = dict(qkv=np.zeros((4, 3 * 128), F), cs=G.rope_table(64), tok_seq=[0] * 4, q_off=[0], q_len=[4], Hq=1, kcache=z, vcache=z, vt=np.zeros((1, 1, 128, 64), F), tiled=True)
    eng.test_rope_append(tok_pos=[0, 1, 2, 3], **args)
    for bad in ([1, 2, 3, 4], [0, 2, 1, 3], [0, 1, 2, 64]):
        with pytest.raises(SonicError):
            eng.test_rope_append(tok_pos=bad, **args)
    with pytest.raises(SonicError):
        eng.test_rope_append(tok_pos=[0, 1, 2, 3], **dict(args, q_len=[3]))


@pytest.mark.parametrize("rd", [32, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_rope_enc(E, kind, rd):
    e = E(kind)
    rt = G.rounder(kind)
    rng = np.random.default_rng(rd)
    T, heads2, hd = 5, 6, 64
    M, ld = 2 * T, heads2 * hd + 24
    qk = poison((M, ld), kind); qk[:, :heads2 * hd] = rt(rng.standard_normal((M, heads2 * hd)))
    cs = G.rope_table(T, hd=rd)
    want = qk.copy()
    want[:, :heads2 * hd] = G.rope(qk[:, :heads2 * hd].reshape(M, heads2, hd), cs[np.arange(M) % T][:, None, :], rd, kind).reshape(M, -1)
    got = e.test_rope_enc(qk, T, heads2, rd, cs)
    same(got, want, "qk [row, column]")
    keep = np.ones(ld, bool); keep[:heads2 * hd] = (np.arange(heads2 * hd) % hd) >= rd
    assert np.array_equal(bits(got[:, keep]), bits(qk[:, keep]))
