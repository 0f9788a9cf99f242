"""The int8 token step's dequantising consumers, each behind one decode-flavour Linear8bitLt run the way decode_step_i8() runs it (the sonic_test_decode_i8_* hooks of
csrc/engine_hooks.cpp: launch_quant_rows or the on-the-fly form, skinny_i8 into int32 slabs, deq_info, then the consumer's own launcher).

The contract is tests/test_gpu_int8.py's: the int32 products are exact and the dequantisation follows the oracle's operation order, so the Linear agrees with
oracle.linear_int8(x_row[None], *oracle.quantize_rows(W)) - one reference call per row - bit for bit.  Nothing here is measured:
  * the slab sum equals, as integers, the rows' codes (glue_ref.quant_row) times CB^T (glue_ref.int8_product);
  * add_rmsnorm: x_out = glue_ref.residual_add(x, lin) bit for bit, every element of y one of the two values glue_ref.norm_lo_hi allows for the kernel's own residual
    rows (under AMBIGUOUS_CAP; tests/test_glue_ref.py checks the cap for this data on the CPU), the five quantiser outputs = glue_ref.quant_row of the kernel's own y;
  * swiglu_quant: act = glue_ref.swiglu of lin as one fp32 slab, bit for bit; the quantiser outputs likewise;
  * decode attention: lin as ONE fp32 slab through attn_ref.fused_prologue: the appended K / V rows bit for bit, every other cache element as uploaded, the output within
    1.5 u (A + |o|) of the float64 attention - what tests/test_gpu_attn_kernels.py holds the fp16 kernel to -, amax_out / big_out bit-exact functions of the kernel's own output;
  * form 0 (listed outliers) and form 1 (on-the-fly quantisation, the consumer scans) agree in every bit, and so do the tiled and the k-major weight copy.
The hooks return the GEMM's ksplit and tiling as launched; every case asserts both, so a shape that lands on another kernel fails.

Rows carry 0, 1, 2, 3, 4, 5, 7, 63, 64, 65, 66, 129 and K outliers (glue_ref.i8_rows): every tail of the consumers' pair and quad walks, both sides of the 64-entry LDS
stage, the spill path of the scanning form.  Buffers are larger than the kernels may touch and hold finite poison there, which must come back as it went in.
"""
import numpy as np
import pytest

import attn_ref as R
import glue_ref as G
from gpu_common import bits, load_oracle, make_engine
from sonicscribe_amd.engine import MODE_INT8
from test_gpu_attn_kernels import SCALE, decode_ratio
from test_gpu_decode_glue import check_quant, poison, same

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 1e-5
KIND = "f16"


@pytest.fixture(scope="module")
def eng8():
    e = make_engine(mode=MODE_INT8, max_ctx=256)
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    return load_oracle()


_REF = {}


def reference(orc, key, make):
    """per case: the data and the oracle's rows, computed once and shared by the row counts (a launch of M rows takes the first M); never modified"""
    if key not in _REF:
        d = make()
        d["cb"], d["scb"] = orc.quantize_rows(d["W"])
        X = d["X"]
        d["lin"] = np.concatenate([orc.linear_int8(X[i:i + 1], d["cb"], d["scb"]) for i in range(X.shape[0])])
        assert np.all(np.isfinite(d["lin"]))
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = d
    return _REF[key]


def check_gemm(r, ks, cfg, codes, cb, what):
    assert (r["ksplit"], r["cfg"]) == (ks, cfg), (what, "tiling as launched (ksplit, cfg)", (r["ksplit"], r["cfg"]), "expected", (ks, cfg))
    want = G.int8_product(codes, cb)
    bad = np.argwhere(r["slab"].astype(np.int64) != want)
    assert bad.size == 0, (what, "the GEMM's slab sum differs from codes . CB^T at", len(bad), "places; first [row, column]", bad[0].tolist(),
                           int(r["slab"][tuple(bad[0])]), int(want[tuple(bad[0])]))


def same_quant(a, b, what):
    for name, x, y in zip(("q", "sca", "oc_cnt", "oc_list", "oc_val"), a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, name)


# ------------------------------------------------------------------------------------------ o_proj / down_proj -> add_rmsnorm
def norm_params():
    for N, K, ks, cfg, forms, Ms in G.I8_NORM_CASES:
        for M in Ms:
            yield pytest.param(N, K, ks, cfg, forms, M, id=f"{N}x{K}-M{M}")


def scan_inputs(X, n):
    """form 1's inputs: the partials of glue_ref.i8_partials; the counts as a producer would leave them, or all of a row's in the last / in the first slot"""
    amax, big = G.i8_partials(X)
    for i in range(X.shape[0]):
        if i % 3 == 1:
            big[i] = [0, 0, 0, n[i]]
        elif i % 3 == 2:
            big[i] = [n[i], 0, 0, 0]
    return amax, big


@pytest.mark.parametrize("N,K,ks,cfg,forms,M", list(norm_params()))
def test_norm_consumer(eng8, orc, N, K, ks, cfg, forms, M):
    """slab8_load / slab8_finish<1, 8> in add_rmsnorm_kernel: listed form and scanning form, tiled and k-major gathers.  K = 2304 runs the slab loop from the ninth
    slab on; the scanning form spills list entries 64 and up into the row's oc_list / oc_val and reads them back"""
    d = reference(orc, ("norm", N, K), lambda: dict(zip(("X", "n", "W", "x", "w"), G.i8_norm_data(N, K))))
    X, n, W, w, lin = d["X"][:M], d["n"][:M], d["W"], d["w"], d["lin"][:M]
    rows_alloc = M + 3
    x_in = np.concatenate([d["x"][:M], poison((3, N), KIND)])
    y_in = poison((rows_alloc, N), KIND, flip=True)
    want_x = np.concatenate([G.residual_add(d["x"][:M], lin, KIND), x_in[M:]])
    codes = G.i8_codes(X)
    amax, big = scan_inputs(X, n)
    assert np.array_equal(G.i8_codes(X, amax.max(axis=1)), codes)            # the maximum of the partials quantises to the same codes
    first = None
    for form in forms:
        for layout in (0, 1):
            what = (f"{N}x{K}", "M", M, "form", form, "layout", layout)
            r = eng8.test_decode_i8_norm(X, W, x_in, w, EPS, form, layout, amax=amax if form else None, big=big if form else None, y_init=y_in, want_slab=True)
            check_gemm(r, ks, cfg, codes, d["cb"], what)
            same(r["x"], want_x, what + ("x_out: residual_add(x, oracle rows); rows behind M as sent",))
            same(r["y"][M:], y_in[M:], what + ("y rows behind M",))
            lo, hi = G.norm_lo_hi(r["x"][:M], w, EPS, KIND)
            ok, share = G.in_pair(r["y"][:M], lo, hi)
            assert share <= G.AMBIGUOUS_CAP[KIND], what + (share,)
            assert ok, what + ("y outside the acceptance set", int(np.sum((bits(r["y"][:M]) != bits(lo)) & (bits(r["y"][:M]) != bits(hi)))))
            check_quant(r["quant"], r["y"][:M], what)
            if first is None:
                first = r
            else:
                same(r["x"], first["x"], what + ("x_out against the first launch",))
                same(r["y"], first["y"], what + ("y against the first launch",))
                same_quant(r["quant"], first["quant"], what + ("quantiser outputs against the first launch",))


def test_norm_consumer_refusals(eng8):
    from sonicscribe_amd.engine import SonicError
    z = lambda *s: np.zeros(s, F)
    ok = dict(X=z(2, 256), W=z(256, 256), x=z(2, 256), norm_w=z(256), eps=EPS, form=0, layout=0)
    eng8.test_decode_i8_norm(**ok)
    for bad in (dict(X=z(2, 320), W=z(256, 320)),                            # K no multiple of 256
                dict(W=z(272, 256), x=z(2, 272), norm_w=z(272)),             # N no multiple of 32
                dict(W=z(4096, 256), x=z(2, 4096), norm_w=z(4096)),          # wider than the norm kernel's block
                dict(X=z(65, 256), x=z(65, 256)),                            # more rows than a token step
                dict(form=1),                                               # the scanning form without its partials
                dict(form=2), dict(layout=2),
                dict(X=z(2, 4096), W=z(256, 4096), form=1, amax=z(2, 4), big=np.zeros((2, 4), np.int32))):     # K > 32 x 64 threads: the scan cannot cover the row
        with pytest.raises(SonicError):
            eng8.test_decode_i8_norm(**dict(ok, **bad))
    e = make_engine(max_batch=1, max_ctx=256)
    try:
        with pytest.raises(SonicError, match="mode int8"):
            e.test_decode_i8_norm(**ok)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ gate/up -> swiglu_quant
def swiglu_params():
    for N, K, ks, cfg, Ms in G.I8_SWIGLU_CASES:
        for M in Ms:
            yield pytest.param(N // 2, K, ks, cfg, M, id=f"{N}x{K}-M{M}")


def swiglu_data(ff, K):
    X, n = G.i8_rows(K, 64 if ff <= 2048 else max(G.I8_LARGE_M), G.I8_SEED + ff + K)
    return dict(X=X, n=n, W=G.interleave16(G.i8_weights(ff, K, G.I8_SEED + 2 * ff + K), G.i8_weights(ff, K, G.I8_SEED + 3 * ff + K)))


@pytest.mark.parametrize("ff,K,ks,cfg,M", list(swiglu_params()))
def test_swiglu_consumer(eng8, orc, ff, K, ks, cfg, M):
    """slab8_load / slab8_finish<2, 2> in swiglu_quant_kernel (K = 768: three slabs, the third through the rolled loop): act = fp16(fp16(silu(g)) * u) on the
    Linear's fp16 outputs, which is glue_ref.swiglu of one fp32 slab holding them"""
    d = reference(orc, ("swiglu", ff, K), lambda: swiglu_data(ff, K))
    X, W, lin = d["X"][:M], d["W"], d["lin"][:M]
    with np.errstate(over="ignore"):                                        # (exp(-g) of a large negative gate: inf, silu = -0)
        want = G.swiglu(lin[None], M, 0, KIND)
    act_in = poison((M + 3, ff), KIND)
    codes = G.i8_codes(X)
    first = None
    for layout in (0, 1):
        what = (f"{2 * ff}x{K}", "M", M, "layout", layout)
        r = eng8.test_decode_i8_swiglu(X, W, layout, act_init=act_in, want_slab=True)
        check_gemm(r, ks, cfg, codes, d["cb"], what)
        same(r["act"], np.concatenate([want, act_in[M:]]), what + ("act; rows behind M as sent",))
        check_quant(r["quant"], r["act"][:M], what)
        if first is None:
            first = r
        else:
            same_quant(r["quant"], first["quant"], what + ("quantiser outputs against the tiled launch",))


# ------------------------------------------------------------------------------------------ q|k|v -> decode attention
def attn_params():
    for Hq, Hkv, D, ks, cfg, Ms in G.I8_ATTN_CASES:
        for B in Ms:
            yield pytest.param(Hq, Hkv, D, ks, cfg, B, id=f"{Hq}-{Hkv}-{D}-B{B}")


AMAX_POISON, BIG_POISON = F(1e4), 12345


@pytest.mark.parametrize("Hq,Hkv,D,ks,cfg,B", list(attn_params()))
def test_attention_consumer(eng8, orc, Hq, Hkv, D, ks, cfg, B):
    """slab1x2_load / slab1x2_finish in decode_attn_kernel's prologue, and the kernel's amax_out / big_out"""
    d = reference(orc, ("attn", Hq, Hkv, D, B), lambda: G.i8_attn_data(Hq, Hkv, D, B))
    X, W, lin, kv_len, cs = d["X"], d["W"], d["lin"], d["kv_len"], d["cs"]
    pos = kv_len - 1
    rows = np.arange(B)
    q, k_new, v_new = R.fused_prologue(lin[None], cs[pos], Hq, Hkv, KIND)
    want_k, want_v = d["kc"].copy(), d["vc"].copy()
    want_k[rows, :, pos] = k_new; want_v[rows, :, pos] = v_new
    for b in range(B):                                                       # the bound's premise for fp16 (attn_ref's docstring), from the reference alone
        for h in range(Hq):
            assert G.f16_subnormal_share(q[b, h], want_k[b, h // (Hq // Hkv)], want_v[b, h // (Hq // Hkv)], int(kv_len[b]), SCALE) <= 0.25
    codes = G.i8_codes(X)
    amax_in = np.full((B, 4), AMAX_POISON, F); big_in = np.full((B, 4), BIG_POISON, np.int32)
    first = None
    for layout in (0, 1):
        what = (f"Hq:Hkv {Hq}:{Hkv} D {D}", "B", B, "layout", layout)
        r = eng8.test_decode_i8_attn(X, W, cs, d["kc"], d["vc"], kv_len, Hq, amax_in, big_in, layout, want_slab=True)
        check_gemm(r, ks, cfg, codes, d["cb"], what)
        ko, vo, out = r["kcache"], r["vcache"], r["out"]
        assert np.array_equal(ko[rows, :, pos], k_new), what + ("appended K rows differ; first [row, kv head, dim]", np.argwhere(ko[rows, :, pos] != k_new)[0].tolist())
        assert np.array_equal(vo[rows, :, pos], v_new), what + ("appended V rows differ; first [row, kv head, dim]", np.argwhere(vo[rows, :, pos] != v_new)[0].tolist())
        assert np.array_equal(ko, want_k) and np.array_equal(vo, want_v), what + ("cache touched outside the appended row", np.argwhere(ko != want_k)[:4].tolist(), np.argwhere(vo != want_v)[:4].tolist())
        worst, where = decode_ratio(out, q, want_k, want_v, kv_len, KIND)
        print(f"int8 decode attention {what}: worst err / (u (A + |o|)) = {worst:.3f} at (row, head, kv_len) {where}")
        assert worst <= R.C_BOUND, what + (worst, where)
        one = np.flatnonzero(kv_len == 1)                                   # one key: its probability is exp(0) = 1, the row sum 1: the output IS the new value row
        assert np.array_equal(out[one], np.repeat(v_new[one], Hq // Hkv, axis=1)), what + ("kv_len 1: out differs from the appended V row",)
        am, bg = G.head_partials(out, Hkv)
        same(r["amax"][:, :Hkv], am, what + ("amax_out: per kv head the absmax of the kernel's own outputs below 6.0 [row, kv head]",))
        assert np.array_equal(r["big"][:, :Hkv], bg), what + ("big_out [row, kv head]", np.argwhere(r["big"][:, :Hkv] != bg)[:4].tolist())
        assert np.all(r["amax"][:, Hkv:] == AMAX_POISON) and np.all(r["big"][:, Hkv:] == BIG_POISON), what + ("partials of kv heads the launch does not have were written",)
        if first is None:
            first = r
            if B >= 5:                                                       # the data does what it is for: heads with and without outputs >= 6.0, partials beside counts
                assert (bg > 0).any() and (bg == 0).any() and ((bg > 0) & (am > 0)).any()
                assert Hkv == 1 or any((bg[b] > 0).any() and (bg[b] == 0).any() for b in range(B))
        else:
            for name in ("out", "kcache", "vcache", "amax"):
                same(r[name], first[name], what + (name, "against the tiled launch"))
            assert np.array_equal(r["big"], first["big"])


def test_swiglu_and_attention_consumer_refusals(eng8):
    from sonicscribe_amd.engine import SonicError
    z = lambda *s: np.zeros(s, F)
    eng8.test_decode_i8_swiglu(z(2, 256), z(64, 256), 0)
    for X, W, layout in ((z(2, 256), z(16400, 256), 0),                      # ff = 8200: wider than swiglu_quant_kernel's block covers
                         (z(2, 256), z(48, 256), 0),                         # ff = 24: no whole 16-column gate / up groups
                         (z(2, 384), z(64, 384), 0),                         # K no multiple of 256
                         (z(65, 256), z(64, 256), 0), (z(2, 256), z(64, 256), 3)):
        with pytest.raises(SonicError):
            eng8.test_decode_i8_swiglu(X, W, layout)

    def attn(B=2, D=256, Hq=2, Hkv=1, ctx=8, kv_len=None, layout=0):
        p = np.full((B, 4), 1.0, F)
        return eng8.test_decode_i8_attn(z(B, D), z((Hq + 2 * Hkv) * 128, D), G.rope_table(ctx), z(B, Hkv, ctx, 128), z(B, Hkv, ctx, 128),
                                        [1] * B if kv_len is None else kv_len, Hq, p, p.astype(np.int32), layout)
    attn()
    for bad in (dict(kv_len=[0, 1]), dict(kv_len=[1, 9]),                   # outside 1 .. ctx_max
                dict(Hq=5), dict(Hq=8),                                      # no whole GQA group; more than four q heads per kv head
                dict(Hq=8, Hkv=8),                                           # more kv heads than the partials have slots
                dict(D=384), dict(B=65), dict(layout=-1)):
        with pytest.raises(SonicError):
            attn(**bad)
