"""Plain numpy references for the decode-step and prefill glue kernels (tests/test_gpu_decode_glue.py, checked itself by tests/test_glue_ref.py).

Every function restates ONE kernel's arithmetic at its rounding points: fp32 operations, and rt = rounder(kind) wherever the kernel converts to its element
type (bf16 or fp16).  Single fp32 multiplications, additions, divisions and square roots are correctly rounded on both sides (the build has no fast-math),
so wherever the ORDER of the operations is fixed by the kernel the result can be compared bit for bit.

What is not reproducible is the fp32 sum of squares behind an RMSNorm scale: its association differs per kernel.
  * add_rmsnorm_kernel: 8 fused multiply-adds per thread, 6 levels of the wave butterfly, at most 4 wave partials, then the division by d (+ eps), the
    square root and the reciprocal: 8 + 6 + 4 + 3 = 21 roundings on the path.
  * skinny_o_kernel + rmsnorm_ss_kernel / skinny_gu_kernel<NORM>: 16 squares of a block's columns added in sequence, then up to 16 groups x 4 block partials per
    lane half in sequence, one add of the halves, and the same three closing operations: at most 16 + 64 + 1 + 3 = 84 roundings.
  All terms of the sum are >= 0, so n roundings move the total by at most n 2^-24 relatively, and r = total^(-1/2) by half of that; the three closing
  operations add at most 2.5 x 2^-24 (the root halves the division's error).  Worst path: (81 / 2 + 2.5) 2^-24 = 43 x 2^-24 < 2^-18.
  So the scale a kernel uses lies within r64 (1 -+ 2^-18) (R_MARGIN) of the exact one.  norm_lo_hi() pushes both ends of that interval through the kernel's
  two roundings per element; x r is monotone in r and so is every rounding, and 2^-18 is far below one element-type step, so rt(x r) takes one of two
  ADJACENT values and every element of a correct kernel's y equals y_lo or y_hi - bit for bit wherever the two agree.  The share of elements where they
  differ is a property of the inputs (about 2^-9 of N(0, 1) rows in bf16, 2^-6 in fp16); AMBIGUOUS_CAP bounds it so that a test cannot pass by declaring
  everything ambiguous (tests/test_glue_ref.py checks the caps for the seeds the GPU tests use).

skinny_o_kernel on random data: the o_proj sum v itself comes out of the MFMA pipeline in an order this file does not restate.  The random o_proj data is
therefore drawn WITHOUT cancellation (att >= 0, Wo > 0: a relative margin cannot be derived for a sum that cancels).  The products of two element-type
values are exact in fp32 (16 or 22 significant bits).  An output element is the sum of K <= 2048 of them: per wave K / 256 <= 8 chained MFMA steps of 32
products each, then 8 wave partials added in sequence.  Allowing 8 roundings inside every MFMA step (the hardware does fewer) that is 8 x 8 + 8 = 72
roundings of non-negative partial sums: |v - v64| <= 72 x 2^-24 v64 < 2^-17 v64 (V_MARGIN).  resid_out must equal rt(x + rt(v64 (1 - 2^-17))) or
rt(x + rt(v64 (1 + 2^-17))) (o_resid_lo_hi), the same two-adjacent-values argument, under the same share cap.
"""
import numpy as np

from attn_ref import rounder, rope_table  # noqa: F401  (rope_table: re-exported for the tests)

F = np.float32
R_MARGIN = 2.0 ** -18
V_MARGIN = 2.0 ** -17
AMBIGUOUS_CAP = {"bf16": 0.01, "f16": 0.05}
THRESHOLD = F(6.0)                       # LLM.int8 outlier threshold
FLT_MIN = F(1.17549435e-38)
OUTL_CAP = 64                            # pairs a consumer stages in LDS (int8_util.h): the producer's list is not capped


# ------------------------------------------------------------------------------------------ RMSNorm family
def slab_sum(slabs):
    """[ksplit][rows][n] fp32 -> [rows][n]: from 0.f, ascending ks"""
    slabs = np.asarray(slabs, F)
    acc = np.zeros(slabs.shape[1:], F)
    for ks in range(slabs.shape[0]):
        acc = (acc + slabs[ks]).astype(F)
    return acc


def residual_add(x, v, kind):
    """x' = rt(x + rt(v)): the epilogue of add_rmsnorm_kernel (v = slab sum) and of skinny_o_kernel (v = the o_proj sum)"""
    rt = rounder(kind)
    return rt((np.asarray(x, F) + rt(np.asarray(v, F))).astype(F))


def scale32(tot, d, eps):
    """r = 1 / sqrt(tot / d + eps) with the kernels' three fp32 operations; tot [rows] fp32"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (F(1.0) / np.sqrt((np.asarray(tot, F) / F(d) + F(eps)).astype(F)).astype(F)).astype(F)


def norm_apply(xn, w, r, kind):
    """y = rt(w * rt(x' * r)); xn [rows][d], w [d] fp32, r [rows] fp32"""
    rt = rounder(kind)
    with np.errstate(invalid="ignore"):
        return rt((np.asarray(w, F)[None, :] * rt((np.asarray(xn, F) * np.asarray(r, F)[:, None]).astype(F))).astype(F))


def sumsq_exact(xn):
    """row sums of squares in float64 (exact for the integer constructions: every partial sum stays below 2^24)"""
    return (np.asarray(xn, np.float64) ** 2).sum(axis=1)


def add_rmsnorm(x, slabs, w, eps, kind):
    """add_rmsnorm_kernel with an exactly known sum of squares (integer data): -> (x' [rows][d], y [rows][d])"""
    xn = residual_add(x, slab_sum(slabs), kind)
    tot = sumsq_exact(xn)
    assert np.all(tot[np.isfinite(tot)] < 2.0 ** 24)
    return xn, norm_apply(xn, w, scale32(tot.astype(F), xn.shape[1], eps), kind)


def norm_lo_hi(xn, w, eps, kind):
    """the two admissible outputs of an RMSNorm kernel for rows xn (module docstring): r64 (1 -+ 2^-18) through the kernel's roundings -> (y_lo, y_hi)"""
    xn = np.asarray(xn, F)
    r64 = 1.0 / np.sqrt(sumsq_exact(xn) / xn.shape[1] + float(F(eps)))
    return norm_apply(xn, w, (r64 * (1.0 - R_MARGIN)).astype(F), kind), norm_apply(xn, w, (r64 * (1.0 + R_MARGIN)).astype(F), kind)


def o_resid_lo_hi(att, Wo, x, kind):
    """skinny_o_kernel on data without cancellation: the two admissible residual rows (module docstring) -> (lo, hi)"""
    att = np.asarray(att, np.float64); Wo = np.asarray(Wo, np.float64)
    assert att.min() >= 0 and Wo.min() > 0
    v64 = att @ Wo.T
    return residual_add(x, (v64 * (1.0 - V_MARGIN)).astype(F), kind), residual_add(x, (v64 * (1.0 + V_MARGIN)).astype(F), kind)


def in_pair(got, lo, hi):
    """(every element equals lo or hi - bit for bit -, share of elements where lo and hi differ)"""
    g, a, b = (np.ascontiguousarray(t, F).view(np.uint32) for t in (got, lo, hi))
    return bool(np.all((g == a) | (g == b))), float(np.mean(a != b))


# ------------------------------------------------------------------------------------------ SwiGLU of the gate/up slabs
def swiglu_maps(ff, gu8):
    """column of the gate and of the up value of output column c in the interleaved projection [2 ff]: groups of 16 (gu8 = 0, EPI_SWIGLU's layout) or 8"""
    c = np.arange(ff)
    g = (c >> 3) * 16 + (c & 7) if gu8 else (c >> 4) * 32 + (c & 15)
    return g, g + (8 if gu8 else 16)


def swiglu(slabs, rows, gu8, kind):
    """swiglu_slab_kernel: act = rt(rt(silu(rt(g))) * rt(u)), g / u the slab sums; slabs [ksplit][mpad][2 ff] -> [rows][ff]"""
    rt = rounder(kind)
    p = slab_sum(np.asarray(slabs, F)[:, :rows])
    gi, ui = swiglu_maps(p.shape[1] // 2, gu8)
    g = rt(p[:, gi]); u = rt(p[:, ui])
    s = rt((g / (F(1.0) + np.exp(-g).astype(F))).astype(F))
    return rt((s * u).astype(F))


# ------------------------------------------------------------------------------------------ row quantiser (quant_emit_row)
def quant_row(y):
    """One row of fp16 values -> (codes int8 [K], sca fp32, outlier columns ascending, their values).  amax = the row's absmax over |y| < 6 starting from
    -FLT_MIN (what sca receives when nothing is below the threshold, as in oracle/sonic_oracle.c linear_int8); codes rint(y * (127 / amax)) in fp32, 0 for
    outliers and for the whole row when !(amax > 0); outliers are the elements with !(|y| < 6): 6.0 itself and NaN count."""
    y = np.asarray(y, F)
    with np.errstate(invalid="ignore"):
        small = np.abs(y) < THRESHOLD
    amax = F(max(-FLT_MIN, np.abs(y[small]).max())) if small.any() else -FLT_MIN
    codes = np.zeros(y.shape, np.int8)
    if amax > 0:
        scale = F(127.0) / amax
        codes[small] = np.rint((y[small] * scale).astype(F)).astype(np.int8)
    cols = np.flatnonzero(~small).astype(np.int32)
    return codes, F(amax), cols, y[cols]


# ------------------------------------------------------------------------------------------ rotate-half RoPE
def rope(x, cs, rd, kind):
    """x [..., hd] element-type values, cs [..., rd] fp32 (cos[0 .. rd/2) | sin[0 .. rd/2), broadcast against x): the first rd dims are rotated in pairs
    (i, i + rd/2) with every product and the sum rounded - first half rt(rt(x1 c) + rt(-x2 s)), second half rt(rt(x2 c) + rt(x1 s)) -, the rest passes through.
    rd = 128 = hd: the decoder (rope_append kernels); rd <= hd = 64: the encoder (rope_enc_kernel)."""
    rt = rounder(kind)
    x = np.asarray(x, F); cs = np.asarray(cs, F)
    h = rd // 2
    x1, x2, c, s = x[..., :h], x[..., h:rd], cs[..., :h], cs[..., h:rd]
    out = x.copy()
    out[..., :h] = rt((rt((x1 * c).astype(F)) + rt((-x2 * s).astype(F))).astype(F))
    out[..., h:rd] = rt((rt((x2 * c).astype(F)) + rt((x1 * s).astype(F))).astype(F))
    return out


# ------------------------------------------------------------------------------------------ data of the GPU tests (shared with tests/test_glue_ref.py)
def o_chain_exact(M, K, D, rows_alloc, seed):
    """integer data for the o_proj chain: att in [-2, 2], Wo[n] = +1 at n mod K and -1 at (7 n + 3) mod K (asymmetric: a wrong lane / k map shows), resid in
    [-8, 8] with a +-1e4 sentinel in the rows behind M.  v = att Wo^T is an integer in [-4, 4], x' = resid + v in [-12, 12]: exact in both types, in any order."""
    rng = np.random.default_rng(seed)
    att = rng.integers(-2, 3, size=(M, K)).astype(F)
    n = np.arange(D)
    Wo = np.zeros((D, K), F)
    Wo[n, n % K] += 1.0; Wo[n, (7 * n + 3) % K] -= 1.0
    resid = np.empty((rows_alloc, D), F)
    resid[:M] = rng.integers(-8, 9, size=(M, D))
    resid[M:] = np.where((np.arange((rows_alloc - M) * D) % 2) == 0, 1e4, -1e4).reshape(rows_alloc - M, D)
    return att, Wo, resid


def split_ints(rng, total, ksplit, spread=50):
    """integer array `total` as ksplit uneven integer slabs [ksplit][...] that sum to it exactly in any order (all partial sums far below 2^24)"""
    parts = rng.integers(-spread, spread + 1, size=(ksplit,) + total.shape).astype(F)
    parts[-1] = total - parts[:-1].sum(axis=0)
    return parts


U_EXP = {"bf16": (-60, 128), "f16": (-12, 22)}          # (lowest exponent, how many) of the power-of-two part of u
U_MANT = [37, 41, 43, 47, 53, 59]                       # primes above every g: g m = g' m' only for (g, m) = (g', m')


def swiglu_exact(ff, rows, ksplit, gu8, kind, seed):
    """Slabs whose SwiGLU is exact and different in every output column of a row: g = 16 + (c mod 16) (silu(g) rounds to g in both types: exp(-16) < u / 2),
    u = sign(row) m 2^e with (m, e) encoding c // 16 - a power of two times a 6-bit prime mantissa, so g u has at most 11 significant bits (bf16: m = 1, the
    exponent range alone covers ff / 16 = 128 groups).  g is split into integer slabs, u into u/2 + u/4 + ... (exact).  -> (slabs [ksplit][mpad][2 ff], expected)"""
    rng = np.random.default_rng(seed)
    c = np.arange(ff)
    grp = c // 16
    e0, ne = U_EXP[kind]
    assert ff // 16 <= ne * (1 if kind == "bf16" else len(U_MANT))
    mant = np.ones(ff) if kind == "bf16" else np.asarray(U_MANT, np.float64)[grp // ne] / 32.0
    u = (mant * 2.0 ** (e0 + grp % ne)).astype(F)
    g = (16 + (c % 16)).astype(F)
    sign = np.where(np.arange(rows) % 2 == 0, 1.0, -1.0).astype(F)[:, None]
    G = np.broadcast_to(g, (rows, ff)).copy(); Uu = (sign * u[None, :]).astype(F)
    mpad = (rows + 15) // 16 * 16 + 16
    slabs = np.full((ksplit, mpad, 2 * ff), 1e4, F)                    # rows no request owns: a mis-indexed row shows
    gi, ui = swiglu_maps(ff, gu8)
    gs = split_ints(rng, G, ksplit)
    w = np.asarray([0.5 ** (k + 1) for k in range(ksplit)]); w[-1] *= 2.0   # 1/2, 1/4, .., 1/2^(n-1), 1/2^(n-1): sums to 1
    if ksplit == 1:
        w = np.asarray([1.0])
    for ks in range(ksplit):
        slabs[ks, :rows, gi] = gs[ks].T
        slabs[ks, :rows, ui] = (Uu * F(w[ks])).T
    return slabs, (G * Uu).astype(F)


OUTLIER_COLS = (0, 7, 8, 511, 512)                       # + K - 1: both sides of a thread's 8 elements and of a wave's 512


def quant_rows_data(K, seed):
    """fp16 rows for the row quantiser, in this order: no outlier; outliers at columns 0, 7, 8, 511, 512, K - 1; exactly 6.0 / -6.0 (outliers) and 5.996 (the
    largest fp16 below 6: not one); more outliers than OUTL_CAP (70; K - 4 where the row is shorter) spread over the row; all zero; all outliers; one NaN"""
    rng = np.random.default_rng(seed)
    rt = rounder("f16")
    base = lambda: rt(np.clip(rng.standard_normal(K) * 1.5, -5.9, 5.9))
    big = lambda n: rt(rng.choice([-1.0, 1.0], size=n) * rng.uniform(6.5, 30.0, size=n))
    rows = [base()]
    r = base(); cols = [c for c in OUTLIER_COLS if c < K - 1] + [K - 1]; r[cols] = big(len(cols)); rows.append(r)
    r = base(); r[3] = 6.0; r[K // 2] = -6.0; r[K // 2 + 1] = 5.99609375; rows.append(r)
    r = base(); n = min(70, K - 4); cols = np.sort(rng.choice(K, size=n, replace=False)); r[cols] = big(n); rows.append(r)
    rows.append(np.zeros(K, F))
    rows.append(big(K))
    r = base(); r[K // 3] = np.nan; rows.append(r)
    return np.stack(rows).astype(F)


def norm_quant_data(d, seed):
    """Integer rows x' (to be delivered as x = 0 plus slabs), a norm weight and eps for add_rmsnorm + QuantOut on an fp16 engine, so that the normalised rows are,
    in this order: no outlier; outliers at the OUTLIER_COLS and d - 1; exactly +-6.0 and 5.996; 70 outliers; all zero.  w is 2 except 6 at those columns and 5.996
    at column 100; eps = 2^-24 leaves mean(x^2) = 4 as it is, so the all-+-2 row is scaled by exactly 1/2, and gives the zero row the finite scale 2^12."""
    rng = np.random.default_rng(seed)
    sp = [c for c in OUTLIER_COLS] + [d - 1]
    w = np.full(d, 2.0, F); w[sp] = 6.0; w[100] = 5.99609375
    sg = lambda: rng.choice([-1.0, 1.0], size=d)
    r0 = sg(); r0[sp] = 0; r0[100] = 0
    r1 = 2 * sg(); r1[sp] *= 2
    r2 = 2 * sg()
    r3 = 2 * sg(); cols = rng.choice(d, size=70, replace=False); r3[cols] *= 32
    return np.stack([r0, r1, r2, r3, np.zeros(d)]).astype(F), w, 2.0 ** -24


def norm_random(rows, d, ksplit, kind, seed):
    """N(0, 1) residual rows, slabs whose sum is N(0, 1) and a norm weight in [0.5, 1.5] -> (x, slabs [ksplit][rows][d], w)"""
    rng = np.random.default_rng(seed)
    x = rounder(kind)(rng.standard_normal((rows, d)))
    slabs = (rng.standard_normal((ksplit, rows, d)) / np.sqrt(ksplit)).astype(F)
    return x, slabs, rng.uniform(0.5, 1.5, size=d).astype(F)


def o_random(M, K, D, ff, kind, seed):
    """random o_proj chain data without cancellation in the o_proj sum (module docstring): att = |N(0, 1)|, Wo in [2^-11, 2^-9] (so v ~ 1), resid N(0, 1),
    norm weight in [0.5, 1.5], gate / up weights 0.05 N(0, 1) -> (att, Wo, resid, ln_w, Wg, Wu)"""
    rng = np.random.default_rng(seed)
    rt = rounder(kind)
    att = rt(np.abs(rng.standard_normal((M, K)))); Wo = rt(rng.uniform(0.25, 1.0, size=(D, K)) * 2.0 ** -9)
    resid = rt(rng.standard_normal((M, D)))
    w = rng.uniform(0.5, 1.5, size=D).astype(F)
    return att, Wo, resid, w, rt(rng.standard_normal((ff, D)) * 0.05), rt(rng.standard_normal((ff, D)) * 0.05)


def interleave16(Wg, Wu):
    """gate / up rows interleaved in groups of 16 (the layout of the prefill GEMM's SwiGLU epilogue; the hooks tile it on the device)"""
    ff, K = Wg.shape
    Wi = np.empty((2 * ff, K), F)
    Wi.reshape(ff // 16, 2, 16, K)[:, 0] = Wg.reshape(ff // 16, 16, K); Wi.reshape(ff // 16, 2, 16, K)[:, 1] = Wu.reshape(ff // 16, 16, K)
    return Wi


# the random cases of tests/test_gpu_decode_glue.py (tests/test_glue_ref.py checks the ambiguity caps for exactly these)
NORM_RANDOM_CASES = [(3, 264, 3), (17, 2048, 8), (64, 2048, 1)]            # (rows, d, ksplit)
O_RANDOM_CASES = [(5, 256, 256, 2048), (64, 2048, 2048, 2048)]            # (M, K, D, ff)
NORM_SEED, O_SEED = 2048, 4096
