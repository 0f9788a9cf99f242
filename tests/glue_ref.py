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


# ------------------------------------------------------------------------------------------ the int8 token step: a decode-flavour Linear8bitLt and its consumers
# (tests/test_gpu_int8_decode_glue.py).  The Linear's spec is oracle.linear_int8(x_row[None], *oracle.quantize_rows(W)), one row per call; what is restated here is the
# exact integer product the skinny GEMM must deliver, and the data.
F16_BELOW_6 = F(5.99609375)              # the largest fp16 value below the threshold: not an outlier
I8_COUNTS = [65, 0, 3, 129, -1, 1, 2, 4, 5, 7, 63, 64, 66]      # outliers of row i: I8_COUNTS[i % 13]; -1: every element of the row
I8_FIRST = (0, -1, 63, 64)               # where a row's first outliers go: column 0, column K - 1, both sides of a 64-column tile boundary of the tiled weights


def int8_product(codes, cb):
    """codes [M][K] int8 (quant_row's), cb [N][K] int8 -> codes . cb^T as int64 [M][N].  Computed by the float64 BLAS: every partial sum is an integer of
    magnitude <= K 127^2 < 2^53, so each float64 operation is exact and the result is the int64 product in any order"""
    codes = np.asarray(codes); cb = np.asarray(cb)
    assert codes.dtype == np.int8 and cb.dtype == np.int8 and codes.shape[1] == cb.shape[1] and codes.shape[1] * 127 * 127 < 2 ** 53
    p = codes.astype(np.float64) @ cb.astype(np.float64).T
    return p.astype(np.int64)


def i8_dequant(acc, sca, scb):
    """the Linear's output for a row WITHOUT outliers from its integer product (oracle/sonic_oracle.c linear_int8): fp16(fma(float(acc), (sca scb) C, 0)) with fp32
    products in that order.  acc [N] int, sca fp32, scb [N] fp32.  float(acc) scale is rounded once by the fma: computed in float64 (exact: 24 x 24 bits) and rounded"""
    sc = ((F(sca) * np.asarray(scb, F)).astype(F) * F(6.200012e-05)).astype(F)
    return rounder("f16")((np.asarray(acc).astype(F).astype(np.float64) * sc.astype(np.float64)).astype(F))


def i8_rows(K, M, seed):
    """M hidden rows of width K, fp16 values: N(0, 1.5) kept below the threshold (|x| <= 5.9), with I8_COUNTS[i % 13] planted outliers in row i - the first four at
    I8_FIRST, the others anywhere, ascending lists of every length around the consumers' pair / quad walks and the 64-entry LDS stage.  Outliers are a random sign
    times U(6.5, 12), except that a row's outlier at column 0 is exactly +6.0 or -6.0 (alternating by row); row i gets +-5.99609375 at column 1 of its
    quarter i % 4 unless an outlier sits there.  -> (X [M][K], n [M] the rows' outlier counts)"""
    rng = np.random.default_rng(seed)
    rt = rounder("f16")
    X = rt(np.clip(rng.standard_normal((M, K)) * 1.5, -5.9, 5.9))
    n_out = np.zeros(M, np.int64)
    for i in range(M):
        n = I8_COUNTS[i % len(I8_COUNTS)]
        n = K if n < 0 else min(n, K)
        first = [c % K for c in I8_FIRST][:n]
        rest = np.setdiff1d(np.arange(K), first)
        cols = np.concatenate([first, rng.choice(rest, size=n - len(first), replace=False)]).astype(np.int64) if n else np.zeros(0, np.int64)
        X[i, cols] = rt(rng.choice([-1.0, 1.0], size=n) * rng.uniform(6.5, 12.0, size=n))
        if n:
            X[i, 0] = 6.0 if i % 2 == 0 else -6.0
        c6 = (i % 4) * (K // 4) + 1                                   # (the row's absmax below the threshold: in a different quarter of the row from row to row)
        if n < K and c6 not in cols:
            X[i, c6] = F16_BELOW_6 if i % 8 < 4 else -F16_BELOW_6
        n_out[i] = n
    return X.astype(F), n_out


def i8_weights(N, K, seed, row_scale=None):
    """W [N][K]: N(0, 0.05) rounded to fp16; row_scale [N] (optional) multiplies the rows first"""
    w = np.random.default_rng(seed).standard_normal((N, K)) * 0.05
    if row_scale is not None:
        w = w * np.asarray(row_scale, np.float64)[:, None]
    return rounder("f16")(w).astype(F)


def i8_partials(X, parts=4):
    """what a producer that owns a quarter of each row leaves for the on-the-fly form: per quarter the absmax over |x| < 6 (0 where there is none) and the count of
    the other elements -> (amax [M][4] fp32, big [M][4] int32).  The row's scale is the maximum of its four partials"""
    X = np.asarray(X, F)
    M, K = X.shape
    q = np.abs(X).reshape(M, parts, K // parts)
    small = q < THRESHOLD
    return np.where(small, q, F(0)).max(axis=2).astype(F), (~small).sum(axis=2).astype(np.int32)


def i8_codes(X, sca=None):
    """the rows' int8 codes: quant_row's; with sca [M] given, the codes for that scale instead of the row's own (the on-the-fly form quantises with the maximum of
    the partials, which is 0 where quant_row says -FLT_MIN: both give all-zero codes)"""
    X = np.asarray(X, F)
    out = np.zeros(X.shape, np.int8)
    for i, y in enumerate(X):
        codes, a, _, _ = quant_row(y)
        if sca is not None:
            assert (F(sca[i]) == a) or (not a > 0 and not F(sca[i]) > 0), (i, float(sca[i]), float(a))
        out[i] = codes
    return out


def head_partials(out, Hkv):
    """the decode attention's amax_out / big_out from its own output rows out [B][Hq][128]: per kv head h the maximum over that head's G * 128 outputs of
    (|o| if |o| < 6 else 0), and the number of outputs with not |o| < 6 -> (amax [B][Hkv] fp32, big [B][Hkv] int32)"""
    o = np.abs(np.asarray(out, F))
    B = o.shape[0]
    o = o.reshape(B, Hkv, -1)
    with np.errstate(invalid="ignore"):
        small = o < THRESHOLD
    return np.where(small, o, F(0)).max(axis=2).astype(F), (~small).sum(axis=2).astype(np.int32)


# the cases of tests/test_gpu_int8_decode_glue.py: (N, K, ksplit, cfg, forms, rows); tests/test_glue_ref.py checks the ambiguity cap for the norm cases
I8_SMALL_M = (1, 5, 16, 17, 33, 64)
I8_LARGE_M = (5, 33)
I8_NORM_CASES = [(256, 256, 1, 4, (0, 1), I8_SMALL_M), (256, 2304, 9, 4, (0,), I8_SMALL_M), (256, 1024, 2, 3, (0, 1), I8_SMALL_M),
                 (2048, 2048, 4, 3, (0, 1), I8_LARGE_M), (2048, 6144, 8, 2, (0, 1), I8_LARGE_M)]
I8_SWIGLU_CASES = [(1024, 768, 3, 4, I8_SMALL_M), (9216, 2048, 2, 1, I8_LARGE_M)]          # N = 2 ff
I8_SEED = 8192


def i8_norm_data(N, K, seed=I8_SEED):
    """the 64 master rows of a norm case (a launch of M rows takes the first M): X, outlier counts, W, residual rows N(0, 1) with three rows of +-1e4 behind them,
    norm weight in [0.5, 1.5]"""
    X, n = i8_rows(K, 64, seed + N + K)
    W = i8_weights(N, K, seed + 7 * N + K)
    rng = np.random.default_rng(seed + N + 3 * K)
    x = rounder("f16")(rng.standard_normal((64, N))).astype(F)
    return X, n, W, x, rng.uniform(0.5, 1.5, size=N).astype(F)


I8_ATTN_CTX = 200
# (Hq, Hkv, D, ksplit, cfg, rows): TINY's q|k|v (512 x 256), production's (3072 x 2048), and 512 x 2304: nine slabs, the prologue's slab loop from the ninth on
I8_ATTN_CASES = [(2, 1, 256, 1, 4, I8_SMALL_M), (16, 4, 2048, 2, 0, I8_LARGE_M), (2, 1, 2304, 9, 4, I8_LARGE_M)]
I8_ATTN_LENS = (I8_ATTN_CTX - 1, 128, 1, 17, 129, 64, 2, 100)
V_LOUD = 6.5                             # factor of a loud (row, kv head)'s cached value rows


def i8_attn_data(Hq, Hkv, D, B, seed=I8_SEED, ctx=I8_ATTN_CTX):
    """The int8 attention hook's inputs for B rows (the first B of 64 master rows).
    Hidden rows: i8_rows.  Wqkv: N(0, 0.05) with rows scaled so that q, k and v come out of an outlier-free row with a standard deviation of about 1.2 whatever D is
    (1.5 x 0.05 x sqrt(D) is 1.2 at D = 256 and 3.4 at 2048: scores of q . k / sqrt(128) with both at 3.4 put most rows under one dominating key, where fp16
    probabilities leave the normal range that attn_ref's bound presumes), the v rows of the even kv heads three times that (so that new value rows pass 6.0 there).
    kv_len: 1 for the rows with 63 outliers or more (their q and k are large, see above; with one key the output is the new value row itself), else I8_ATTN_LENS in turn.
    Caches: keys N(0, 1), values attn_ref.values (fp16: away from zero), +-1e4 from position kv_len - 1 on; the values of (row b, kv head h) with (b + h) even are
    'loud': V_LOUD |v| with one sign per column, so that the outputs there land on both sides of 6.0, while the other heads of the row stay far below it.
    -> dict X, n, W, kc, vc, kv_len, cs"""
    from attn_ref import values
    rt = rounder("f16")
    X, n = i8_rows(D, 64, seed + D + Hq)
    X, n = X[:B], n[:B]
    base = 1.2 / (1.5 * 0.05 * np.sqrt(D))
    scale = np.full((Hq + 2 * Hkv, 128), base)
    scale[Hq + Hkv::2] *= 3.0
    W = i8_weights((Hq + 2 * Hkv) * 128, D, seed + 11 * D + Hq, scale.reshape(-1))
    rng = np.random.default_rng(seed + 5 * D + B)
    kv_len = np.zeros(B, np.int32)
    j = 0
    for b in range(B):
        if n[b] >= 63:
            kv_len[b] = 1
        else:
            kv_len[b] = I8_ATTN_LENS[j % len(I8_ATTN_LENS)]; j += 1
    pois = rt(np.where(np.arange(B * Hkv * ctx * 128) % 2 == 0, 1e4, -1e4).astype(F)).reshape(B, Hkv, ctx, 128)
    kc, vc = pois.copy(), -pois
    sgn = rng.choice([-1.0, 1.0], size=128)
    for b in range(B):
        m = int(kv_len[b]) - 1
        kc[b, :, :m] = rt(rng.standard_normal((Hkv, m, 128))); vc[b, :, :m] = values(rng, (Hkv, m, 128), "f16")
        for h in range(Hkv):
            if (b + h) % 2 == 0:
                vc[b, h, :m] = rt(np.abs(vc[b, h, :m]) * sgn[None, :] * V_LOUD)
    return dict(X=X, n=n, W=W, kc=kc.astype(F), vc=vc.astype(F), kv_len=kv_len, cs=rope_table(ctx))


def f16_subnormal_share(q, k, v, n, scale):
    """The premise of attn_ref's bound for fp16, checked on the reference alone: a probability below 2^-14 of the row's largest is rounded with an ABSOLUTE error of up
    to 2^-25, which the bound u (A + |o|) does not know.  q [hd], k / v [n][hd] -> max over the output elements of (2^-25 x sum of |v_i| over those keys) /
    (u (A + |o|)): the share of the c = 1 bound that term can take (0 where no key is that far down)"""
    q = np.asarray(q, np.float64); k = np.asarray(k, np.float64)[:n]; v = np.asarray(v, np.float64)[:n]
    s = (k @ q) * scale
    e = np.exp(s - s.max())
    p = e / e.sum()
    o = p @ v; A = p @ np.abs(v)
    extra = 2.0 ** -25 * np.abs(v[e < 2.0 ** -14]).sum(axis=0)
    b = 2.0 ** -11 * (A + np.abs(o))
    return float(np.max(np.where(extra > 0, extra / np.where(b > 0, b, 1e-300), 0.0)))
