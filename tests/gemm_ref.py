"""Plain numpy references for the MFMA GEMM family in its production launch forms (tests/test_gpu_gemm_forms.py, checked itself by tests/test_gemm_ref.py).

Every function is float64 arithmetic with rt = rounder(kind) wherever the kernels convert to their element type (bf16 or fp16; csrc/gemm.hip, csrc/gemm256.hip,
gemm_lin in csrc/int8_util.h).  A float64 value reaches the element type through float32, as the kernels' fp32 accumulators do.

  linear      x W^T + b, unrounded (float64)                      the accumulator plus the bias
  EPI_BIAS    rt(linear)
  EPI_GELU    rt(gelu(rt(linear))), erf form
  EPI_RESID   rt(rt(linear) + R)
  EPI_SWIGLU  rt(rt(silu(rt(g))) * rt(u)), gate / up columns interleaved in groups of 16 (or 8) columns of the projection
  conv1d      an explicit sliding window, pad 1, stride 1 or 2    the conv stem, which the engine runs as a batched GEMM over overlapping rows of a padded buffer
  q|k|v       columns < n_split row-major, the rest transposed per segment of seg_T rows
  fused RoPE  heads of 64 columns, the first 32 rotated in pairs (i, i + 16): rt(rt(x1 c) + rt(-x2 s)), rt(rt(x2 c) + rt(x1 s)) on the unrounded linear

What the references do not restate is the order of the fp32 accumulation; the bounds (ulp_tol, rope_bound) are the project's: 2 ulp for a plain product, 3 for GELU
and the residual add, 4 ulp + 1e-3 where two roundings follow the linear (SwiGLU's product, the rotation's sum)."""
import numpy as np

from attn_ref import rounder
from glue_ref import swiglu_maps

F = np.float32
ULP = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}          # one unit in the last place of a value in [1, 2)


def ulp_tol(ref, n_ulp, kind):
    """n_ulp units in the last place of |ref| (relative, floored at |ref| = 1e-2): test_gpu_parity.ulp_tol with the element type's ulp"""
    return n_ulp * np.maximum(np.abs(ref), 1e-2) * ULP[kind]


def to_kind(x64, kind):
    """float64 -> the element type, through float32 (the accumulator's type)"""
    return rounder(kind)(np.asarray(x64, np.float64).astype(F))


def linear(A, W, bias=None):
    """A [M][K], W [N][K], bias [N] or None -> float64 [M][N], unrounded"""
    out = np.asarray(A, np.float64) @ np.asarray(W, np.float64).T
    return out if bias is None else out + np.asarray(bias, np.float64)


def erf64(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


def gelu(l, kind):
    """l: the rounded linear (element-type values) -> rt(0.5 l (1 + erf(l / sqrt 2)))"""
    l = np.asarray(l, np.float64)
    return to_kind(0.5 * l * (1.0 + erf64(l / np.sqrt(2.0))), kind)


def resid(l, R, kind):
    """l: the rounded linear, R: the residual (element-type values) -> (rt(l + R), |l| + |R|: the magnitude the bound follows, since the add can cancel)"""
    l = np.asarray(l, np.float64); R = np.asarray(R, np.float64)
    return to_kind(l + R, kind), np.abs(l) + np.abs(R)


def interleave(Wg, Wu, group=16):
    """gate rows Wg [ff][K] and up rows Wu [ff][K] -> the projection [2 ff][K] interleaved in groups of `group` rows (16: EPI_SWIGLU's layout and the source of
    launch_tile_weights_gu8; 8: the order inside that tiled copy)"""
    ff, K = Wg.shape
    assert Wu.shape == Wg.shape and ff % group == 0
    out = np.empty((2 * ff, K), F)
    o = out.reshape(ff // group, 2, group, K)
    o[:, 0] = np.asarray(Wg, F).reshape(ff // group, group, K); o[:, 1] = np.asarray(Wu, F).reshape(ff // group, group, K)
    return out


def swiglu(l, kind, gu8=False):
    """l: the rounded linear of the interleaved projection [M][2 ff] (groups of 16 columns, or 8 with gu8) -> rt(rt(silu(g)) * u) [M][ff]"""
    l = np.asarray(l, np.float64)
    gi, ui = swiglu_maps(l.shape[1] // 2, gu8)
    g, u = l[:, gi], l[:, ui]
    s = to_kind(g / (1.0 + np.exp(-g)), kind).astype(np.float64)
    return to_kind(s * u, kind)


# ------------------------------------------------------------------------------------------ conv stem
def conv1d(x, w, b, stride):
    """x [T][Ci], w [Co][Ci][3] (torch's Conv1d weight), b [Co], pad 1, stride 1 or 2 -> float64 [T_out][Co], T_out = (T + 2 - 3) // stride + 1: the window of output t
    is the input rows stride * t - 1 .. stride * t + 1, rows outside [0, T) read as zero"""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    T, Ci = x.shape
    assert w.shape[1:] == (Ci, 3) and stride in (1, 2)
    T_out = (T - 1) // stride + 1
    out = np.tile(np.asarray(b, np.float64), (T_out, 1))
    for tap in range(3):
        for t in range(T_out):
            r = stride * t - 1 + tap
            if 0 <= r < T:
                out[t] += w[:, :, tap] @ x[r]
    return out


def conv_operands(xs, w):
    """the engine's operands for the conv GEMMs: xs [W][T][Ci] -> the padded buffer [W][T + 2][Ci] (a zero row on each side of a window), and w [Co][Ci][3] -> the
    GEMM matrix [Co][3 Ci] in im2col order, k = tap * Ci + ci.  GEMM row t of a window starts at padded row stride * t: lda = stride * Ci, K = 3 Ci"""
    xs = np.asarray(xs, F)
    Wn, T, Ci = xs.shape
    buf = np.zeros((Wn, T + 2, Ci), F)
    buf[:, 1:T + 1] = xs
    return buf, np.ascontiguousarray(np.asarray(w, F).transpose(0, 2, 1).reshape(w.shape[0], 3 * Ci))


# ------------------------------------------------------------------------------------------ q|k|v
def qkv_split(l, n_split, seg_T):
    """l [M][N] -> (q|k [M][n_split], V^T [segments][N - n_split][seg_T]): rows of segment s are s * seg_T .. ; a short last segment leaves its tail columns at NaN"""
    l = np.asarray(l)
    M, N = l.shape
    n_seg = -(-M // seg_T)
    vt = np.full((n_seg, N - n_split, seg_T), np.nan, l.dtype)
    for s in range(n_seg):
        rows = l[s * seg_T:(s + 1) * seg_T, n_split:]
        vt[s, :, :rows.shape[0]] = rows.T
    return l[:, :n_split].copy(), vt


def rope_fused(lin64, cs, kind):
    """the q|k|v epilogue's partial RoPE: lin64 [M][ncols] the UNROUNDED linear of the q / k columns (heads of 64), cs [T][32] = cos[16] | sin[16], row m at position
    m mod T.  Dims [0, 16) and [16, 32) of every head are rotated, every product and the sum rounded; dims [32, 64) are rt(linear).  -> (out, mag): mag = |x1 c| + |x2 s|
    resp. |x2 c| + |x1 s| on the rotated dims (the magnitude rope_bound follows: the sum can cancel) and |out| elsewhere"""
    lin64 = np.asarray(lin64, np.float64); cs = np.asarray(cs, np.float64)
    M, ncols = lin64.shape
    assert ncols % 64 == 0 and cs.shape[1] == 32
    x = lin64.reshape(M, ncols // 64, 64)
    pos = np.arange(M) % cs.shape[0]
    c, s = cs[pos, None, :16], cs[pos, None, 16:]
    x1, x2 = x[..., :16], x[..., 16:32]
    r = lambda v: to_kind(v, kind).astype(np.float64)
    out = to_kind(x, kind)
    mag = np.abs(out).astype(np.float64)
    out[..., :16] = to_kind(r(x1 * c) + r(-x2 * s), kind)
    out[..., 16:32] = to_kind(r(x2 * c) + r(x1 * s), kind)
    mag[..., :16] = np.abs(x1 * c) + np.abs(x2 * s)
    mag[..., 16:32] = np.abs(x2 * c) + np.abs(x1 * s)
    return out.reshape(M, ncols), mag.reshape(M, ncols)


def rope_bound(mag, kind):
    """two roundings follow the linear, as in SwiGLU's product: 4 ulp of the addends' magnitude + 1e-3"""
    return 4.0 * np.maximum(mag, 1e-2) * ULP[kind] + 1e-3


def enc_rope_table(T, theta=10000.0):
    """[T][32] fp32: cos | sin of position * theta^(-2 i / 32), i < 16 (an input of the tests, not under test)"""
    inv = theta ** (-np.arange(16, dtype=np.float64) * 2.0 / 32)
    ang = np.arange(T, dtype=np.float64)[:, None] * inv[None, :]
    return np.concatenate([np.cos(ang), np.sin(ang)], axis=1).astype(F)


# ------------------------------------------------------------------------------------------ int8 (Linear8bitLt): the oracle's own functions, group by group
def linear_int8(orc, X, W, bias, group_rows):
    """oracle.quantize_rows / oracle.linear_int8 as tests/test_gpu_int8.py uses them: W quantised row-wise, X in groups of group_rows rows (one reference call each)"""
    cb, scb = orc.quantize_rows(W)
    out = np.empty((X.shape[0], W.shape[0]), F)
    for r0 in range(0, X.shape[0], group_rows):
        out[r0:r0 + group_rows] = orc.linear_int8(X[r0:r0 + group_rows], cb, scb, bias)
    return out
