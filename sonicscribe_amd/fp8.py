"""Mode fp8's weight model in numpy: the statement the library's fp8_snap_kernel (csrc/gemv_fp8.hip, csrc/fp8_codec.h) is held to, bit for bit.

Every output row n of a decoder matrix W[N][K] gets a power-of-two scale s_n - the smallest with amax_n / s_n <= 448, 1 for an all-zero row, never below 2^-117 -
its codes are q = RNE_e4m3fn(W / s_n) (OCP e4m3fn: 4 exponent bits at bias 7, 3 mantissa bits, no infinities, largest magnitude 448) and the snapped row is
W' = s_n q.  W / s_n is exact, and W' has four significant bits: it is exact in bfloat16.  The snap is idempotent and amax / s lies in (224, 448]."""
from typing import Dict, Tuple

import numpy as np

E4M3_MAX = 448.0
SCALE_EXP_MIN = -117       # s >= 2^-117: s times the smallest e4m3 step (2^-9) is still a normal bfloat16


def row_scales(w: np.ndarray) -> np.ndarray:
    """s_n of every row of w [N][K]: float32 powers of two"""
    amax = np.abs(np.asarray(w, np.float32)).max(axis=1) if w.shape[1] else np.zeros(w.shape[0], np.float32)
    if not np.isfinite(amax).all():
        raise ValueError("fp8.row_scales: the matrix holds a value that is not finite")
    m, x = np.frexp(amax)                                   # amax = m 2^x, m in [0.5, 1); 448 = 0.875 * 2^9
    e = np.where(amax > 0, np.maximum(x - 9 + (m > 0.875), SCALE_EXP_MIN), 0).astype(np.int32)
    return np.ldexp(np.float32(1.0), e).astype(np.float32)


def encode(v: np.ndarray) -> np.ndarray:
    """round-to-nearest-even of v (float32, |v| <= 448) to e4m3fn codes (uint8)"""
    v = np.ascontiguousarray(v, np.float32)
    u = v.view(np.uint32)
    sign = ((u >> 24) & 0x80).astype(np.uint32)
    a = u & 0x7FFFFFFF
    t = a.view(np.float32) * np.float32(512.0)              # below 2^-6: the subnormal grid of step 2^-9 (np.rint rounds ties to even; 8 is the first normal code)
    sub = np.rint(np.where(a < 0x3C800000, t, 0)).astype(np.uint32)
    r = a + 0x7FFFF + ((a >> 20) & 1)                       # RNE at mantissa bit 20
    nrm = np.minimum((((r >> 23) - 120) << 3) | ((r >> 20) & 7), 0x7E)
    return (sign | np.where(a < 0x3C800000, sub, nrm)).astype(np.uint8)


def decode(codes: np.ndarray) -> np.ndarray:
    """the float32 values of e4m3fn codes"""
    c = np.asarray(codes).astype(np.int32)
    E, m = (c >> 3) & 15, c & 7
    a = np.where(E > 0, np.ldexp((8 + m).astype(np.float32), E - 10), m.astype(np.float32) * np.float32(2.0 ** -9)).astype(np.float32)
    return np.where(c & 0x80, -a, a).astype(np.float32)


def snap(w: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """w [N][K] -> (W' float32 [N][K], s float32 [N], codes uint8 [N][K])"""
    w = np.asarray(w, np.float32)
    s = row_scales(w)
    codes = encode(w / s[:, None])
    return (s[:, None] * decode(codes)).astype(np.float32), s, codes


def snapped_names(dims) -> Tuple[str, ...]:
    """the tensors mode fp8 snaps: the decoder's seven projections per layer and the tied embedding - nothing of the encoder, the projector or the norms"""
    lm = "model.language_model."
    names = [lm + "embed_tokens.weight"]
    for i in range(dims.dec_layers):
        p = f"{lm}layers.{i}."
        names += [p + "self_attn." + n + "_proj.weight" for n in ("q", "k", "v", "o")] + [p + "mlp." + n + "_proj.weight" for n in ("gate", "up", "down")]
    return tuple(names)


def snap_state_dict(sd: Dict[str, np.ndarray], dims) -> Dict[str, np.ndarray]:
    """a copy of the state dict with exactly the tensors the engine snaps replaced by their W' (the scales are per row, so the engine's packing of q|k|v and of
    gate/up does not matter)"""
    out = dict(sd)
    for name in snapped_names(dims):
        out[name] = snap(sd[name])[0]
    return out


def extra_weight_bytes(dims) -> int:
    """what option fp8_weights adds to an engine's weight bytes: one byte per snapped weight and four per snapped row (the packed matrices' N K + 4 N, summed)"""
    qd, kd, D, ff = dims.dec_heads * dims.dec_head_dim, dims.dec_kv_heads * dims.dec_head_dim, dims.dec_d, dims.dec_ff
    mats = [(qd + 2 * kd, D), (D, qd), (2 * ff, D), (D, ff)] * dims.dec_layers + [(dims.vocab, D)]
    return sum(n * k + 4 * n for n, k in mats)
