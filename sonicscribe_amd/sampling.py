"""Temperature sampling of the greedy loop, restated in numpy (include/sonic_hip.h at sonic_set_request_sampling).

The contract.  A request with temperature t > 0 and a 64-bit seed emits, as its n-th token (n = 0 for the prefill's first token), the first maximum over the
vocabulary of y_i = fdiv_rn(s_i, t) + g_i in fp32, where s is the fully processed score (request bias, repetition penalty, bans - HF's order of processors, then its
TemperatureLogitsWarper) and g_i is Gumbel noise: g_i = -ln(-ln(u_i)), u_i = ((w_i >> 9) + 0.5) * 2^-23, w_i = output word i & 3 of Philox4x32-10 with
key = (seed & 0xffffffff, seed >> 32) and counter = (i >> 2, n, 0, 0).  By the Gumbel-max identity the token is an exact draw from softmax(s / t), and it is a pure
function of (scores, t, seed, n): batch, row, slot and scheduler play no part.  t = 0 is greedy decoding.  The kernel evaluates g with two fp32 logs and is
within EPS_G of the float64 value below.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
T_MIN, T_MAX = 1e-3, 100.0
# |g_kernel - g| <= EPS_G.  The device logf is the hardware's base-2 logarithm (v_log_f32: 1 ulp, so a relative error of at most 2^-23) times ln 2 in extended
# precision, rounded once (2^-24): a relative error r <= 1.5 * 2^-23 (+ second-order terms).  L = -logf(u), u exact: L = L_exact * (1 + d), |d| <= r, which moves
# ln(L) by at most r (absolute); the outer logf adds r * |g|, |g| <= 16.64.  (1 + 16.64) * 1.5 * 2^-23 = 3.154e-6, rounded up.
EPS_G = 3.2e-6
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32 (Salmon et al., SC'11).  counter: [..., 4] and key: [..., 2] of 32-bit words (broadcast against each other) -> [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _M32
    k = np.asarray(key, dtype=np.uint64) & _M32
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j], shape).copy() for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j], shape).copy() for j in range(2))
    for _ in range(int(rounds)):
        p0 = np.uint64(PHILOX_M0) * c0              # (32 x 32 -> 64 bits: no overflow in uint64)
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def check_seed(seed) -> int:
    s = int(seed)
    if not 0 <= s < 1 << 64:
        raise ValueError(f"seed {seed!r} is outside 0 .. 2^64 - 1")
    return s


def check_temperature(t) -> float:
    """0 (greedy) or a value in [1e-3, 100]; nothing is clamped (ValueError otherwise, NaN included)"""
    try:
        v = float(t)
    except (TypeError, ValueError):
        raise ValueError(f"temperature {t!r} is not a number") from None
    if not (v == 0.0 or T_MIN <= v <= T_MAX):
        raise ValueError(f"temperature {t!r} is invalid: 0 (greedy) or a value in [{T_MIN}, {T_MAX}]")
    if v != 0.0 and not T_MIN <= float(np.float32(v)) <= T_MAX:
        raise ValueError(f"temperature {t!r} leaves [{T_MIN}, {T_MAX}] when rounded to float32")
    return v


def fork_seed(seed: int, j: int) -> int:
    """the seed of fork j of a best_of request: (seed + j) mod 2^64 - fork 0 draws with the request's own seed, so best_of = 1 is the request itself"""
    if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or int(j) < 0:
        raise ValueError(f"fork index must be a non-negative integer (got {j!r})")
    return (check_seed(seed) + int(j)) & 0xFFFFFFFFFFFFFFFF


def temperatures(temperature) -> Tuple[Tuple[float, ...], bool]:
    """a float (one attempt) or a sequence (the fallback ladder) -> (validated tuple, is it a ladder)"""
    if isinstance(temperature, (int, float, np.floating, np.integer)):
        return (check_temperature(temperature),), False
    ts = tuple(check_temperature(t) for t in temperature)
    if not ts:
        raise ValueError("temperature: an empty sequence")
    return ts, True


def uniforms(seed: int, step: int, V: int) -> np.ndarray:
    """u_i of the contract for ids 0 .. V - 1, float64 (every value is exact in fp32 too and strictly inside (0, 1))"""
    seed = check_seed(seed)
    ng = (int(V) + 3) // 4
    ctr = np.zeros((ng, 4), np.uint64)
    ctr[:, 0] = np.arange(ng, dtype=np.uint64)
    ctr[:, 1] = np.uint64(int(step) & 0xFFFFFFFF)
    w = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)).reshape(-1)[: int(V)]
    return ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_noise(seed: int, step: int, V: int) -> np.ndarray:
    """g_i = -ln(-ln(u_i)) in float64"""
    return -np.log(-np.log(uniforms(seed, step, V)))


def perturbed(scores_f32, t: float, seed: int, step: int, noise: Optional[np.ndarray] = None) -> np.ndarray:
    """y of the contract: the fp32 quotient (correctly rounded, as the kernel's) plus the noise, in float64 (`noise`: in place of gumbel_noise)"""
    s = np.asarray(scores_f32, np.float32)
    with np.errstate(invalid="ignore"):
        q = (s / np.float32(t)).astype(np.float32)
    g = gumbel_noise(seed, step, s.shape[-1]) if noise is None else np.asarray(noise, np.float64)
    return q.astype(np.float64) + g


def sample_reference(scores_f32, t: float, seed: int, step: int) -> int:
    """the token of the contract with exact noise: the first maximum of y (t = 0: of the scores); a row of -inf only gives 0"""
    t = check_temperature(t)
    s = np.asarray(scores_f32, np.float32)
    if t == 0.0:
        return int(np.argmax(s))
    return int(np.argmax(perturbed(s, t, seed, step)))


def pack_sampling(temperature: Sequence[float], seed: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """per-request values -> sonic_set_request_sampling's arrays (float32 temperatures, uint64 seeds), validated"""
    t = np.asarray([check_temperature(x) for x in temperature], np.float32)
    s = np.asarray([check_seed(x) for x in seed], np.uint64)
    if t.shape != s.shape:
        raise ValueError("one temperature and one seed per request")
    return t, s
