"""Temperature sampling of the greedy loop, restated in numpy (include/sonic_hip.h at sonic_set_request_sampling).

The contract.  A request with temperature t > 0 and a 64-bit seed emits, as its n-th token (n = 0 for the prefill's first token), the first maximum over the
vocabulary of y_i = fdiv_rn(s_i, t) + g_i in fp32, where s is the fully processed score (request bias, repetition penalty, bans - HF's order of processors, then its
TemperatureLogitsWarper) and g_i is Gumbel noise: g_i = -ln(-ln(u_i)), u_i = ((w_i >> 9) + 0.5) * 2^-23, w_i = output word i & 3 of Philox4x32-10 with
key = (seed & 0xffffffff, seed >> 32) and counter = (i >> 2, n, 0, 0).  By the Gumbel-max identity the token is an exact draw from softmax(s / t), and it is a pure
function of (scores, t, seed, n): batch, row, slot and scheduler play no part.  t = 0 is greedy decoding.  The kernel evaluates g with two fp32 logs and is
within EPS_G of the float64 value below.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
T_MIN, T_MAX = 1e-3, 100.0
NO_CUT = (0, 1.0, 0.0)      # (top_k, top_p, min_p) that cut nothing
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


class CallSampling(NamedTuple):
    """One call's sampling as ASRModel._request_sampling resolves it: the temperatures (one, or the fallback ladder's), whether they are a ladder, the seed and the
    (top_k, top_p, min_p) of every sampled decode - always a triple, NO_CUT when the call cuts nothing."""
    temperatures: Tuple[float, ...]
    ladder: bool
    seed: int
    cut: Tuple[int, float, float] = NO_CUT

    @property
    def cuts(self) -> bool:      # does the call cut the tail at all
        return tuple(self.cut) != NO_CUT

    def attempt(self, t: float, seed: Optional[int] = None) -> tuple:
        """What the scheduler is told for one attempt at temperature t (seed: a fork's own, else the call's): the pair (t, seed) at t = 0 - greedy rows ignore the
        cut - and for a call that cuts nothing, as such requests always stated; (t, seed, top_k, top_p, min_p) otherwise."""
        pair = (t, self.seed if seed is None else seed)
        return pair + tuple(self.cut) if self.cuts and t > 0 else pair


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


# ---------------------------------------------------------------- truncation: top_k, top_p, min_p
"""The contract.  A request with t > 0 may bring top_k (integer >= 0, 0 = off), top_p (in (0, 1], 1 = off) and min_p (in [0, 1], 0 = off); rows with t = 0 ignore them.
y_i = fdiv_rn(s_i, t) in fp32, s the fully processed score.  The ids are ordered by (y descending, id ascending); every filter keeps a prefix of that order and the
kept set is the shortest of the three prefixes - HF's chain TopK -> TopP -> MinP, each later filter stated on the renormalised survivors of the earlier ones:
  top_k  every id with y_i >= the k-th largest y (HF's `scores < kth` keeps the ties; k >= the number of finite scores removes nothing)
  top_p  over the top_k survivors K, masses w_i = exp(y_i - y_max): rank r is kept iff the mass of ranks 0 .. r - 1 is < top_p * mass(K) (HF's
         `cumulative_probs <= 1 - top_p` on the ascending sort, rewritten; rank 0 always stays).  Equal values at the boundary go by the lower id (HF leaves them to
         torch.sort)
  min_p  every id with y_i >= fadd_rn(y_max, lnm), lnm = float32(log(min_p)) (HF's `p_i < min_p * p_max` in the log domain)
A row whose scores are all -inf keeps everything.  The token is the first maximum of y_i + g_i over the kept ids: an exact draw from the renormalised truncated
distribution.  The kernel accumulates the masses in fixed point (2^-32) from the hardware exponential: its normalised cumulative mass is within EPS_MASS of float64."""
TOP_K_MAX = (1 << 31) - 1
# |c_kernel(r) - c(r)| <= EPS_MASS, c(r) = mass of ranks 0 .. r - 1 over mass(K), for vocabularies up to 65 536 ids.  A term is
# rint(exp2(fl(fl(y - y_max) * fl(log2 e))) * 2^32): three roundings of 2^-24 on an argument of at most 33 in size (a term beyond it is below half a quantum) move it
# by 33 * 3 * 2^-24 = 5.9e-6, the exponential by ln 2 times that, 4.09e-6, relative; v_exp_f32 adds 1 ulp, 2^-23 = 1.2e-7: rho = 4.21e-6 per term, hence per sum.  The
# rounding to the quantum adds at most V / 2 quanta to a sum, and mass(K) is at least 2^32 quanta (the maximum's own term is exactly 2^32): V * 2^-33 each for the
# numerator and the denominator.  A quotient of two such sums moves by 2 rho + 2 V 2^-33 = 8.42e-6 + 1.53e-5 = 2.37e-5 at V = 65 536; the threshold's own rounding
# (the product top_p * mass in float64, then one quantum) is below 2^-31.  Rounded up
EPS_MASS = 2.4e-5


def check_truncation(top_k=0, top_p=1.0, min_p=0.0) -> Tuple[int, float, float]:
    """(top_k, top_p, min_p) validated: nothing is clamped (ValueError names the parameter; NaN included)"""
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 0 <= int(top_k) <= TOP_K_MAX:
        raise ValueError(f"top_k {top_k!r} is invalid: an integer in 0 .. 2^31 - 1 (0 = off)")
    try:
        p, m = float(top_p), float(min_p)
    except (TypeError, ValueError):
        raise ValueError(f"top_p {top_p!r} / min_p {min_p!r} is not a number") from None
    if not 0.0 < p <= 1.0 or not 0.0 < float(np.float32(p)) <= 1.0:
        raise ValueError(f"top_p {top_p!r} is invalid: a value in (0, 1] (1 = off), also when rounded to float32")
    if not 0.0 <= m <= 1.0:
        raise ValueError(f"min_p {min_p!r} is invalid: a value in [0, 1] (0 = off)")
    return int(top_k), p, m


def truncation_words(top_k=0, top_p=1.0, min_p=0.0) -> np.ndarray:
    """the row of "request_truncation": float32 [top_k, top_p, min_p] (top_k must be exact in float32: up to 2^24, beyond that it is off for every vocabulary
    the kernel serves and is sent as 2^24)"""
    k, p, m = check_truncation(top_k, top_p, min_p)
    return np.array([min(k, 1 << 24), p, m], np.float32)


def log_min_p(min_p: float) -> np.float32:
    """lnm of the contract: float32(log(min_p)) (min_p = 0: -inf, the filter is off)"""
    with np.errstate(divide="ignore"):
        return np.float32(np.log(np.float64(np.float32(min_p))))


def quotient(scores_f32, t: float) -> np.ndarray:
    """y of the truncation contract: fdiv_rn(s, t) in fp32 (numpy's float32 division is correctly rounded); -0.0 counts as +0.0"""
    with np.errstate(invalid="ignore"):
        y = (np.asarray(scores_f32, np.float32) / np.float32(t)).astype(np.float32)
    return y + np.float32(0.0)


def truncation_order(y) -> np.ndarray:
    """the ids by (y descending, id ascending)"""
    return np.argsort(-np.asarray(y, np.float64), kind="stable")


def truncation_counts(y, top_k=0, top_p=1.0, min_p=0.0, p_shift: float = 0.0) -> Tuple[int, int, int]:
    """(n_k, n_p, n_m): the lengths of the three prefixes of truncation_order(y) (V where a filter is off).  p_shift moves top_p for the tests' bracket
    n(p - eps) <= n_kernel <= n(p + eps); the masses are float64"""
    k, p, m = check_truncation(top_k, top_p, min_p)
    y = np.asarray(y, np.float32)
    V = y.shape[0]
    ymax = y.max() if V else np.float32(-np.inf)
    if not np.isfinite(ymax):                      # every score -inf: nothing is removed
        return V, V, V
    ys = y[truncation_order(y)]
    n_k = V
    if 0 < k < V:
        n_k = int(np.count_nonzero(ys >= ys[k - 1]))
    n_p = V
    if np.float32(p) < 1.0:
        w = np.exp(ys[:n_k].astype(np.float64) - np.float64(ymax))
        before = np.concatenate([[0.0], np.cumsum(w)[:-1]])
        thr = (np.float64(np.float32(p)) + p_shift) * w.sum()
        n_p = max(1, int(np.count_nonzero(before < thr)))      # (before is non-decreasing: the kept ranks are a prefix)
    n_m = V
    if m > 0.0:
        n_m = int(np.count_nonzero(ys >= np.float32(ymax + log_min_p(m))))
    return n_k, n_p, n_m


def truncation_kept(scores_f32, t: float, top_k=0, top_p=1.0, min_p=0.0, p_shift: float = 0.0) -> np.ndarray:
    """the kept ids in the contract's order: the first min(n_k, n_p, n_m) of truncation_order(y)"""
    y = quotient(scores_f32, check_temperature(t))
    return truncation_order(y)[: min(truncation_counts(y, top_k, top_p, min_p, p_shift))]


def sample_truncated(scores_f32, t: float, seed: int, step: int, top_k=0, top_p=1.0, min_p=0.0) -> int:
    """the token of the contract with exact noise: the first maximum of y + g over the kept ids (t = 0: greedy, the three parameters are ignored)"""
    t = check_temperature(t)
    s = np.asarray(scores_f32, np.float32)
    if t == 0.0:
        return int(np.argmax(s))
    kept = np.sort(truncation_kept(s, t, top_k, top_p, min_p))
    yy = perturbed(s, t, seed, step)[kept]
    return int(kept[int(np.argmax(yy))])


def pack_truncation(values: Sequence) -> np.ndarray:
    """per-request (top_k, top_p, min_p) -> float32 [R][3] for sonic_load_tensor "request_truncation", validated"""
    return np.stack([truncation_words(*v) for v in values]).astype(np.float32).reshape(-1, 3)
