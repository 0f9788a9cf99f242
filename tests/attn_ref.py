"""Plain float64 reference for the attention kernel tests (tests/test_gpu_attn_kernels.py, checked itself by tests/test_attn_ref.py).

attention(): softmax attention of one (sequence, head) with an explicit count of visible keys per query.  Besides o = sum_i p_i v_i it returns
A = sum_i p_i |v_i|, the quantity the error bound needs.

The bound.  The kernels (csrc/attn.hip) compute the scores and every accumulation in fp32, round each probability to the element type before the
P.V product (relative error <= u), keep the row sum in fp32, and round the output once (u again).  With q_i = p_i (1 + d_i), |d_i| <= u:
    |sum_i q_i v_i - o| <= u * sum_i p_i |v_i| = u * A,   and the final rounding adds u * |o|  (second-order terms dropped), hence
    |got - o| <= c * u * (A + |o|)   element by element,   u = 2^-8 (bf16), 2^-11 (fp16).
c = 1 is the derivation; the tests use c = 1.5, the margin for fp32 accumulation order and the hardware exp.  The margin is not fitted to a kernel:
emulate() below restates the decode kernel's rounding points (16 keys per step, online softmax, fp32 row sum, rounded probabilities, one rounded output)
in numpy, and over random, spiked and rising-score rows with 1..600 keys it stays below 0.6 of the c = 1 bound in both types (tests/test_attn_ref.py
runs 60 such rows per type and asserts c <= 1 for them).

The derivation presumes NORMAL numbers.  fp16 leaves that range early: below 2^-14 a rounding costs up to 2^-25 absolutely, whatever the value, and a
probability below 2^-25 becomes 0.  Next to a key that dominates by more than ~10 nats every other probability is down there, so the error carries a term
2^-25 * sum_i |v_i| (about 1e-5 for 600 keys) that u (A + |o|) covers only while A + |o| itself is not tiny - it fails where the dominating value element
happens to be ~1e-4 or the output itself is subnormal (seen in emulate(): 4.4 x the c = 1 bound on an element with |o| = 2.7e-5).  bf16 shares fp32's
exponent range and has no such term.  The bound is kept as derived; values() therefore draws fp16 VALUE rows away from zero (0.25 <= |v| <= 1.5), which makes
A >= 0.25 and the absolute term at most ~0.12 of the c = 1 bound at 600 keys.  Queries and keys stay N(0, 1) in both types.

fused_prologue(): the rounding sequence of the fused decode prologue (slab sum in ascending slab order, rounded; rotate-half RoPE with every product and
the sum rounded), written out in fp32 so that the appended K / V rows can be compared bit for bit.
"""
import numpy as np

from sonicscribe_amd import synth

U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
C_BOUND = 1.5


def rounder(kind):
    return synth.round_bf16 if kind == "bf16" else synth.round_f16


def values(rng, shape, kind):
    """value rows for the bound tests, rounded to the element type: N(0, 1) for bf16; for fp16 a random sign times U(0.25, 1.5) (module docstring)"""
    if kind == "bf16":
        return synth.round_bf16(rng.standard_normal(shape).astype(np.float32))
    return synth.round_f16((rng.choice([-1.0, 1.0], size=shape) * rng.uniform(0.25, 1.5, size=shape)).astype(np.float32))


def attention(q, k, v, n_vis, scale):
    """q [nq][hd], k / v [nk][hd], n_vis [nq] (query i sees keys 0 .. n_vis[i] - 1, at least one) -> (o, A), both float64 [nq][hd]"""
    q = np.asarray(q, np.float64); k = np.asarray(k, np.float64); v = np.asarray(v, np.float64)
    n_vis = np.asarray(n_vis).reshape(-1)
    assert q.ndim == 2 and k.shape == v.shape and n_vis.shape == (q.shape[0],) and n_vis.min() >= 1 and n_vis.max() <= k.shape[0]
    nmax = int(n_vis.max())
    k = k[:nmax]; v = v[:nmax]                      # nothing behind the last visible key takes part (it may be poison)
    s = (q @ k.T) * scale
    vis = np.arange(nmax)[None, :] < n_vis[:, None]
    s = np.where(vis, s, -np.inf)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return p @ v, p @ np.abs(v)


def bound(o, A, kind, c=C_BOUND):
    return c * U[kind] * (A + np.abs(o))


def worst_ratio(got, o, A, kind):
    """max over the elements of |got - o| / (u * (A + |o|)): the share of the c = 1 bound in use; the tests assert <= C_BOUND.  Where the bound is 0
    (every visible value 0) the result must be exactly 0."""
    got = np.asarray(got, np.float64)
    b = bound(o, A, kind, 1.0)
    err = np.abs(got - o)
    if not np.isfinite(got).all():
        return float("inf")
    r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def emulate(q, k, v, n, scale, kind, slice_keys=16, waves=8):
    """The decode kernel's arithmetic at its rounding points, one query: keys dealt round-robin in slices of `slice_keys` to `waves` online-softmax states
    (fp32), probabilities rounded to the element type for P.V only, states merged in fp32, one rounded output.  -> [hd] float32"""
    rt = rounder(kind)
    f = np.float32
    q = np.asarray(q, f); k = np.asarray(k, f)[:n]; v = np.asarray(v, f)[:n]
    m = np.full(waves, -1e30, f); l = np.zeros(waves, f); acc = np.zeros((waves, v.shape[1]), f)
    for s0 in range(0, n, slice_keys):
        w = (s0 // slice_keys) % waves
        sc = ((k[s0:s0 + slice_keys] @ q).astype(f) * f(scale)).astype(f)
        mn = max(m[w], sc.max())
        alpha = np.exp(f(m[w] - mn)).astype(f)
        p = np.exp((sc - mn).astype(f)).astype(f)
        l[w] = f(l[w] * alpha + p.sum(dtype=f))
        acc[w] = (acc[w] * alpha + rt(p) @ v[s0:s0 + slice_keys]).astype(f)
        m[w] = mn
    M = m.max()
    fw = np.exp((m - M).astype(f)).astype(f)
    num = (fw[:, None] * acc).sum(axis=0, dtype=f); den = (fw * l).sum(dtype=f)
    return rt((num / den).astype(f))


def rope_table(ctx_max, theta=10000.0, hd=128):
    """[ctx_max][hd] fp32: cos | sin of position * theta^(-2 i / hd), i < hd / 2 (the table's values are an input of the tests, not under test)"""
    inv = theta ** (-np.arange(hd // 2, dtype=np.float64) * 2.0 / hd)
    ang = np.arange(ctx_max, dtype=np.float64)[:, None] * inv[None, :]
    return np.concatenate([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)


def fused_prologue(slabs, cs_rows, Hq, Hkv, kind):
    """slabs [ksplit][B][(Hq + 2 Hkv) * 128] fp32 (the rows in use), cs_rows [B][128] fp32 (the table row of each sequence's position) ->
    (q [B][Hq][128], k [B][Hkv][128], v [B][Hkv][128]) fp32 holding element-type values, with the kernel's roundings:
    y = rT(slab sum, ascending ks);  q, k: first half rT(rT(y1 c) + rT(-y2 s)), second half rT(rT(y2 c) + rT(y1 s));  v = y."""
    rt = rounder(kind)
    f = np.float32
    slabs = np.asarray(slabs, f)
    B = slabs.shape[1]
    x = np.zeros(slabs.shape[1:], f)
    for ks in range(slabs.shape[0]):
        x = (x + slabs[ks]).astype(f)
    y = rt(x).reshape(B, Hq + 2 * Hkv, 128)
    c = np.asarray(cs_rows, f)[:, None, :64]; s = np.asarray(cs_rows, f)[:, None, 64:]
    y1, y2 = y[:, :Hq + Hkv, :64], y[:, :Hq + Hkv, 64:]
    o1 = rt((rt((y1 * c).astype(f)) + rt((-y2 * s).astype(f))).astype(f))
    o2 = rt((rt((y2 * c).astype(f)) + rt((y1 * s).astype(f))).astype(f))
    qk = np.concatenate([o1, o2], axis=2)
    return qk[:, :Hq].copy(), qk[:, Hq:].copy(), y[:, Hq + Hkv:].copy()
