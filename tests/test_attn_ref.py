"""CPU check of the reference the attention kernel tests use (tests/attn_ref.py): the float64 attention with its derived bound
|got - o| <= 1.5 u (A + |o|) must hold for arithmetic that rounds where the kernels round, without any kernel in the loop -
the C oracle's oracle_attention (bf16 probabilities and output, pinned to the reference fixtures by test_oracle_golden.py) and a numpy
restatement of the decode kernel's 16-key online softmax in both element types."""
import numpy as np
import pytest

import attn_ref as R
from gpu_common import load_oracle
from sonicscribe_amd import synth


@pytest.fixture(scope="module")
def orc():
    return load_oracle()


def bf(x):
    return synth.round_bf16(np.asarray(x, np.float32))


@pytest.mark.parametrize("Tq,Tk,Hq,Hkv,hd,causal,q_pos0", [
    (40, 40, 2, 2, 64, 0, 0),            # every key visible
    (130, 130, 4, 1, 128, 1, 0),         # causal
    (65, 265, 4, 2, 128, 1, 200),        # causal with an offset: query t sits at position 200 + t
    (1, 277, 4, 1, 128, 1, 276),         # the decode shape of test_decode_attention
    (33, 97, 16, 4, 128, 1, 64),         # the production group layout
    (50, 50, 4, 4, 128, 1, 0),
])
def test_oracle_attention_within_bound(orc, Tq, Tk, Hq, Hkv, hd, causal, q_pos0):
    rng = np.random.default_rng(Tq * 1000 + Tk)
    q = bf(rng.standard_normal((Tq, Hq, hd))); k = bf(rng.standard_normal((Tk, Hkv, hd))); v = bf(rng.standard_normal((Tk, Hkv, hd)))
    if Tk > 20:
        k[Tk // 2, 0] = bf(q[Tq // 2, 0] * 4.0)                 # one dominant key (~45 nats at hd = 128) for one query of head 0
    got = np.empty((Tq, Hq, hd), np.float32)
    orc.lib().oracle_attention(q.ctypes.data, k.ctypes.data, v.ctypes.data, got.ctypes.data, Tq, Tk, Hq, Hkv, hd, causal, q_pos0, 1)
    n_vis = np.minimum(q_pos0 + np.arange(Tq) + 1, Tk) if causal else np.full(Tq, Tk)
    worst = 0.0
    for h in range(Hq):
        o, A = R.attention(q[:, h], k[:, h // (Hq // Hkv)], v[:, h // (Hq // Hkv)], n_vis, 1.0 / np.sqrt(hd))
        worst = max(worst, R.worst_ratio(got[:, h], o, A, "bf16"))
    print(f"oracle_attention vs float64: worst err / (u (A + |o|)) = {worst:.3f}")
    assert worst <= R.C_BOUND, worst


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_kernel_rounding_points_within_bound(kind):
    """the decode kernel's rounding points restated in numpy (attn_ref.emulate), random and spiked rows with 1..600 keys: the margin c = 1.5 covers them
    with room to spare.  fp16 value rows come from attn_ref.values(), away from zero: the derivation holds for normal numbers (attn_ref's docstring)"""
    rng = np.random.default_rng(5 if kind == "bf16" else 6)
    rt = R.rounder(kind)
    worst = 0.0
    for case in range(60):
        n = int(rng.integers(1, 601))
        q = rt(rng.standard_normal(128)); k = rt(rng.standard_normal((n, 128))); v = R.values(rng, (n, 128), kind)
        if case % 3 == 1:
            k[int(rng.integers(0, n))] = rt(q * (2.0 if kind == "f16" else 4.0))
        if case % 3 == 2:
            k *= np.linspace(0.0, 1.0, n, dtype=np.float32)[:, None]; k = rt(k)
        got = R.emulate(q, k, v, n, 1.0 / np.sqrt(128.0), kind)
        o, A = R.attention(q[None], k, v, [n], 1.0 / np.sqrt(128.0))
        worst = max(worst, R.worst_ratio(got[None], o, A, kind))
    print(f"{kind}: emulated kernel rounding vs float64: worst err / (u (A + |o|)) = {worst:.3f}")
    assert worst <= 1.0, worst


def test_worst_ratio_sees_a_wrong_key():
    """the bound is tight enough to matter: one key too many or one missing in a 24-key average is far outside it, the output rounding alone uses at
    most half of it.  (A single ordinary key among n weighs about |v| / n, which sinks towards u A as n passes 1 / u: the kernel tests therefore count
    keys with exact one-hot patterns and do not lean on the bound for that.)"""
    rng = np.random.default_rng(9)
    q = bf(rng.standard_normal((1, 128)) * 0.3); k = bf(rng.standard_normal((278, 128))); v = bf(rng.standard_normal((278, 128)))
    sc = 1.0 / np.sqrt(128.0)
    o, A = R.attention(q, k, v, [24], sc)
    for n in (23, 25):
        o2, _ = R.attention(q, k, v, [n], sc)
        assert R.worst_ratio(bf(o2), o, A, "bf16") > 2 * R.C_BOUND
    assert R.worst_ratio(bf(o), o, A, "bf16") <= 0.5 + 1e-9          # the output rounding alone: u |o| <= u (A + |o|) / 2


def test_fused_prologue_is_a_rotation_up_to_rounding():
    rng = np.random.default_rng(2)
    Hq, Hkv, B = 4, 2, 3
    slabs = rng.standard_normal((4, B, (Hq + 2 * Hkv) * 128)).astype(np.float32)
    cs = R.rope_table(64)[[0, 5, 63]]
    q, k, v = R.fused_prologue(slabs, cs, Hq, Hkv, "bf16")
    x = slabs.astype(np.float64).sum(0).reshape(B, Hq + 2 * Hkv, 128)
    assert np.array_equal(q[0], bf(x[0, :Hq].astype(np.float32)))                    # position 0: cos 1, sin 0
    assert np.abs(v - x[:, Hq + Hkv:]).max() <= 2.0 ** -8 * np.abs(x).max()
    c, s = cs[:, None, :64].astype(np.float64), cs[:, None, 64:].astype(np.float64)
    want = np.concatenate([x[:, Hq:Hq + Hkv, :64] * c - x[:, Hq:Hq + Hkv, 64:] * s, x[:, Hq:Hq + Hkv, 64:] * c + x[:, Hq:Hq + Hkv, :64] * s], axis=2)
    assert np.abs(k - want).max() <= 4 * 2.0 ** -8 * np.abs(x).max()
