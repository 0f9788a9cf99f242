"""tests/gemm_ref.py pinned on the CPU: against torch where torch has the operation (linear, GELU, SiLU, conv1d), against glue_ref.rope for the rotation, and
against a loop for the layouts.  No GPU."""
import numpy as np
import pytest
import torch

import gemm_ref as R
import glue_ref as G
from attn_ref import rounder
from gpu_common import load_oracle

F = np.float32
t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))


def _values(rng, shape, kind, scale=1.0):
    return rounder(kind)((rng.standard_normal(shape) * scale).astype(F))


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_linear_gelu_resid_against_torch(kind):
    rng = np.random.default_rng(3)
    A, W, b = _values(rng, (37, 64), kind, 0.5), _values(rng, (48, 64), kind, 0.2), _values(rng, 48, kind, 0.1)
    lin = R.linear(A, W, b)
    assert lin.dtype == np.float64 and np.array_equal(lin, torch.nn.functional.linear(t64(A), t64(W), t64(b)).numpy())
    assert np.array_equal(R.linear(A, W), torch.nn.functional.linear(t64(A), t64(W)).numpy())
    l = R.to_kind(lin, kind)
    assert l.dtype == F and np.array_equal(l, rounder(kind)(l)) and np.abs(l - lin).max() <= np.abs(lin).max() * R.ULP[kind]
    g = R.gelu(l, kind)
    want = torch.nn.functional.gelu(t64(l)).numpy()                   # approximate="none": the erf form
    assert np.array_equal(g, R.to_kind(want, kind)) and np.array_equal(R.erf64(l), torch.special.erf(t64(l)).numpy())
    Rs = _values(rng, l.shape, kind)
    out, mag = R.resid(l, Rs, kind)
    assert np.array_equal(out, R.to_kind(l.astype(np.float64) + Rs, kind)) and np.array_equal(mag, np.abs(l.astype(np.float64)) + np.abs(Rs))
    assert R.ULP == {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
    assert np.array_equal(R.ulp_tol(np.array([0.0, 1.0, -4.0]), 2, kind), 2 * np.array([1e-2, 1.0, 4.0]) * R.ULP[kind])


@pytest.mark.parametrize("kind,group", [("bf16", 16), ("bf16", 8), ("f16", 16), ("f16", 8)])
def test_swiglu_and_interleave(kind, group):
    rng = np.random.default_rng(4)
    ff, K, M = 48, 64, 9
    Wg, Wu, A = _values(rng, (ff, K), kind, 0.2), _values(rng, (ff, K), kind, 0.2), _values(rng, (M, K), kind)
    Wi = R.interleave(Wg, Wu, group)
    for n in range(2 * ff):                                           # row n of the projection: group n // (2 group), gate half first
        blk, r = divmod(n, 2 * group)
        assert np.array_equal(Wi[n], (Wg if r < group else Wu)[blk * group + r % group])
    if group == 16:
        assert np.array_equal(Wi, G.interleave16(Wg, Wu))
    got = R.swiglu(R.to_kind(R.linear(A, Wi), kind), kind, gu8=group == 8)
    g, u = R.to_kind(R.linear(A, Wg), kind), R.to_kind(R.linear(A, Wu), kind)
    s = R.to_kind(torch.nn.functional.silu(t64(g)).numpy(), kind)
    assert np.array_equal(got, R.to_kind(s.astype(np.float64) * u, kind))


@pytest.mark.parametrize("stride,T,Ci,Co", [(1, 21, 8, 5), (2, 22, 6, 7), (2, 21, 6, 7), (1, 1, 4, 3)])
def test_conv1d_against_torch_and_its_gemm_form(stride, T, Ci, Co):
    rng = np.random.default_rng(T)
    x, w, b = rng.standard_normal((T, Ci)), rng.standard_normal((Co, Ci, 3)), rng.standard_normal(Co)
    ref = R.conv1d(x, w, b, stride)
    want = torch.nn.functional.conv1d(t64(x.T)[None], t64(w), t64(b), stride=stride, padding=1)[0].numpy().T
    assert ref.shape == want.shape and np.abs(ref - want).max() <= 1e-12
    # the engine's GEMM over the padded buffer: row t of the window starts at padded row stride * t and spans 3 Ci elements (lda = stride * Ci < K: overlapping rows)
    buf, Wm = R.conv_operands(x.astype(F)[None], w.astype(F))
    assert buf.shape == (1, T + 2, Ci) and not buf[0, 0].any() and not buf[0, -1].any() and Wm.shape == (Co, 3 * Ci)
    flat = buf.reshape(-1).astype(np.float64)
    T_out = ref.shape[0]
    assert stride * Ci * (T_out - 1) + 3 * Ci <= flat.size
    rows = np.stack([flat[stride * Ci * t: stride * Ci * t + 3 * Ci] for t in range(T_out)])
    gemm = R.linear(rows, Wm, b)
    assert np.abs(gemm - R.conv1d(x.astype(F), w.astype(F), b, stride)).max() <= 1e-12


def test_qkv_split():
    M, N, n_split, seg_T = 10, 7, 4, 4
    l = np.arange(M * N, dtype=F).reshape(M, N)
    qk, vt = R.qkv_split(l, n_split, seg_T)
    assert qk.shape == (M, n_split) and vt.shape == (3, N - n_split, seg_T) and np.array_equal(qk, l[:, :n_split])
    for m in range(M):
        for n in range(n_split, N):
            assert vt[m // seg_T, n - n_split, m % seg_T] == l[m, n]
    assert np.isnan(vt[2, :, 2:]).all() and not np.isnan(vt[:2]).any()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_rope_fused_against_glue_ref(kind):
    """On a linear that is already element-type valued the fused form IS rope_enc_kernel's arithmetic (glue_ref.rope, rd = 32 of hd = 64); on an unrounded one
    the two differ by the rounding of x1 / x2 alone, which rope_bound covers with room"""
    rng = np.random.default_rng(6)
    M, T, heads = 23, 7, 3
    cs = R.enc_rope_table(T)
    assert cs.shape == (T, 32) and cs.dtype == F and np.array_equal(cs[0], np.r_[np.ones(16), np.zeros(16)].astype(F))
    assert np.allclose(cs[3, 1], np.cos(3 * 10000.0 ** (-2.0 / 32))) and np.allclose(cs[3, 17], np.sin(3 * 10000.0 ** (-2.0 / 32)))
    x = _values(rng, (M, heads * 64), kind)
    out, mag = R.rope_fused(x, cs, kind)
    want = G.rope(x.reshape(M, heads, 64), cs[np.arange(M) % T][:, None, :], 32, kind).reshape(M, -1)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    x3 = x.reshape(M, heads, 64).astype(np.float64); c = cs[np.arange(M) % T].astype(np.float64)
    assert np.array_equal(mag.reshape(M, heads, 64)[..., 5], np.abs(x3[..., 5] * c[:, None, 5]) + np.abs(x3[..., 21] * c[:, None, 21]))
    assert np.array_equal(mag.reshape(M, heads, 64)[..., 40], np.abs(x3[..., 40]))
    raw = rng.standard_normal((M, heads * 64))
    out_raw, mag_raw = R.rope_fused(raw, cs, kind)
    rounded_first, _ = R.rope_fused(R.to_kind(raw, kind), cs, kind)
    assert (np.abs(out_raw - rounded_first) <= R.rope_bound(mag_raw, kind)).all()
    assert np.array_equal(R.rope_bound(np.array([0.0, 2.0]), kind), 4 * np.array([1e-2, 2.0]) * R.ULP[kind] + 1e-3)


def test_linear_int8_is_the_oracle_group_by_group():
    orc = load_oracle()
    rng = np.random.default_rng(7)
    f16 = rounder("f16")
    X, W, b = f16(rng.standard_normal((10, 128)).astype(F)), f16((rng.standard_normal((16, 128)) * 0.06).astype(F)), f16((rng.standard_normal(16) * 0.1).astype(F))
    X[7, 5] = 6.0                                                     # an outlier column in the second group only
    got = R.linear_int8(orc, X, W, b, 4)
    cb, scb = orc.quantize_rows(W)
    assert np.array_equal(got, np.concatenate([orc.linear_int8(X[r:r + 4], cb, scb, b) for r in (0, 4, 8)]))
    assert got.dtype == F and got.shape == (10, 16)
