"""The word-timestamp kernels (csrc/align.hip) through the hook: sonic_test_attention on an align handle runs align_probs / align_reduce / align_dtw
on caller data through production's descriptor (align_probs_args) - every head takes part, a sequence's audio run is all its Tk keys.  bf16, and fp16 on an
int8-mode handle.

  (a) M against the float64 restatement from the element-type inputs, held to the bound tests/align_ref.py derives (matrix_bound: gamma_128 on the dot product, the
      softmax terms, the normalisation scaled by 1 / std).  Thin columns (0 < std < 16 x the std's own error bound) are compared before the normalisation only
      (debug buffer align_probs); they are at most THIN_CAP of a case's columns (checked on the CPU by tests/test_align_host.py).
  (b) the returned t_n equals the restated fp32 DTW of the RETURNED M exactly
  (c) a planted alignment is recovered: t_n == f(n)
  (d) a sequence alone and as sequence 2 of 3: the same bits.  (The hook has one Tk per call; sequences of different audio length side by side are in
      tests/test_gpu_align.py, where a batch's requests have different audio.)
"""
import numpy as np
import pytest

import align_ref as R
from gpu_common import bits
from sonicscribe_amd import spec

pytestmark = pytest.mark.gpu
KINDS = {"bf16": 0, "f16": 1}      # engine mode: native (bf16), int8 (fp16 activations)


@pytest.fixture(scope="module", params=list(KINDS))
def handle(request):
    from sonicscribe_amd.engine import Engine
    e = Engine(spec.TINY, 0, KINDS[request.param], max_batch=4, max_ctx=512)
    e.set_option("forced_parallel", 1)
    e.set_option("forced_align", 1)
    yield request.param, e
    e.close()


@pytest.mark.parametrize("shape", R.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matrix_bound_and_dtw(handle, shape):
    kind, e = handle
    B, Tq, Tk, Hq, Hkv = shape
    q, k = R.kernel_data(shape, kind)
    M, t = e.test_align(q, k)
    P = e.debug_read("align_probs", Hq * B * Tq * Tk).reshape(Hq, B, Tq, Tk)
    worst = worst_p = 0.0
    for b in range(B):
        r = R.matrix_bound(q[b], k[b])
        assert r["thin_share"] <= R.THIN_CAP
        perr = np.abs(P[:, b].astype(np.float64) - r["p"])
        worst_p = max(worst_p, float((perr / r["p_bound"]).max()))
        ok = r["ok"]
        err = np.abs(M[b].astype(np.float64) - r["M"])
        exact = ok & (r["bound"] == 0)
        assert np.all(err[exact] == 0)                                        # one row / one key: z = 0 on both sides
        live = ok & (r["bound"] > 0)
        if live.any():
            worst = max(worst, float((err[live] / r["bound"][live]).max()))
        assert np.array_equal(t[b], R.times_of(M[b])), (shape, b)              # (b): the DTW of the returned matrix, exactly
        assert np.all(np.diff(t[b]) >= 0) and t[b].min() >= 0 and t[b].max() < Tk
    print(f"align {kind} {shape}: worst |M - M64| / bound = {worst:.2e}, worst |p - p64| / bound = {worst_p:.2e}")
    assert np.all(np.isfinite(M)) and worst <= 1.0 and worst_p <= 1.0


@pytest.mark.parametrize("Tq,Hq,Hkv", [(2, 2, 1), (17, 4, 2), (65, 2, 1)])
def test_planted_alignment(handle, Tq, Hq, Hkv):
    kind, e = handle
    q, k, f = R.planted(Tq, Hq, Hkv, kind)
    M, t = e.test_align(q, k)
    assert np.array_equal(t[0], f), (t[0], f)
    assert np.array_equal(t[0], R.times_of(M[0]))


def test_same_bits_alone_and_in_a_batch(handle):
    kind, e = handle
    q, k = R.kernel_data((3, 17, 65, 4, 2), kind, seed=11)
    M3, t3 = e.test_align(q, k)
    for b in range(3):
        M1, t1 = e.test_align(q[b:b + 1], k[b:b + 1])
        assert np.array_equal(bits(M1[0]), bits(M3[b])) and np.array_equal(t1[0], t3[b])
    q2 = np.stack([q[2], q[0], q[1]]); k2 = np.stack([k[2], k[0], k[1]])      # sequence 0 as sequence 2 of 3
    Mp, tp = e.test_align(q2, k2)
    assert np.array_equal(bits(Mp[1]), bits(M3[0])) and np.array_equal(tp[1], t3[0])


def test_hook_refusals(handle):
    from sonicscribe_amd.engine import SonicError
    kind, e = handle
    q, k = R.kernel_data((1, 2, 3, 2, 1), kind)
    with pytest.raises(SonicError, match="align hook: bad shape"):
        e.test_align(np.zeros((1, 2, 3, 128), np.float32), np.zeros((1, 3, 2, 128), np.float32))      # Hq = 3 is no multiple of Hkv = 2
    with pytest.raises(SonicError, match="align hook: hd = 128"):
        e.test_align(q[..., :64], k[..., :64])
