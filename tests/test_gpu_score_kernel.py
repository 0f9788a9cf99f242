"""rows_kernel<T, false, false, TOPK> (csrc/rows.hip) through the greedy log-probability hook on a handle with option forced_parallel on: the hook sums the slabs in
the greedy kernel's order, rounds them to the handle's element type - those values are the logits row the kernel reads, and `logits_out` returns them - and launches
one block per row.  The kernel returns log_softmax(row)[forced id] and, with option top_logprobs = K, the K best ids of the row with their log-probabilities.

Accuracy is asserted against the bound DERIVED for the kernel as written (the derivation is 6.3's with this kernel's per-thread element count): with
u = 2^-24, n_t = ceil(V / 16384) * 16 the elements one thread adds (16 per trip: two 16-byte loads of a 16-bit type, four of fp32; 1024 threads) and ref64 the float64
log-softmax of the very values the kernel read,

    |lp - ref64| <= (n_t + 3 * (ceil(n_t / 16) - 1) + 2 + 16 + 1 + 2.25 * ln V) * u + u * |ref64|

The tests print the worst observed error / bound (a report; DESIGN.md quotes it)."""
import math

import numpy as np
import pytest

from gpu_common import make_engine, ref_log_softmax, ref_logprob, score_bound, slabs

pytestmark = pytest.mark.gpu
KINDS = {"bf16": 0, "fp16": 2, "fp32": 3}


@pytest.fixture(scope="module", params=list(KINDS))
def eng(request):
    e = make_engine(mode=KINDS[request.param], max_batch=2, max_ctx=512, options=(("token_logprobs", 1), ("forced_parallel", 1)))
    e.kind = request.param
    yield e
    e.close()


def _rows(V, rng):
    """the issue's rows, each with its target: (row, target or a function of the rounded row)"""
    i = np.arange(V)
    rand = rng.uniform(-4, 4, V).astype(np.float32)
    spike = rng.uniform(-2, 2, V).astype(np.float32)
    sp = int(rng.integers(0, V))
    spike[sp] += 64.0
    equal = np.full(V, 1.5, np.float32)
    ramp = (-3.0 + i * np.float32(60.0 / 59264)).astype(np.float32)      # ascending: the maximum moves at every element (up to the element type's rounding)
    tied = rng.uniform(-2, 2, V).astype(np.float32)
    tied[[1, V // 2, V - 2, 3]] = 5.0                                   # four tied maxima in different threads: the order is by id
    return [("argmax", rand, None), ("id0", rand, 0), ("last", rand, V - 1), ("far", spike, (sp + V // 2) % V), ("equal", equal, V // 3),
            ("ramp", ramp, V // 2), ("tied", tied, V // 2)]


def _batch(V, B, seed):
    rng = np.random.default_rng(seed)
    kinds = _rows(V, rng)
    names, rows, tgt = [], [], []
    for b in range(B):
        n, r, t = kinds[b % len(kinds)]
        if b >= len(kinds):                                              # further rows: fresh random values under the same target rule
            r = (r + rng.uniform(-0.5, 0.5, V)).astype(np.float32) if n not in ("equal", "ramp", "tied") else r
        names.append(n); rows.append(r); tgt.append(t)
    return names, rows, tgt


def _run(e, V, B, ks, seed):
    names, rows, tgt = _batch(V, B, seed)
    mpad = (B + 15) // 16 * 16
    s = slabs(rows, ks, mpad)
    # the argmax target is taken on the values the kernel will read: a first pass returns them (targets are then fixed for the asserted pass)
    if any(t is None for t in tgt):
        _, lg0, _ = e.test_greedy_lp(s, B, force_ids=np.zeros(B, np.int32))
        tgt = [int(lg0[b].argmax()) if t is None else t for b, t in enumerate(tgt)]
    force = np.asarray(tgt, np.int32)
    tok, lg, lp = e.test_greedy_lp(s, B, force_ids=force)
    assert np.array_equal(tok, force)
    return names, force, lg, lp


@pytest.mark.parametrize("V", [8, 1000, 1024, 59264])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_bound(eng, V, B):
    eng.set_option("top_logprobs", 0)
    for ks in ((1, 3) if V <= 1024 else (2,)):
        names, force, lg, lp = _run(eng, V, B, ks, seed=V + B)
        assert lp.dtype == np.float32 and lp.shape == (B,) and np.all(np.isfinite(lp))
        ref = ref_logprob(lg, force)
        err = np.abs(lp.astype(np.float64) - ref)
        bound = score_bound(V, ref)
        print(f"score hook {eng.kind} V={V} B={B} ks={ks}: worst |lp - ref64| / bound = {(err / bound).max():.3f} (max err {err.max():.3e}, lp in [{lp.min():.3f}, {lp.max():.3f}])")
        assert np.all(err <= bound), (eng.kind, V, B, ks, float((err / bound).max()))
        for b, n in enumerate(names):
            if n == "equal":
                assert abs(float(lp[b]) + math.log(V)) <= score_bound(V, -math.log(V)), (V, lp[b])      # lp = -ln V within the bound
            if n == "far" and b < 7:
                assert ref[b] <= -60.0                                   # the target sits at least 60 below the maximum
            if n == "argmax":
                assert force[b] == lg[b].argmax()


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("V", [8, 1000, 59264])
def test_alternatives(eng, V, K):
    eng.set_option("top_logprobs", K)
    try:
        B = 7
        names, force, lg, sc = _run(eng, V, B, 1, seed=7 * V + K)
        lp, top_lp, top_ids = sc
        assert top_lp.shape == (B, K) and top_ids.shape == (B, K)
        ref = ref_log_softmax(lg)
        worst = 0.0
        for b in range(B):
            order = np.lexsort((np.arange(V), -lg[b].astype(np.float64)))[:K]       # (value descending, id ascending)
            assert np.array_equal(top_ids[b], order), (eng.kind, V, K, names[b], top_ids[b], order)
            err = np.abs(top_lp[b].astype(np.float64) - ref[b, order])
            bound = score_bound(V, ref[b, order])
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (eng.kind, V, K, names[b])
            assert abs(float(lp[b]) - ref[b, force[b]]) <= score_bound(V, ref[b, force[b]])
            hit = np.nonzero(top_ids[b] == force[b])[0]
            if hit.size:                                                 # a forced token that is among the alternatives carries the bits of [0]
                assert top_lp[b, hit[0]].view(np.uint32) == lp[b].view(np.uint32), (names[b], top_lp[b, hit[0]], lp[b])
        assert any(force[b] in top_ids[b] for b in range(B))
        if V > 8:
            t = names.index("tied")
            assert list(top_ids[t][:min(K, 4)]) == sorted([1, 3, V // 2, V - 2])[:min(K, 4)]      # tied values: by id
        print(f"score hook {eng.kind} V={V} K={K}: worst alternative |lp - ref64| / bound = {worst:.3f}")
    finally:
        eng.set_option("top_logprobs", 0)


@pytest.mark.parametrize("K", [0, 8])
def test_same_bits_whatever_the_batch(eng, K):
    """a row's record alone, as row 2 of 3 and as row 64 of 65: the same bits"""
    eng.set_option("top_logprobs", K)
    try:
        V = 1024
        rng = np.random.default_rng(5)
        row = rng.uniform(-4, 4, V).astype(np.float32)
        others = [rng.uniform(-4, 4, V).astype(np.float32) for _ in range(64)]
        t = 321

        def rec(rows, at):
            B = len(rows)
            force = np.full(B, 7, np.int32); force[at] = t
            _, _, out = eng.test_greedy_lp(slabs(rows, 1, (B + 15) // 16 * 16), B, force_ids=force)
            parts = [out] if K == 0 else list(out)
            return [np.ascontiguousarray(p[at]).reshape(-1).view(np.uint32) for p in parts]
        alone, of3, of65 = rec([row], 0), rec(others[:2] + [row], 2), rec(others + [row], 64)
        for a, b, c in zip(alone, of3, of65):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    finally:
        eng.set_option("top_logprobs", 0)


def test_hook_refusals(eng):
    from sonicscribe_amd.engine import SonicError
    s = np.zeros((1, 16, 8), np.float32)
    with pytest.raises(SonicError, match="forced"):
        eng.test_greedy_lp(s, 1)                                          # force_ids is required on this route
    with pytest.raises(SonicError, match="vocabulary"):
        eng.test_greedy_lp(s, 1, force_ids=np.array([8], np.int32))
