"""rows_kernel<T, CHOOSE, GUARD, TOPK> (csrc/rows.hip): the property the one kernel rests on - CHOOSE changes no arithmetic.  The same rows,
with planted exact ties of the maximum, go through the score route (the log-probability hook on a handle with option forced_parallel: CHOOSE = false) and through
the verify route with neutral guards (the guard hook with forced ids on a handle with option draft_verify: CHOOSE = true, GUARD = false).  Both hooks build the
logits row from the slabs in the same way, so the kernels read the same bits; the returned rows, and the 1 + 2K floats of every record, must then be the same
bits on both routes, and the verify route's token the row's first maximum."""
import numpy as np
import pytest

from gpu_common import make_engine, slabs
from test_gpu_draft_kernel import HLD, _case  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = {"bf16": 0, "fp16": 2}


@pytest.fixture(scope="module", params=list(KINDS))
def routes(request):
    out = []
    for option in ("forced_parallel", "draft_verify"):
        e = make_engine(mode=KINDS[request.param], max_batch=2, max_ctx=512, options=(("token_logprobs", 1), (option, 1)))
        e.kind = request.param
        out.append(e)
    yield out
    for e in out:
        e.close()


def _parts(sc, K):
    """the record's members: lp [B] alone, or with K > 0 lp, top_logprobs [B, K] and top_ids [B, K] (the id floats as int32: an exact image of their bits)"""
    return [sc] if K == 0 else list(sc)


@pytest.mark.parametrize("K", [0, 8])
@pytest.mark.parametrize("V", [8, 1004, 16388])
@pytest.mark.parametrize("B", [3, 65])
def test_choice_changes_no_arithmetic(routes, V, B, K):
    score, verify = routes
    for e in routes:
        e.set_option("top_logprobs", K)
    try:
        rows, _, _ = _case(V, B, seed=V + B)
        force = np.random.default_rng(V + B + 1).integers(0, V, B).astype(np.int32)
        hist, hlen = np.zeros((B, HLD), np.int32), np.zeros(B, np.int32)
        for ks in (1, 3):
            s = slabs(rows, ks, (B + 15) // 16 * 16)
            tok_s, raw_s, sc_s = score.test_greedy_lp(s, B, force_ids=force)
            tok_v, raw_v, sc_v = verify.test_greedy_guard(s, B, hist, hlen, force_ids=force, want_lp=True)
            assert np.array_equal(tok_s, force)
            assert np.array_equal(raw_s.view(np.uint32), raw_v.view(np.uint32)), (score.kind, V, B, ks, "the two routes read different rows")
            for b in range(B):
                assert int(tok_v[b]) == int(np.argmax(raw_v[b])), (score.kind, V, B, ks, b)      # the first maximum
            if B >= 3:
                assert int(tok_v[1]) == 1                                  # row 1: four tied maxima, the lowest id
            ps, pv = _parts(sc_s, K), _parts(sc_v, K)
            assert len(ps) == len(pv) == (1 if K == 0 else 3)
            for a, c in zip(ps, pv):
                a = np.ascontiguousarray(a); c = np.ascontiguousarray(c)
                assert a.dtype == c.dtype and a.shape == c.shape
                diff = np.flatnonzero(a.reshape(B, -1).view(np.uint32) != c.reshape(B, -1).view(np.uint32))
                assert diff.size == 0, (score.kind, V, B, ks, K, "records differ at", diff[:8])
    finally:
        for e in routes:
            e.set_option("top_logprobs", 0)
