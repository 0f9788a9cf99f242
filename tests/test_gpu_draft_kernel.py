"""rows_kernel<T, true, GUARD, TOPK> (csrc/rows.hip) through the greedy guard hook on a handle with option draft_verify on: with forced ids the hook sums the
slabs in the greedy kernel's order, rounds them to the handle's element type - those values are the logits row the kernel reads, and `logits_out` returns them -
and launches one block per row.  Row b is one draft position: its history is hist[b][:hist_len[b]], its draft id force_ids[b].  The kernel returns the first maximum
of the processed scores and the record of the draft id: log_softmax(processed)[draft id] and, with option top_logprobs = K, the K best ids with their values.

The choice is exact: np.argmax(GenerationGuards.apply(row, history)), and the token greedy_kernel<T, ., true> picks for the same row on an ordinary handle.
The record is held to the row kernel's derived bound (tests/test_gpu_score_kernel.py), evaluated over the processed scores: the guards add no
term, since s * p, s / p (correctly rounded fp32) and -inf are the very values the float64 reference starts from."""
import numpy as np
import pytest

from gpu_common import flags, make_engine, ref_log_softmax, score_bound, slabs
from sonicscribe_amd.genconfig import GenerationGuards

pytestmark = pytest.mark.gpu
KINDS = {"bf16": 0, "fp16": 2}
HLD = 40
GUARDS = {"neutral": {}, "penalty": dict(repetition_penalty=1.5), "ngram1": dict(no_repeat_ngram_size=1), "ngram2": dict(no_repeat_ngram_size=2),
          "ngram3": dict(no_repeat_ngram_size=3), "suppress": dict(suppress_tokens=[5, 2]),
          "all3": dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[5, 2])}


@pytest.fixture(scope="module", params=list(KINDS))
def engs(request):
    out = []
    for draft in (1, 0):
        e = make_engine(mode=KINDS[request.param], max_batch=2, max_ctx=512, options=[("token_logprobs", 1)] + flags((draft, "draft_verify", 1)))
        e.kind = request.param
        out.append(e)
    yield out
    for e in out:
        e.close()


def _bf16(x):
    """fp32 values rounded to bf16 (RNE): exact in fp16 too at these magnitudes, so the bf16 greedy hook and a handle of either kind read the same rows"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)).view(np.float32)


def _case(V, B, seed):
    """rows with planted exact ties, histories of length 0, 1 (below n - 1 for n = 3), HLD (= hist_ld) and in between; repeats so that the n-gram rules bind"""
    rng = np.random.default_rng(seed)
    rows, hist, hlen = [], np.zeros((B, HLD), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        r = _bf16(rng.uniform(-4, 4, V).astype(np.float32))
        r[np.abs(r) < 2.0 ** -10] = 0.0                                  # (fp16 would round what lies below its normal range)
        if b % 3 == 1:                                                   # exact ties of the maximum in different threads: the lower id wins
            r[[1, V // 2, V - 2, 3]] = 5.0
        if b % 3 == 2:                                                   # ... and a tie that the penalty breaks: id 1 is in every history below
            r[[1, V - 1]] = 6.0
        rows.append(r)
        L = [0, 1, HLD, 7, 2][b % 5]
        pool = [1, 3, V // 2, 0]                                         # (never V - 1: row 2's unseen twin)
        h = [pool[int(i)] for i in rng.integers(0, len(pool), L)]
        if L >= 7:
            h[-2:] = [1, 3]; h[0:3] = [1, 3, V // 2]; h[3] = 3                     # (1, 3) -> V // 2 happened before: banned at n = 3; 3 -> V // 2, 3 -> x at n = 2
        hist[b, :L] = h; hlen[b] = L
    return rows, hist, hlen


def _check(engs, V, B, ks, gname, seed, K=0):
    ev, plain = engs
    guards = GUARDS[gname]
    g = GenerationGuards(**guards)
    rows, hist, hlen = _case(V, B, seed)
    mpad = (B + 15) // 16 * 16
    s = slabs(rows, ks, mpad)
    rng = np.random.default_rng(seed + 1)
    force = rng.integers(0, V, B).astype(np.int32)
    force[0] = 1                                                          # (a seen id on the rows that have a history)
    tok, raw, sc = ev.test_greedy_guard(s, B, hist, hlen, force_ids=force, want_lp=True, **guards)
    lp, top_lp, top_ids = (sc, None, None) if K == 0 else sc
    # the same rows through greedy_kernel<., true, true> on an ordinary handle (64 rows per launch; that hook launches the bf16 kernel whatever the handle: the rows
    # hold bf16 values, which fp16 represents exactly)
    for b0 in range(0, B, 64):
        n = min(64, B - b0)
        tok_g, raw_g, _ = plain.test_greedy_guard(slabs(rows[b0:b0 + n], ks, (n + 15) // 16 * 16), n, hist[b0:b0 + n], hlen[b0:b0 + n], want_lp=True, **guards)
        assert np.array_equal(raw_g.view(np.uint32), raw[b0:b0 + n].view(np.uint32)), "both kernels read the same rows"
        assert np.array_equal(tok_g, tok[b0:b0 + n]), (ev.kind, V, B, gname, "verify kernel and greedy kernel disagree")
    worst = 0.0
    for b in range(B):
        proc = g.apply(raw[b], hist[b, :hlen[b]])
        assert int(tok[b]) == int(np.argmax(proc)), (ev.kind, V, B, gname, b, int(tok[b]), int(np.argmax(proc)))
        ref = ref_log_softmax(proc)
        if np.isneginf(proc[force[b]]):
            assert np.isneginf(lp[b]), (gname, b, lp[b])
        else:
            err = abs(float(lp[b]) - ref[force[b]]); bound = score_bound(V, ref[force[b]])
            worst = max(worst, err / bound)
            assert np.isfinite(lp[b]) and err <= bound, (ev.kind, V, B, gname, b, float(lp[b]), ref[force[b]])
        if K:
            fin = np.flatnonzero(np.isfinite(proc))
            order = fin[np.lexsort((fin, -proc[fin].astype(np.float64)))][:K]                 # (value descending, id ascending) over the finite scores
            assert np.array_equal(top_ids[b][:len(order)], order), (ev.kind, V, K, gname, b, top_ids[b], order)
            assert int(top_ids[b][0]) == int(tok[b])                                        # alternative 0 is the choice
            assert np.all(top_ids[b][len(order):] == -1) and np.all(np.isneginf(top_lp[b][len(order):]))
            e2 = np.abs(top_lp[b][:len(order)].astype(np.float64) - ref[order])
            assert np.all(e2 <= score_bound(V, ref[order])), (ev.kind, V, K, gname, b)
            hit = np.nonzero(top_ids[b] == force[b])[0]
            if hit.size:                                                  # a draft id among the alternatives carries the bits of [0]
                assert top_lp[b, hit[0]].view(np.uint32) == lp[b].view(np.uint32)
    return tok, worst


@pytest.mark.parametrize("V", [8, 1000, 1024, 59264])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_choice_and_record(engs, V, B):
    engs[0].set_option("top_logprobs", 0); engs[1].set_option("top_logprobs", 0)
    names = list(GUARDS) if V * B <= 59264 * 3 else ["neutral", "all3"]
    for gname in names:
        for ks in ((1, 3) if V <= 1024 else (2,)):
            tok, worst = _check(engs, V, B, ks, gname, seed=V + B)
            print(f"verify hook {engs[0].kind} V={V} B={B} ks={ks} {gname}: worst |lp - ref64| / bound = {worst:.3f}")
            if B >= 3 and gname == "neutral":
                assert int(tok[1]) == 1                                   # four tied maxima: the lowest id
            if B >= 3 and gname == "penalty":
                assert int(tok[2]) == V - 1                               # row 2: ids 1 and V - 1 tie at 6.0; 1 is in its history (6.0 / 1.5), V - 1 is not


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("V", [8, 1000, 59264])
def test_alternatives(engs, V, K):
    for e in engs:
        e.set_option("top_logprobs", K)
    try:
        for gname in ("neutral", "all3"):
            _check(engs, V, 7, 1, gname, seed=7 * V + K, K=K)
    finally:
        for e in engs:
            e.set_option("top_logprobs", 0)


def test_every_id_banned_gives_token_zero(engs):
    ev = engs[0]
    V = 8
    rows = [np.linspace(-1, 1, V).astype(np.float32)]
    tok, raw, lp = ev.test_greedy_guard(slabs(rows, 1, 16), 1, np.zeros((1, HLD), np.int32), np.zeros(1, np.int32), force_ids=np.array([3], np.int32), want_lp=True,
                                        suppress_tokens=list(range(V)))
    assert int(tok[0]) == 0 and not np.isfinite(lp[0])                    # torch.argmax of equal values; no finite score to normalise by


def test_unaligned_rows_take_the_same_order(engs):
    """V * sizeof(T) not a multiple of 16: every second row starts off a 16-byte boundary and is read element by element, in the same visiting order - the record of
    a row is the same bits at an aligned and at an unaligned place"""
    ev = engs[0]
    V = 1004
    rng = np.random.default_rng(11)
    row = rng.uniform(-4, 4, V).astype(np.float32)
    rows = [row, row, row]
    hist = np.tile(np.arange(HLD, dtype=np.int32) % 7, (3, 1)); hlen = np.full(3, HLD, np.int32)
    force = np.full(3, 5, np.int32)
    tok, raw, lp = ev.test_greedy_guard(slabs(rows, 1, 16), 3, hist, hlen, force_ids=force, want_lp=True, **GUARDS["all3"])
    assert tok[0] == tok[1] == tok[2] and len(set(lp.view(np.uint32).tolist())) == 1
    proc = GenerationGuards(**GUARDS["all3"]).apply(raw[1], hist[1])
    assert int(tok[1]) == int(np.argmax(proc))


def test_same_bits_whatever_the_batch(engs):
    """a position's choice and record alone, as row 2 of 3 and as row 64 of 65: the same bits"""
    ev = engs[0]
    V = 1024
    rng = np.random.default_rng(5)
    row = rng.uniform(-4, 4, V).astype(np.float32)
    others = [rng.uniform(-4, 4, V).astype(np.float32) for _ in range(64)]
    h = (np.arange(HLD, dtype=np.int32) * 37) % V

    def rec(rows, at):
        B = len(rows)
        hist = np.zeros((B, HLD), np.int32); hlen = np.zeros(B, np.int32)
        hist[at] = h; hlen[at] = HLD
        force = np.full(B, 7, np.int32); force[at] = 321
        tok, _, lp = ev.test_greedy_guard(slabs(rows, 1, (B + 15) // 16 * 16), B, hist, hlen, force_ids=force, want_lp=True, **GUARDS["all3"])
        return int(tok[at]), int(lp[at:at + 1].view(np.uint32)[0])
    assert rec([row], 0) == rec(others[:2] + [row], 2) == rec(others + [row], 64)


def test_hook_refusals(engs):
    from sonicscribe_amd.engine import SonicError
    s = np.zeros((1, 16, 8), np.float32)
    with pytest.raises(SonicError, match="vocabulary"):
        engs[0].test_greedy_guard(s, 1, np.zeros((1, 4), np.int32), np.zeros(1, np.int32), force_ids=np.array([8], np.int32), want_lp=True)
    with pytest.raises(SonicError, match="history length"):
        engs[0].test_greedy_guard(s, 1, np.zeros((1, 4), np.int32), np.array([5], np.int32), force_ids=np.array([1], np.int32), want_lp=True)
