"""Shallow fusion on the device (csrc/lm.hip lm_step_kernel, and the LM instantiations of csrc/greedy.hip; option lm) through the language-model hooks
(Engine.test_lm_step, Engine.test_greedy_lm), in the handle's own type: bf16, fp16 and the fp32 kind.

1. lm_step_kernel alone on random automata: states, pending tokens and vectors are BIT FOR BIT ngram.NGramLM's (step / scores) - the contract fixes every fp32
   operation and its order.  V = 8 (fewer ids than threads), 1000 (a multiple of 4, not of 4096), 16388 (one group past a full trip of 4096 ids) and 59264 (the
   production vocabulary); order 1 (the root only), 2 and 4.  The automata hold nodes without edges, one node of about 2 000 edges (V - 1 at the small sizes: the 64-ary
   search's wide passes and its last probe) and chains of full depth.  Four rows per launch; the pending tokens hit at the row's node, after one backoff, after two,
   miss down to the root, and lie outside [0, V); rows without a pending token; a finished row, of which nothing is written.
2. the eight LM families at 1 - 3 slabs: the token is the argmax (or, sampling, the first maximum on the reported noise) of the numpy chain vector -> bias -> guards
   over the raw dump, the dump stays raw, log-probabilities and alternatives lie within the bounds test_gpu_logprobs.py / test_gpu_top_logprobs_kernel.py hold (the
   same sum over other scores), lm_tok holds the emitted id; at weight 0 every LM family gives its non-LM family's tokens, lp, alternatives and noise bit for bit."""
import numpy as np
import pytest

from gpu_common import SEED, check_lp, make_engine, same_bits, slabs
from sonicscribe_amd.genconfig import GenerationGuards
from sonicscribe_amd.ngram import NGramLM
from sonicscribe_amd.reqbias import RequestBias
from test_gpu_request_bias import _histories  # noqa: E402
from test_gpu_sampling_kernel import bf16_exact, select  # noqa: E402
from test_gpu_top_logprobs_kernel import check_alternatives  # noqa: E402

pytestmark = pytest.mark.gpu
B = 4
MODES = pytest.mark.parametrize("mode", [0, 2, 3], ids=["bf16", "f16", "f32"])
GUARDS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)


def automaton(V, order, seed=SEED):
    """a random prefix-closed backoff model -> NGramLM: about half of the listed unigrams are contexts without continuations (nodes with no edge), one context lists
    about 2 000 ids, and at order 4 three-token contexts give chains of full depth"""
    rng = np.random.default_rng(seed + 31 * V + order)
    w = lambda: float(rng.uniform(-9.0, -0.5))
    bo = lambda: float(rng.uniform(-2.0, -0.1))
    ids = np.arange(V) if V <= 1000 else np.sort(rng.choice(V, 3000, replace=False))
    grams = {(int(t),): (w(), bo() if order > 1 and rng.random() < 0.5 else 0.0) for t in ids}
    if order >= 2:
        big = int(ids[len(ids) // 3])
        for t in rng.choice(ids, min(2000, len(ids) - 1), replace=False):
            grams[(big, int(t))] = (w(), bo() if order > 2 and rng.random() < 0.3 else 0.0)
        level = [k for k in grams if len(k) == 2]
        for L in range(2, order + 1):
            nxt = [level[i] for i in rng.choice(len(level), min(len(level), 150), replace=False)] if L > 2 else [(int(a),) for a in rng.choice(ids, min(len(ids), 100), replace=False)]
            level = []
            for k in nxt:
                for t in rng.choice(ids, 3, replace=False):
                    key = k + (int(t),)
                    grams.setdefault(key, (w(), bo() if L < order and rng.random() < 0.5 else 0.0))
                    level.append(key)
    x = [int(t) for t in ids[:order]]                              # one chain of full depth: every suffix of x[:-1] is a context that lists the next id
    for a in range(order - 1):
        for b in range(a + 2, order + 1):
            grams.setdefault(tuple(x[a:b]), (w(), bo() if b - a < order else 0.0))
    return NGramLM.from_ngrams(V, grams, floor=-12.0)


def backoffs_until_hit(lm, n, t):
    """how many backoff links the transition of (n, t) follows before an edge lists t (None: it misses down to the root)"""
    k = 0
    while True:
        if lm._find(n, t) >= 0:
            return k
        if n == 0:
            return None
        n, k = int(lm.bo_next[n]), k + 1


def pending_cases(lm, rng):
    """(state, token) pairs by what the transition meets: a hit at the node, after one and two backoffs, a miss, a token outside the vocabulary, none pending"""
    found = {}
    N, V = lm.n_nodes, lm.vocab
    deep = [n for n in range(N) if len(lm.chain(n)[0]) == lm.order]                      # chains of full depth
    big = int(np.argmax(np.diff(lm.node_off)))
    for n in ([big] * 40 + deep[:200] + list(rng.integers(0, N, 400))):
        n = int(n)
        a, b = int(lm.node_off[n]), int(lm.node_off[n + 1])
        toks = [int(lm.edge_tok[i]) for i in (a, b - 1, (a + b) // 2)] if b > a else []  # first, last, middle edge of the node
        for c in lm.chain(n)[0][1:]:
            a2, b2 = int(lm.node_off[c]), int(lm.node_off[c + 1])
            if b2 > a2:
                toks.append(int(lm.edge_tok[int(rng.integers(a2, b2))]))
        toks += [int(t) for t in rng.integers(0, V, 3)]
        for t in toks:
            found.setdefault(backoffs_until_hit(lm, n, t), []).append((n, t))
    out = []
    for k in (0, 1, 2, None):
        out += [(k, n, t) for n, t in found.get(k, [])[:6]]
    out += [("outside", n, t) for n, t in ((N - 1, V), (0, V + 5), (big, V + 1000))]
    out += [("none", n, -1) for n in (0, N - 1, big, deep[0] if deep else 0)]
    return out


@pytest.fixture(scope="module")
def engines():
    es = {}

    def get(mode, topk=0):
        if mode not in es:
            es[mode] = make_engine(mode=mode, max_batch=B)
            es[mode].set_option("token_logprobs", 1)
        es[mode].set_option("top_logprobs", topk)
        return es[mode]
    yield get
    for e in es.values():
        e.arm_lm_hook(None)
        e.close()


# ------------------------------------------------------------------------------------------ 1. lm_step_kernel alone
@pytest.mark.parametrize("order", [1, 2, 4])
@pytest.mark.parametrize("V", [8, 1000, 16388, 59264])
def test_states_and_vectors_are_the_reference_bit_for_bit(engines, V, order):
    eng = engines(0)
    lm = automaton(V, order)
    rng = np.random.default_rng(V + order)
    cases = pending_cases(lm, rng)
    kinds = {c[0] for c in cases}
    width = np.diff(lm.node_off)
    print(f"V={V} order={order}: {lm.n_nodes} nodes ({int((width == 0).sum())} without edges, the widest {int(width.max())}), {lm.n_edges} edges, "
          f"deepest chain {max(len(lm.chain(n)[0]) for n in range(min(lm.n_nodes, 4000))) - 1} links; cases {sorted(map(str, kinds))}")
    assert lm.order == order and {"outside", "none"} <= kinds
    if order >= 2:
        assert (V == 8 or (width == 0).any()) and width.max() >= min(2000, V - 1) - 1 and 0 in kinds and (V == 8 or None in kinds)      # (V = 8: every id is a context, so none is without continuations and no token misses)
    if order == 4:
        assert {1, 2} <= kinds and any(len(lm.chain(n)[0]) == 4 for n in range(lm.n_nodes))
    eng.arm_lm_hook(lm)
    weights = (0.3, 1.0, 0.0, 2.5)
    for i in range(0, len(cases), B - 1):
        rows = cases[i:i + B - 1]
        rows = rows + [rows[0]] * (B - len(rows))                       # the last row of every launch is a finished copy of the first
        state = [r[1] for r in rows]
        tok = [r[2] for r in rows]
        fin = [0] * (B - 1) + [1]
        lam = weights[(i // (B - 1)) % len(weights)]
        so, to, add = eng.test_lm_step(B, state, tok, lam, finished=fin)
        for b in range(B):
            tag = (V, order, rows[b], lam, b)
            if fin[b]:
                assert int(so[b]) == state[b] and int(to[b]) == tok[b] and not add[b].any(), ("a finished row writes nothing", tag)
                continue
            want = lm.step(state[b], tok[b]) if tok[b] >= 0 else state[b]
            assert int(so[b]) == want and int(to[b]) == -1, (tag, int(so[b]), want, int(to[b]))
            assert same_bits(add[b], lm.scores(want, lam)), (tag, float(np.abs(add[b] - lm.scores(want, lam)).max()))


def test_the_hook_validates_as_the_load_does(engines):
    from sonicscribe_amd.engine import SonicError
    eng = engines(0)
    lm = automaton(8, 2)
    w = lm.pack()
    with pytest.raises(SonicError, match="the automaton's vocabulary is 8, the model's 16"):
        eng.arm_lm_hook(w, 16)
    bad = w.copy(); bad[3] = 9
    with pytest.raises(SonicError, match="order 9 is outside 1 .. 8"):
        eng.arm_lm_hook(bad, 8)
    bad = w.copy(); bad[5 + 8 + lm.n_nodes + 1] = 0                       # bo_next[0]
    with pytest.raises(SonicError, match=r"bo_next\[0\] is 0, not -1"):
        eng.arm_lm_hook(bad, 8)
    with pytest.raises(SonicError, match="arm a hook language model first"):
        eng.test_lm_step(B, [0] * B, [-1] * B, 0.5)


# ------------------------------------------------------------------------------------------ 2. the eight LM families
@pytest.fixture(scope="module")
def family_case():
    memo = {}

    def get(V):
        if V not in memo:
            rng = np.random.default_rng(SEED + V)
            lm = automaton(V, 4)
            rows = [bf16_exact(rng.uniform(-4.0, 4.0, V)) for _ in range(B)]
            hist, hlen = _histories(V, rng)
            deep = [n for n in range(lm.n_nodes) if len(lm.chain(n)[0]) == 4]
            states = [0, int(np.argmax(np.diff(lm.node_off))), deep[0], lm.n_nodes - 1]
            memo[V] = (lm, rows, hist, hlen, states)
        return memo[V]
    return get


def chain(raw, add, hist, table, guards):
    """numpy's processors in the kernel's order: the language model's vector first, then the request bias, then penalty and bans"""
    s = (np.asarray(raw, np.float32) + add).astype(np.float32)
    s = table.apply(s, hist) if table is not None else s
    return guards.apply(s, hist)


def first_max(s):
    return 0 if np.isneginf(s).all() else int(np.argmax(s))


@MODES
@pytest.mark.parametrize("V,slab_counts", [(8, (1,)), (16388, (1, 2, 3))])
def test_families_token_lp_alternatives_and_pending_token(engines, family_case, V, slab_counts, mode):
    lm, rows, hist, hlen, states = family_case(V)
    guards = GenerationGuards(**GUARDS)
    lam = 0.8
    listed = [int(t) for t in lm.edge_tok[lm.node_off[states[1]]:lm.node_off[states[1] + 1]][:3]]
    tables = [RequestBias([[[listed[0]], 1.5]]), None, RequestBias([[[listed[-1]], 0.75]], bad_words_ids=[[listed[1]]]), None]
    samp = ([0.7, 0.0, 2.0, 1.0], [3, 0x123456789ABCDEF0, 17, 1], [0, 7, 1000, 2])
    changed = 0
    for topk in (0, 8):
        eng = engines(mode, topk)
        for ks in slab_counts:
            s = slabs(rows, ks)
            for bias in (False, True):
                for sample in (False, True):
                    tb = tables if bias else None
                    tok, raw, lp, noise, add, pend = eng.test_greedy_lm(s, B, lm, states, lam, hist=hist, hist_len=hlen, tables=tb, samp=samp if sample else None, **GUARDS)
                    for b in range(B):
                        tag = (V, mode, topk, ks, bias, sample, b)
                        assert same_bits(raw[b], rows[b]), ("the dump is the raw logits", tag)
                        assert same_bits(add[b], lm.scores(states[b], lam)), tag
                        m = chain(raw[b], add[b], hist[b, :hlen[b]], tb[b] if tb else None, guards)
                        want = select(m, samp[0][b], noise[b])[0] if sample and samp[0][b] > 0 else first_max(m)
                        assert int(tok[b]) == want and int(pend[b]) == want, (tag, int(tok[b]), want, int(pend[b]))
                        changed += want != first_max(chain(raw[b], np.zeros(V, np.float32), hist[b, :hlen[b]], tb[b] if tb else None, guards))
                        if topk:
                            check_alternatives(tag, m, lp.top_logprobs[b], lp.top_ids[b], 8)
                            check_lp(tag, lp.lp[b], m, tok[b])
                        else:
                            check_lp(tag, lp[b], m, tok[b])
    assert changed > 0, "the vector moved no token: the test would pass without the add"


@MODES
def test_forced_id_is_scored_over_the_fused_scores_and_left_pending(engines, family_case, mode):
    V = 16388
    lm, rows, hist, hlen, states = family_case(V)
    eng = engines(mode)
    forced = np.array([5, int(lm.edge_tok[lm.node_off[states[1]]]), V - 1, 0], np.int32)
    tok, raw, lp, _, add, pend = eng.test_greedy_lm(slabs(rows, 2), B, lm, states, 1.25, hist=hist, hist_len=hlen, force_ids=forced)
    assert tok.tolist() == forced.tolist() == pend.tolist()
    for b in range(B):
        check_lp(("forced", mode, b), lp[b], chain(raw[b], add[b], hist[b, :hlen[b]], None, GenerationGuards()), forced[b])


@MODES
def test_weight_zero_gives_the_bits_of_the_families_without_the_flag(engines, family_case, mode):
    V = 16388
    lm, rows, hist, hlen, states = family_case(V)
    s = slabs(rows, 2)
    tables = [RequestBias([[[11], 1.5]]), None, RequestBias([[[7], 9.0]], bad_words_ids=[[int(np.argmax(rows[2]))]]), None]
    samp = ([0.7, 0.0, 2.0, 1.0], [3, 4, 5, 6], [0, 1, 2, 3])
    kw = dict(suppress_tokens=[int(np.argmax(rows[1]))], **GUARDS)
    for topk in (0, 8):
        eng = engines(mode, topk)
        for bias in (False, True):
            for sample in (False, True):
                tb = tables if bias else None
                tok, raw, lp, noise, add, pend = eng.test_greedy_lm(s, B, lm, states, 0.0, hist=hist, hist_len=hlen, tables=tb, samp=samp if sample else None, **kw)
                assert not add.any() and pend.tolist() == tok.tolist()
                if sample:
                    tok0, raw0, lp0, noise0 = eng.test_greedy_sample(s, B, *samp, hist=hist, hist_len=hlen, tables=tb, **kw)
                    assert same_bits(noise, noise0)
                elif bias:
                    tok0, raw0, lp0 = eng.test_greedy_bias(s, B, hist, hlen, tb, want_lp=True, **kw)
                else:
                    tok0, raw0, lp0 = eng.test_greedy_guard(s, B, hist, hlen, want_lp=True, **kw)
                tag = (mode, topk, bias, sample)
                assert np.array_equal(tok, tok0) and same_bits(raw, raw0), tag
                if topk:
                    assert same_bits(lp.lp, lp0.lp) and same_bits(lp.top_logprobs, lp0.top_logprobs) and np.array_equal(lp.top_ids, lp0.top_ids), tag
                else:
                    assert same_bits(lp, lp0), tag
