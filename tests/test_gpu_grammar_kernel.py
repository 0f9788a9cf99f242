"""The GRAMMAR instantiations of the greedy kernel (csrc/greedy.hip, option grammar) through the guard / bias / sample hooks with an armed automaton (Engine.test_greedy_grammar), in the handle's own type:
bf16, fp16 and the fp32 kind.

Contract: a row at node n >= 0 of its automaton sees every id that is not an edge token of n at -inf, behind the request bias and the repetition penalty, folded
into the guards' bans; a row at -2 sees everything but the EOS ids at -inf; a free row (-1) is the kernel without the flag.  Compare, log-probability, alternatives
and the Gumbel draw run over the masked scores.  The emitted id - argmax, draw or forced id - moves the state along its edge, or to -2 if the node has none.

Reference: NumPy forms the masked scores - reqbias.RequestBias.apply, genconfig.GenerationGuards.apply, grammar.Grammar.apply, held against HF's own processors by
tests/test_grammar_host.py - and Grammar.step the state.  Tokens, states, alternatives' ids and the raw dump must be equal; every log-probability lies within
DESIGN.md 6.3's derived bound (check_lp of test_gpu_request_bias.py) of float64 log_softmax over the masked scores.

Shapes: four rows per launch - a free row, a row at a node with one edge, a row at a node with about 2 000 edges (V / 2 at the small sizes), a row at -2 - at
V = 8 (fewer ids than threads), 1000 (a multiple of 4 and not of 32: the inverted map's last word has pad bits), 16388 (one id group past a full trip of the loop)
and 59264 (the production vocabulary); 1, 2 and 3 slabs."""
import numpy as np
import pytest

from gpu_common import SEED, check_lp, make_engine, same_bits, slabs
from sonicscribe_amd.genconfig import GenerationGuards
from sonicscribe_amd.grammar import Grammar
from sonicscribe_amd.reqbias import RequestBias
from test_gpu_request_bias import _histories  # noqa: E402
from test_gpu_sampling_kernel import bf16_exact, select  # noqa: E402
from test_gpu_top_logprobs_kernel import check_alternatives  # noqa: E402

pytestmark = pytest.mark.gpu
B = 4
NEG = np.float32("-inf")
SIZES = (8, 1000, 16388, 59264)
SHAPES = pytest.mark.parametrize("V", SIZES)
MODES = pytest.mark.parametrize("mode", [0, 2, 3], ids=["bf16", "f16", "f32"])
STATES = np.array([-1, 0, 1, -2], np.int32)
GUARDS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)


@pytest.fixture(scope="module")
def engines():
    es = {}

    def get(mode, topk=0):
        if mode not in es:
            es[mode] = make_engine(mode=mode, max_batch=B)                 # the hook takes everything but top_logprobs as arguments
            es[mode].set_option("token_logprobs", 1)
        es[mode].set_option("top_logprobs", topk)
        return es[mode]
    yield get
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def cases():
    """per V, computed once and left unchanged: the automaton, its EOS ids, the raw rows, the histories"""
    memo = {}

    def get(V):
        if V not in memo:
            rng = np.random.default_rng(SEED + V)
            eos = sorted([V - 1, 3])
            one = 5 if V == 8 else 12                                      # node 0's only edge: an id no history holds
            pool = np.setdiff1d(np.arange(V), eos)
            kids = np.sort(rng.choice(np.setdiff1d(pool, [0, one]), min(2000, V // 2 - 1), replace=False))
            # node 0: {one -> 1}; node 1: the children, leading to 2 and 0 in turn (a bisection that lands one edge off shows in the state); node 2: the EOS loops
            off = [0, 1, 1 + len(kids), 1 + len(kids) + 2]
            tok = [one] + [int(k) for k in kids] + eos
            nxt = [1] + [2 if i % 2 else 0 for i in range(len(kids))] + [2, 2]
            g = Grammar(off, tok, nxt, eos_ids=eos, vocab=V)
            rows = [bf16_exact(rng.uniform(-4.0, 4.0, V)) for _ in range(B)]
            outside = [int(i) for i in np.setdiff1d(pool, np.append(kids, one))]      # ids no state allows; 0 is among them
            assert len(outside) >= 2 and outside[0] == 0
            for b in range(B):                                             # every row's raw maximum is an id no state allows
                rows[b][outside[b % len(outside)]] = np.float32(6.0)
            hist, hlen = _histories(V, rng)
            memo[V] = (g, eos, rows, hist, hlen, kids, outside, one)
        return memo[V]
    return get


def masked(g, eos, raw, hist, table, guards, state):
    s = table.apply(raw, hist) if table is not None else np.array(raw, np.float32)
    return g.apply(guards.apply(s, hist), int(state), eos)


def first_max(s):
    return 0 if np.isneginf(s).all() else int(np.argmax(s))


@MODES
@SHAPES
def test_masked_argmax_lp_and_state(engines, cases, V, mode):
    """guard and bias families: the token is the argmax of the masked chain, never the raw maximum, never an id >= V; the dump stays raw; lp within the bound;
    the state follows the emitted id's edge"""
    eng = engines(mode)
    g, eos, rows, hist, hlen, kids, outside, one = cases(V)
    guards = GenerationGuards(**GUARDS, suppress_tokens=[int(kids[1])])
    tables = [RequestBias([[[int(kids[0])], 1.5]]), None, RequestBias([[[int(kids[-1])], 0.75], [[outside[0]], 3.0]], bad_words_ids=[[int(kids[2])]]), RequestBias([[[eos[0]], 0.5]])]
    for ks in (1, 2, 3):
        s = slabs(rows, ks)
        for fam, tb in (("guard", None), ("bias", tables)):
            tok, raw, lp, _, so = eng.test_greedy_grammar(s, B, g, STATES, eos, hist=hist, hist_len=hlen, tables=tb, suppress_tokens=[int(kids[1])], **GUARDS)
            for b in range(B):
                assert same_bits(raw[b], rows[b]), "the dump is the raw logits"
                m = masked(g, eos, raw[b], hist[b, :hlen[b]], tb[b] if tb else None, guards, STATES[b])
                want = first_max(m)
                print(f"V={V} mode={mode} ks={ks} {fam} row {b}: state {STATES[b]} token {int(tok[b])} (reference {want}) -> state {int(so[b])}")
                assert int(tok[b]) == want and 0 <= int(tok[b]) < V, (fam, ks, b, int(tok[b]), want)
                dead = bool(np.isneginf(m).all())                          # (V = 8: the guards may leave a row nothing; it then emits token 0 and leaves)
                if STATES[b] != -1 and not dead:
                    assert int(tok[b]) in g.allowed(int(STATES[b]), eos) and int(tok[b]) != int(np.argmax(rows[b])), (fam, ks, b, "a raw maximum outside the grammar won")
                if not dead:
                    check_lp((fam, V, mode, ks, b), lp[b], m, tok[b])
                assert int(so[b]) == g.step(int(STATES[b]), int(tok[b])), (fam, ks, b, int(so[b]))
            assert int(so[0]) == -1 and int(so[1]) == 1 and int(so[3]) == -2 and int(tok[3]) in eos and (V == 8 or int(so[2]) in (0, 2))


@MODES
@SHAPES
def test_alternatives_over_the_masked_scores(engines, cases, V, mode):
    """TOPK families (K = 8): the alternatives are the best allowed ids; the row at the one-edge node has one entry, the row at -2 two"""
    eng = engines(mode, 8)
    g, eos, rows, hist, hlen, kids, outside, one = cases(V)
    guards = GenerationGuards(**GUARDS)
    tables = [None, RequestBias([[[one], -1.0]]), RequestBias([[[int(kids[1])], 2.0]]), None]
    for ks in (1, 2, 3):
        for fam, tb in (("guard", None), ("bias", tables)):
            tok, raw, lp, _, so = eng.test_greedy_grammar(slabs(rows, ks), B, g, STATES, eos, hist=hist, hist_len=hlen, tables=tb, **GUARDS)
            for b in range(B):
                m = masked(g, eos, raw[b], hist[b, :hlen[b]], tb[b] if tb else None, guards, STATES[b])
                check_alternatives((fam, V, mode, ks, b), m, lp.top_logprobs[b], lp.top_ids[b], 8)
                assert not np.isneginf(m).all(), "these guards leave every row an allowed id"
                assert int(lp.top_ids[b, 0]) == int(tok[b]) and same_bits(lp.top_logprobs[b, 0], lp.lp[b])
                assert int(so[b]) == g.step(int(STATES[b]), int(tok[b]))
            assert lp.top_ids[1].tolist() == [one] + [-1] * 7 and sorted(lp.top_ids[3, :2].tolist()) == eos and lp.top_ids[3, 2:].tolist() == [-1] * 6


@MODES
@SHAPES
def test_forced_ids_and_rows_with_every_allowed_id_banned(engines, cases, V, mode):
    eng = engines(mode)
    g, eos, rows, hist, hlen, kids, outside, one = cases(V)
    for ks in (1, 2, 3):
        s = slabs(rows, ks)
        # a forced id outside the grammar: the state is -2 and the id's masked score -inf; inside it: the edge is followed
        off = np.array([outside[0], outside[1], outside[0], int(kids[0])], np.int32)
        tok, raw, lp, _, so = eng.test_greedy_grammar(s, B, g, STATES, eos, hist=hist, hist_len=hlen, force_ids=off)
        assert tok.tolist() == off.tolist() and so.tolist() == [-1, -2, -2, -2] and np.isneginf(lp[1:]).all(), (tok, so, lp)
        check_lp(("forced free row", V, mode, ks), lp[0], GenerationGuards().apply(raw[0], hist[0, :hlen[0]]), off[0])
        mid = int(kids[len(kids) // 2])
        on = np.array([int(kids[0]), one, mid, eos[1]], np.int32)
        tok, raw, lp, _, so = eng.test_greedy_grammar(s, B, g, STATES, eos, hist=hist, hist_len=hlen, force_ids=on)
        assert tok.tolist() == on.tolist() and so.tolist() == [-1, 1, g.step(1, mid), -2] and g.step(1, mid) in (0, 2), (tok, so)
        for b in (1, 2, 3):
            check_lp(("forced inside", V, mode, ks, b), lp[b], masked(g, eos, raw[b], hist[b, :hlen[b]], None, GenerationGuards(), STATES[b]), on[b])
        # the guards ban every id the state allows: token 0 (the first of equal values), which has no edge: -2
        sup = [one] + eos
        assert g.allowed(0).tolist() == [one] and 0 not in eos
        tok, raw, lp, _, so = eng.test_greedy_grammar(s, B, g, np.array([0, 0, -2, -1], np.int32), eos, hist=hist, hist_len=hlen, suppress_tokens=sup)
        assert tok[:3].tolist() == [0, 0, 0] and so[:3].tolist() == [-2, -2, -2] and int(so[3]) == -1, (tok, so)
        m = GenerationGuards(suppress_tokens=sup).apply(raw[3], hist[3, :hlen[3]])
        assert int(tok[3]) == first_max(m)


@MODES
@SHAPES
def test_sampling_draws_from_the_masked_scores(engines, cases, V, mode):
    """SAMPLE families: the token is the first maximum of fdiv(masked, t) + noise on the noise the kernel reports; lp is over the masked scores at temperature 1"""
    eng = engines(mode)
    g, eos, rows, hist, hlen, kids, outside, one = cases(V)
    guards = GenerationGuards(**GUARDS)
    t, seeds, steps = [0.7, 1.0, 2.0, 0.5], [3, 0x123456789ABCDEF0, 17, 1], [0, 7, 1000, 2]
    tables = [None, None, RequestBias([[[int(kids[2])], 2.0]]), None]
    for ks in (1, 2, 3):
        for fam, tb in (("guard", None), ("bias", tables)):
            tok, raw, lp, noise, so = eng.test_greedy_grammar(slabs(rows, ks), B, g, STATES, eos, hist=hist, hist_len=hlen, tables=tb, samp=(t, seeds, steps), **GUARDS)
            for b in range(B):
                m = masked(g, eos, raw[b], hist[b, :hlen[b]], tb[b] if tb else None, guards, STATES[b])
                want, _ = select(m, t[b], noise[b])
                assert int(tok[b]) == want, (fam, ks, b, int(tok[b]), want)
                check_lp((fam, "sample", V, mode, ks, b), lp[b], m, tok[b])
                assert int(so[b]) == g.step(int(STATES[b]), int(tok[b]))


@MODES
def test_free_rows_give_the_bits_of_the_families_without_the_flag(engines, cases, mode):
    """all eight GRAMMAR families with every row free against their non-grammar families: tokens, raw dump, lp, alternatives and noise bit for bit; states stay -1"""
    V = 16388
    g, eos, rows, hist, hlen, kids, outside, one = cases(V)
    s = slabs(rows, 2)
    free = np.full(B, -1, np.int32)
    tables = [RequestBias([[[int(kids[0])], 1.5]]), None, RequestBias([[[7], 9.0]], bad_words_ids=[[int(np.argmax(rows[2]))]]), None]
    samp = ([0.7, 0.0, 2.0, 1.0], [3, 4, 5, 6], [0, 1, 2, 3])
    kw = dict(suppress_tokens=[int(np.argmax(rows[1]))], **GUARDS)
    for topk in (0, 8):
        eng = engines(mode, topk)
        for bias in (False, True):
            for sample in (False, True):
                tb = tables if bias else None
                tok, raw, lp, noise, so = eng.test_greedy_grammar(s, B, g, free, eos, hist=hist, hist_len=hlen, tables=tb, samp=samp if sample else None, **kw)
                if sample:
                    tok0, raw0, lp0, noise0 = eng.test_greedy_sample(s, B, *samp, hist=hist, hist_len=hlen, tables=tb, **kw)
                    assert same_bits(noise, noise0)
                elif bias:
                    tok0, raw0, lp0 = eng.test_greedy_bias(s, B, hist, hlen, tb, want_lp=True, **kw)
                else:
                    tok0, raw0, lp0 = eng.test_greedy_guard(s, B, hist, hlen, want_lp=True, **kw)
                tag = (mode, topk, bias, sample)
                assert np.array_equal(tok, tok0) and same_bits(raw, raw0) and so.tolist() == [-1] * B, tag
                if topk:
                    assert same_bits(lp.lp, lp0.lp) and same_bits(lp.top_logprobs, lp0.top_logprobs) and np.array_equal(lp.top_ids, lp0.top_ids), tag
                else:
                    assert same_bits(lp, lp0), tag
