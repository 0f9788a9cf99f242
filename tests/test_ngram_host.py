"""Shallow fusion, the host side (sonicscribe_amd/ngram.py): the automaton's reference arithmetic against a brute-force backoff model, the builders, the
packed form, every validation error by its message, the library's surface (options, header, the launch table's eight LM lines) and ASRModel's refusals.  No GPU.

Bound of the normalisation test: a score is a chain of at most order fp32 adds and one rounding per stored weight, (order + 1) roundings of 2^-24 relative on terms
of magnitude <= 30: about 2e-5 per score, so logsumexp over a state's scores is 0 within 1e-4."""
import math
import os
import re

import numpy as np
import pytest

import abi_pins
from sonicscribe_amd import asr, ngram
from sonicscribe_amd.ngram import BOS, NGramLM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def random_ngrams(rng, V, order, n_per_level=40):
    """a prefix-closed random backoff model: {ids: (logp, backoff)}"""
    grams = {(t,): (float(rng.uniform(-8, -1)), float(rng.uniform(-2, 0))) for t in range(V) if rng.random() < 0.8}
    level = list(grams)
    for L in range(2, order + 1):
        nxt = []
        for _ in range(n_per_level):
            if not level:
                break
            k = level[rng.integers(len(level))] + (int(rng.integers(V)),)
            grams[k] = (float(rng.uniform(-6, -0.1)), float(rng.uniform(-2, 0)) if L < order else 0.0)
            nxt.append(k)
        level = nxt
    return grams


def brute_logp(grams, hist, w, floor, order):
    """the textbook recursion over the dictionary, in the reference's fp32 operations: p(w | h) listed, else bo(h) + p(w | h[1:]); weights gathered from the
    longest context down, as the contract's A_j"""
    h = tuple(hist[-(order - 1):]) if order > 1 else ()
    ctxs = ngram_contexts(grams, order)
    while h not in ctxs:
        h = h[1:]
    A = F(0.0)
    while True:
        if h and h + (w,) in grams:
            return F(A + F(grams[h + (w,)][0]))
        if not h:
            return F(A + F(grams[(w,)][0] if (w,) in grams else floor))
        A = F(A + F(grams.get(h, (0.0, 0.0))[1]))
        h = h[1:]
        while h not in ctxs:
            h = h[1:]


def ngram_contexts(grams, order):
    c = {()}
    for k, (_, bo) in grams.items():
        if len(k) > 1:
            c.add(k[:-1])
        if bo != 0.0 and len(k) < order:
            c.add(k)
    return c


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_scores_and_step_against_brute_force(order):
    rng = np.random.default_rng(100 + order)
    V, floor = 24, -15.0
    grams = random_ngrams(rng, V, order)
    lm = NGramLM.from_ngrams(V, grams, floor=floor)
    real_order = max(len(k) for k in grams)
    assert lm.order == real_order <= order
    ctxs = sorted(ngram_contexts(grams, real_order), key=lambda c: (len(c), c))
    assert lm.n_nodes == len(ctxs)
    for _ in range(30):
        hist = [int(t) for t in rng.integers(0, V, size=rng.integers(0, 9))]
        state = lm.walk(hist)[0]
        h = tuple(hist[-(real_order - 1):]) if real_order > 1 else ()
        while h not in ctxs:                                    # the longest suffix of the history that is a context
            h = h[1:]
        assert state == ctxs.index(h), (hist, state, h)
        want = np.array([brute_logp(grams, hist, w, floor, real_order) for w in range(V)], np.float32)
        got = lm.scores(state, 1.0)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (hist, np.abs(got - want).max())
        lam = F(0.37)
        assert np.array_equal(lm.scores(state, 0.37).view(np.uint32), (lam * want).astype(np.float32).view(np.uint32))
        for w in (0, V - 1, int(rng.integers(V))):
            assert lm.logp(state, w) == float(want[w])
    assert lm.step(0, -1) == 0 and lm.step(lm.n_nodes - 1, V) == 0


@pytest.mark.parametrize("V", [16, 1000])
def test_from_corpus_every_state_sums_to_one(V):
    rng = np.random.default_rng(V)
    seqs = [rng.integers(0, min(V, 40), size=rng.integers(2, 25)).tolist() for _ in range(60)]
    lm = NGramLM.from_corpus(seqs, V, order=3, discount=0.75, eos_ids=[V - 1])
    assert lm.order == 3 and lm.n_nodes > 10
    worst = 0.0
    for n in range(lm.n_nodes):
        s = lm.scores(n, 1.0).astype(np.float64)
        worst = max(worst, abs(math.log(np.exp(s).sum())))
    print("worst |logsumexp|:", worst)
    assert worst <= 1e-4
    n, total = lm.walk(seqs[0] + [V - 1])
    assert 0 <= n < lm.n_nodes and total < 0 and math.isfinite(total)
    # a sequence of the corpus is more probable than a shuffle of ids the corpus never saw in that order
    assert total > lm.walk([V - 2] * (len(seqs[0]) + 1))[1]


ARPA = """
\\data\\
ngram 1=5
ngram 2=3

\\1-grams:
-1.0\t<unk>
-99\t<s>\t-0.5
-0.7\t</s>
-0.5\ta\t-0.3
-0.6\tb\t-0.2

\\2-grams:
-0.2\t<s> a
-0.3\ta b
-0.4\tb </s>

\\end\\
"""


def test_from_arpa():
    lm = NGramLM.from_arpa(ARPA, 8, token_id={"a": 1, "b": 2}, eos_ids=[6, 7], floor=-20.0)
    ln10 = math.log(10.0)
    assert lm.order == 2 and lm.n_nodes == 4 and lm.start == 1            # (), (<s>), (a), (b); decoding starts behind <s>
    assert lm.uni[1] == F(-0.5 * ln10) and lm.uni[6] == lm.uni[7] == F(-0.7 * ln10) and lm.uni[0] == F(-20.0)
    s = lm.scores(lm.start, 1.0)
    assert s[1] == F(F(0.0) + F(-0.2 * ln10)) and s[2] == F(F(-0.5 * ln10) + F(-0.6 * ln10))
    state, total = lm.walk([1, 2, 7])
    assert state == 0 and abs(total - (-0.2 - 0.3 - 0.4) * ln10) < 1e-5
    ids = NGramLM.from_arpa("\\data\\\n\\1-grams:\n-1 3 -0.1\n-1 4\n\\2-grams:\n-0.5 3 4\n\\end\\\n", 8)      # decimal ids
    assert ids.n_nodes == 2 and ids.step(0, 3) == 1 and ids.scores(1, 1.0)[4] == F(F(0.0) + F(-0.5 * ln10))
    with pytest.raises(ValueError, match="prefix"):
        NGramLM.from_arpa("\\data\\\n\\1-grams:\n-1 3\n\\2-grams:\n-0.5 4 3\n\\end\\\n", 8)
    with pytest.raises(ValueError, match="has no id"):
        NGramLM.from_arpa(ARPA, 8, token_id={"a": 1}, eos_ids=[6])


def small():
    return NGramLM.from_ngrams(8, {(1,): (-1.0, -0.5), (2,): (-2.0, -0.25), (1, 2): (-0.5, -0.125), (2, 1): (-0.75, 0.0), (1, 2, 3): (-0.1, 0.0), (3,): (-3.0, 0.0)})


def test_pack_round_trip():
    lm = small()
    w = lm.pack()
    V, N, E = lm.vocab, lm.n_nodes, lm.n_edges
    assert w.dtype == np.int32 and list(w[:5]) == [V, N, E, 3, 0] and len(w) == 5 + V + (N + 1) + 2 * N + 3 * E
    assert np.array_equal(w[5:5 + V], lm.uni.view(np.int32))
    back = NGramLM.unpack(w)
    assert np.array_equal(back.pack(), w)
    for n in range(N):
        assert np.array_equal(back.scores(n, 0.3).view(np.uint32), lm.scores(n, 0.3).view(np.uint32))
    assert lm.bo_next[0] == -1 and all(0 <= lm.bo_next[n] < n for n in range(1, N))
    r = slice(0, lm.node_off[1])
    assert np.array_equal(lm.edge_w[r].view(np.int32), lm.uni[lm.edge_tok[r]].view(np.int32))


def broken(**change):
    lm = small()
    f = dict(vocab=lm.vocab, order=lm.order, start=lm.start, uni=lm.uni.copy(), node_off=lm.node_off.copy(), bo_next=lm.bo_next.copy(), bo_w=lm.bo_w.copy(),
             edge_tok=lm.edge_tok.copy(), edge_next=lm.edge_next.copy(), edge_w=lm.edge_w.copy())
    for k, v in change.items():
        if isinstance(v, tuple):
            f[k][v[0]] = v[1]
        else:
            f[k] = v
    return NGramLM(**f)


@pytest.mark.parametrize("change,message", [
    (dict(order=9), "order 9 is outside 1 .. 8"),
    (dict(order=0), "order 0 is outside 1 .. 8"),
    (dict(start=99), r"start node 99 \(0 .. "),
    (dict(uni=(3, np.inf)), r"uni\[3\] is not finite"),
    (dict(node_off=(0, 1)), r"node_off\[0\] is 1, not 0"),
    (dict(node_off=(-1, 3)), "not the edge count"),
    (dict(node_off=(1, 99)), "node_off is not monotone at node 1"),
    (dict(bo_next=(0, 0)), r"bo_next\[0\] is 0, not -1"),
    (dict(bo_next=(1, 1)), r"bo_next\[1\] is 1 \(0 .. 0: nodes are numbered by context length\)"),
    (dict(order=2), r"the backoff chain of node \d+ has 2 links \(at most order - 1 = 1\)"),
    (dict(bo_w=(1, np.nan)), r"bo_w\[1\] is not finite"),
    (dict(edge_tok=(0, 8)), r"token id 8 is out of vocabulary \(8\)"),
    (dict(edge_tok=(1, 1)), "the edges of node 0 are not sorted and unique by token id"),
    (dict(edge_next=(0, 77)), r"an edge leads to node 77 \(0 .. "),
    (dict(edge_w=(3, -np.inf)), r"edge_w\[3\] is not finite"),
    (dict(edge_w=(0, -1.5)), r"root edge 0 \(token 1\) does not carry the bits of uni\[1\]"),
])
def test_every_validation_error_by_message(change, message):
    with pytest.raises(ValueError, match="lm: .*" + message):
        broken(**change)


def test_validation_of_the_model_and_the_words():
    with pytest.raises(ValueError, match="the automaton's vocabulary is 8, the model's 16"):
        small().validate(16)
    with pytest.raises(ValueError, match="do not hold the header"):
        NGramLM.unpack(np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="the header .* asks for"):
        NGramLM.unpack(small().pack()[:-1])
    with pytest.raises(ValueError, match="its prefix"):
        NGramLM.from_ngrams(8, {(1,): (-1.0, 0.0), (2, 1): (-1.0, 0.0)})
    with pytest.raises(ValueError, match="out of vocabulary"):
        NGramLM.from_ngrams(8, {(9,): (-1.0, 0.0)})
    assert NGramLM.from_ngrams(8, {(1,): (-1.0, 0.0), (BOS, 1): (-0.5, 0.0)}).start == 1
    # the library states the same rules in the same words
    src = open(os.path.join(abi_pins.CSRC, "engine_generation.cpp")).read()
    for words in ("order %d is outside 1 .. %d", "bo_next[0] is %d, not -1 (node 0 is the root)", "the backoff chain of node %d has %d links (at most order - 1 = %d)",
                  "the edges of node %d are not sorted and unique by token id", "root edge %d (token %d) does not carry the bits of uni[%d]", "is in use: option lm of %d handle"):
        assert words in src, words


def test_surface_and_launch_table():
    abi_pins.check_surface(options=("lm", "lm_weight"), header_strings=('"lm:<id>"', "lm_weight", "hook_lm_state", "hook_lm_tok", "hook_lm_weight", '"lm.hook:<V>"', "DESIGN.md 6.15"),
                           engine_methods=("lm_create", "set_lm", "test_lm_step", "test_greedy_lm"))
    k = open(os.path.join(abi_pins.CSRC, "greedy.hip")).read()
    lines = re.findall(r"greedy_launch<true,\s+true,\s+(true|false),\s+(true|false),\s+(true|false),\s+false,\s+false,\s+true\s*>", k)
    assert len(lines) == 8 and len(set(lines)) == 8, "exactly the eight LP + GUARD families without GRAMMAR carry LM: with and without BIAS, SAMPLE and TOPK"
    assert "lm.hip" in open(os.path.join(abi_pins.CSRC, "Makefile")).read()
    from sonicscribe_amd import engine
    assert "lm" not in engine.MIRRORED_OPTIONS and "lm_weight" not in engine.MIRRORED_OPTIONS
    assert engine.weight_bits(0.3) == int(np.array([0.3], np.float32).view(np.int32)[0])


def test_the_library_refuses_by_name():
    """the engine's refusals, where they are made: lm beside grammar and draft_verify (each way round), row forks, the bulk pipeline, token_logprobs, the splice, a
    destroy while a handle refers to the model; a scoring handle ignores the option (tests/test_gpu_lm.py runs every one of them on the device)"""
    gen = open(os.path.join(abi_pins.CSRC, "engine_generation.cpp")).read()
    for words in ('"lm: option grammar is on:', '"lm: option draft_verify is on:', '"grammar: option lm is on:', '"draft_verify: option lm is on:', '"request_forks: option lm is on:',
                  '"lm: option token_logprobs must be on first', 'opt = "lm";', 'opt = "lm_weight";', "is in use: option lm of %d handle"):
        assert words in gen, words
    assert re.search(r"lm_live\(const sonic_engine\* e\) \{ return [^}]*!e->opt_forced_parallel; \}", open(os.path.join(abi_pins.CSRC, "engine_internal.h")).read()), "a scoring handle ignores the option"
    assert "sonic_pipeline_create: option lm is on on a handle" in open(os.path.join(abi_pins.CSRC, "pipeline.cpp")).read()
    assert "token_logprobs cannot be switched off while option lm is on" in open(os.path.join(abi_pins.CSRC, "engine_options.cpp")).read()
    svc = open(os.path.join(abi_pins.CSRC, "engine_service.cpp")).read()
    assert "a.lm_d[d] = a.lm_s[s]; a.lm_d[64 + d] = a.lm_s[64 + s];" in svc, "splice_state_kernel moves the two words"
    for unit in ("engine_decode.cpp", "engine_stages.cpp", "engine_f32.cpp"):                     # lm_step right ahead of every production greedy launch
        text = open(os.path.join(abi_pins.CSRC, unit)).read()
        assert len(re.findall(r"lm_step\(e, \w+\);[^\n]*\n\s*launch_greedy\(", text)) == {"engine_decode.cpp": 3, "engine_stages.cpp": 1, "engine_f32.cpp": 1}[unit], unit


@pytest.mark.parametrize("kw,message", [
    (dict(token_logprobs=False), "lm= needs token_logprobs=True"),
    (dict(bulk=True), "lm is not supported with bulk=True"),
    (dict(grammar=True), "lm is not supported with grammar=True"),
    (dict(draft_verify=True), "lm is not supported with draft_verify=True"),
    (dict(sampling=True, best_of=2), "lm is not supported with best_of > 1"),
    (dict(lm_weight=-0.1), "lm_weight must be a finite number >= 0"),
    (dict(lm_weight=float("nan")), "lm_weight must be a finite number >= 0"),
    (dict(lm=3), "lm= takes an ngram.NGramLM or the path of an ARPA file"),
])
def test_every_python_refusal(kw, message):
    args = dict(token_logprobs=True, lm=small())
    args.update(kw)
    with pytest.raises(ValueError, match=message):                 # ahead of any engine: no device is touched
        asr.ASRModel("<none>", **args)
    m = asr.ASRModel.__new__(asr.ASRModel)
    with pytest.raises(ValueError, match="lm_score needs a model built with lm="):
        m.lm_score([1, 2])
    m.lm = small()
    assert m.lm_score([1, 2, 3]) == m.lm.walk([1, 2, 3])[1]
    assert ngram.check_weight(0) == 0.0 and ngram.check_weight(0.3) == float(np.float32(0.3))
