"""Grammar-constrained decoding, host side (sonicscribe_amd/grammar.py): the builders and their validation, walk(), Grammar.apply inside the full
NumPy chain against HF's own LogitsProcessorList with PrefixConstrainedLogitsProcessor in it, the ABI surface, and the refusals the Python layer makes before any
engine exists.  Needs no GPU."""
import os
import re

import numpy as np
import pytest

import abi_pins
from sonicscribe_amd import engine, genconfig
from sonicscribe_amd.genconfig import GenerationGuards
from sonicscribe_amd.grammar import MAX_EDGES, MAX_NODES, CompiledGrammar, Grammar
from sonicscribe_amd.reqbias import RequestBias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = [2, 3]


def stub_encode(text):
    """a tokenizer without merges: a space joins the letter behind it (id + 100), every other character is its own id"""
    ids, lead = [], False
    for c in text:
        if c == " ":
            lead = True
            continue
        ids.append(ord(c) - 80 + (100 if lead else 0))
        lead = False
    return ids


# ------------------------------------------------------------------------------------------ builders
def test_a_phrase_that_is_a_prefix_of_another_may_end_or_go_on():
    g = Grammar.from_token_sequences([[5, 6], [5, 6, 7], [9]], EOS, vocab=64)
    assert g.allowed(0).tolist() == [5, 9]
    n = g.step(g.step(0, 5), 6)
    assert g.allowed(n).tolist() == [2, 3, 7]                      # end here (either EOS id) or go on
    assert g.walk([5, 6, 2]) == g.walk([5, 6, 7, 3]) == g.walk([9, 2]) == "accepted"
    assert g.walk([5, 6]) == g.walk([5]) == g.walk([]) == "incomplete"
    assert g.walk([5, 7]) == g.walk([6]) == g.walk([5, 2]) == g.walk([5, 6, 7, 7]) == "left"
    # every node has an edge: the node behind EOS loops on the EOS ids (a finished row never steps again)
    end = g.step(n, 2)
    assert g.allowed(end).tolist() == EOS and g.step(end, 3) == end
    assert g.eos_ids == (2, 3) and g.node_off[0] == 0 and g.node_off[-1] == g.n_edges
    for a, b in zip(g.node_off[:-1], g.node_off[1:]):
        assert b > a and np.all(np.diff(g.edge_tok[a:b]) > 0)


def test_states_outside_the_grammar():
    g = Grammar.from_token_sequences([[5, 6]], EOS)
    s = np.arange(8, dtype=np.float32)
    assert g.step(-1, 5) == -1 and g.step(-2, 2) == -2 and g.step(0, 4) == -2
    assert np.array_equal(g.apply(s, -1), s) and g.apply(s, -1) is not s
    left = g.apply(s, -2)
    assert np.isneginf(left[[0, 1, 4, 5, 6, 7]]).all() and left[2] == 2 and left[3] == 3
    assert np.isneginf(g.apply(s, -2, eos_ids=[7])[:7]).all()
    at0 = g.apply(s, 0)
    assert at0[5] == 5 and np.isneginf(np.delete(at0, 5)).all()


def test_from_phrases_and_repeat_determinisation():
    g = Grammar.from_phrases(["go", "go on", " Stop ", "go"], stub_encode, EOS, vocab=256)
    go, go_sp, on_sp, stop = stub_encode("go"), stub_encode(" go"), stub_encode(" on"), stub_encode("stop")
    assert g.walk(go + EOS[:1]) == g.walk(go_sp + EOS[1:]) == g.walk(stub_encode("go on") + [2]) == g.walk(stop + [2]) == "accepted"       # cleaned as hotwords are: stripped, lower-cased
    assert g.walk(go + go_sp + [2]) == "left" and g.walk(stub_encode("Stop")) == "left"
    r = Grammar.from_phrases(["go", "go on", "stop"], stub_encode, EOS, repeat=True, vocab=256)
    assert r.walk(go + go_sp + stub_encode(" stop") + go_sp + [2]) == "accepted"
    assert r.walk(go + go + [2]) == "left"                          # a following phrase takes its leading-space form
    assert r.walk(go_sp + on_sp + go_sp + on_sp + [3]) == "accepted"
    # behind "go" the space-initial "o" of " on" continues "go on", and a space-initial "g" / "s" starts the next phrase: one deterministic node holds all three
    n = 0
    for t in go:
        n = r.step(n, t)
    assert set(r.allowed(n).tolist()) == {2, 3, on_sp[0], go_sp[0], stub_encode(" stop")[0]}
    # "go on" then " on...": not a phrase in leading-space form
    assert r.walk(stub_encode("go on") + on_sp + [2]) == "left"
    for a, b in zip(r.node_off[:-1], r.node_off[1:]):
        assert b > a and np.all(np.diff(r.edge_tok[a:b]) > 0)


def test_validation_errors_name_the_cause():
    def bad(msg, *a, **k):
        with pytest.raises(ValueError, match=msg):
            Grammar(*a, **k)
    bad(r"node_off\[0\] is 1, not 0", [1, 2], [5, 6], [0, 0])
    bad(r"node_off\[1\] is 1, not the edge count 2", [0, 1], [5, 6], [0, 0])
    bad("not monotone at node 1", [0, 2, 1, 3], [5, 6, 7], [0, 0, 0])
    bad("node 1 has no edge", [0, 1, 1, 2], [5, 6], [0, 0])
    bad("token id 64 is out of vocabulary", [0, 1], [64], [0], vocab=64)
    bad("token id -1 is out of vocabulary", [0, 1], [-1], [0])
    bad("token id 7 is the audio placeholder", [0, 1], [7], [0], audio_token_id=7)
    bad(r"leads to node 1 \(0 \.\. 0\)", [0, 1], [5], [1])
    bad("edges of node 1 are not sorted and unique", [0, 1, 3], [5, 6, 6], [0, 0, 0])
    bad("edges of node 0 are not sorted and unique", [0, 2], [6, 5], [0, 0])
    bad("0 nodes", [0], [], [])
    bad(f"{MAX_NODES + 1} nodes", np.arange(MAX_NODES + 2), np.zeros(MAX_NODES + 1), np.zeros(MAX_NODES + 1))
    bad(f"{MAX_EDGES + 1} edges", [0, MAX_EDGES + 1], np.arange(MAX_EDGES + 1), np.zeros(MAX_EDGES + 1))
    Grammar([0, 2, 3], [5, 6, 5], [1, 0, 0])                        # an ascent ends with its node: 6 then 5 across a boundary is fine
    for msg, seqs, eos in [("no token sequences", [], EOS), ("an empty token sequence", [[]], EOS), ("holds the EOS id 2", [[5, 2]], EOS), ("at least one EOS id", [[5]], [])]:
        with pytest.raises(ValueError, match=msg):
            Grammar.from_token_sequences(seqs, eos)
    with pytest.raises(ValueError, match="no usable phrase"):
        Grammar.from_phrases(["  ", ""], stub_encode, EOS)
    with pytest.raises(ValueError, match=f"{MAX_NODES} nodes"):    # a cap broken by the builder raises too: 70 000 one-token phrases' worth of trie nodes
        Grammar.from_token_sequences([[10 + i // 300, 400 + i % 300, 1000 + i] for i in range(70000)], EOS)


# ------------------------------------------------------------------------------------------ the chain against HF
def bits_equal(a, b):
    """equal values, -0.0 counting as +0.0 (HF adds a mask of zeros: -0.0 + 0.0 = +0.0); no NaN on either side"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b)


@pytest.mark.parametrize("V", [64, 1024])
def test_chain_equals_hf_processor_list_with_prefix_constrained(V):
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(7 + V)
    seqs = [[int(t) for t in rng.integers(4, V, int(rng.integers(1, 6)))] for _ in range(40)] + [[5], [5, 9], [5, 9, 4]]
    g = Grammar.from_token_sequences(seqs, EOS, vocab=V)
    sb = {(5,): 6.0, (4, 5): -2.5, (9,): 3.0, (8, 4, 11): 5.0}
    bw = [[12], [4, 13], [9]]
    guards = GenerationGuards(1.5, 2, [14, 5])
    rb = RequestBias(sb, bw, EOS, vocab=V)
    checked = argmax_moved = 0
    for trial in range(48):
        scores = (rng.standard_normal(V) * 3).astype(np.float32)
        scores[rng.integers(0, V, 3)] = np.float32(-0.0)
        path = seqs[trial % len(seqs)]
        k = int(rng.integers(0, len(path) + 1))
        prompt = [int(t) for t in rng.integers(4, 14, 10)] + [8, 4]
        hist = prompt + path[:k]
        state = 0
        for t in path[:k]:
            state = g.step(state, t)
        assert state >= 0
        got = g.apply(guards.apply(rb.apply(scores, hist), hist), state)
        procs = lp.LogitsProcessorList([lp.SequenceBiasLogitsProcessor(dict(sb)), lp.RepetitionPenaltyLogitsProcessor(1.5), lp.NoRepeatNGramLogitsProcessor(2),
                                        lp.NoBadWordsLogitsProcessor(bw, eos_token_id=EOS), lp.PrefixConstrainedLogitsProcessor(g.prefix_allowed_tokens_fn(len(prompt)), 1),
                                        lp.SuppressTokensLogitsProcessor([14, 5])])
        want = procs(torch.tensor([hist]), torch.from_numpy(scores.copy())[None])[0].numpy()
        assert bits_equal(got, want), (trial, np.nonzero(got != want)[0][:8])
        if not np.isneginf(want).all():
            assert int(np.argmax(got)) == int(np.argmax(want)), trial
            argmax_moved += int(np.argmax(got)) != int(np.argmax(scores))
        else:
            assert np.isneginf(got).all()
        assert np.isneginf(got[np.setdiff1d(np.arange(V), g.allowed(state))]).all()
        checked += 1
    assert checked == 48 and argmax_moved >= 24, "the grammar was expected to move most rows' maximum"


def test_prefix_allowed_tokens_fn_follows_the_generated_ids():
    g = Grammar.from_token_sequences([[5, 6], [5, 7, 8]], EOS)
    fn = g.prefix_allowed_tokens_fn(3)
    assert fn(0, [1, 1, 1]) == [5] and fn(0, np.array([1, 1, 1, 5])) == [6, 7] and fn(0, [1, 1, 1, 5, 6]) == EOS
    assert fn(0, [1, 1, 1, 5, 6, 2]) == EOS                         # behind EOS: the EOS loops
    assert fn(0, [1, 1, 1, 6]) == EOS                               # left: only EOS remains, as a row at -2
    assert fn(0, [1, 1, 1, 6]) == g.allowed(-2).tolist() and g.prefix_allowed_tokens_fn(3, eos_ids=[9])(0, [1, 1, 1, 6]) == [9]


# ------------------------------------------------------------------------------------------ ABI surface and Python refusals
def test_abi_surface():
    """the feature adds no entry point (the header, the binding table and exports.map keep their names and the ABI its version: tests/abi_pins.py): a grammar is
    loaded as an int32 tensor and everything else is an option of the handle"""
    abi_pins.check_surface(options=("grammar", "request_grammar_begin", "request_grammar", "hook_grammar_state", "hook_grammar_eos"),
                           header_strings=("SONIC_DTYPE_I32 = 2", '"grammar:<id>"', '"grammar.hook:<V>"', "int32_t grammar_id;"), names=("sonic_dispatch_submit",))
    assert "grammar_id" in [f for f, _ in engine.DispatchRequest._fields_]
    assert engine.DTYPE_I32 == 2
    import test_binding_signatures
    assert test_binding_signatures.mismatches(engine.SIGNATURES) == []
    k = open(os.path.join(ROOT, "sonicscribe_amd", "csrc", "greedy.hip")).read()
    assert len(re.findall(r"greedy_launch<true,\s+true,\s+(?:true|false),\s+(?:true|false),\s+(?:true|false),\s+true\s*>", k)) == 8, "exactly the eight LP + GUARD families carry GRAMMAR"
    # the packed form the library takes
    g = Grammar.from_token_sequences([[5, 6]], EOS)
    w = engine.grammar_words(g)
    assert w.dtype == np.int32 and w[0] == g.n_nodes and w[1] == g.n_edges and len(w) == 2 + g.n_nodes + 1 + 2 * g.n_edges


def test_python_refusals_before_any_engine():
    from sonicscribe_amd.asr import ASRModel
    with pytest.raises(ValueError, match="grammar=True needs token_logprobs=True"):
        ASRModel("<none>", grammar=True)
    with pytest.raises(ValueError, match="grammar is not supported with bulk=True"):
        ASRModel("<none>", grammar=True, token_logprobs=True, bulk=True)
    for field, value in (("force_words_ids", [[5]]), ("constraints", [1]), ("prefix_allowed_tokens_fn", "fn")):
        with pytest.raises(ValueError, match=field + ".*compile_grammar"):
            genconfig.from_dict({field: value})

    class Root:
        made = 0

        def __init__(self):
            self.root = self

        def grammar_create(self, g):
            Root.made += 1

            class H:
                h = 1

                def close(s):
                    s.h = None
            return H()

    class Slot:
        def __init__(self, root):
            self.root = root
    a, b = Root(), Root()
    c = CompiledGrammar(Grammar.from_token_sequences([[5]], EOS), [a, Slot(a), b])
    assert Root.made == 2 and c.on(Slot(a)) is c.on(a) and c.on(b) is not c.on(a)
    with pytest.raises(ValueError, match="compiled for another model"):
        c.on(Root())
    c.close()
    with pytest.raises(ValueError, match="has been closed"):
        c.on(a)


def test_a_request_carries_its_grammar_through_the_python_schedulers():
    """dispatch.Request keeps the grammar; the batch scheduler states every batch's grammars on an engine with the option and resolves them on that engine"""
    from sonicscribe_amd import dispatch
    seen = []

    class Eng:
        max_batch, grammar = 4, True

        def __init__(self):
            self.root = self

        def transcribe_batch(self, segs, prompts, max_new, req_win=None, **kw):
            seen.append(kw.get("request_grammar"))
            return [np.array([5, 2], np.int32) for _ in prompts], None

    class CG:
        def on(self, engine):
            return ("handle", id(engine.root))
    e = Eng()
    r = dispatch._Replica(e, 0)
    try:
        f1, f2 = dispatch.Request([np.zeros(4, np.int16)], [1], 4, grammar=CG()), dispatch.Request([np.zeros(4, np.int16)], [1], 4)
        r._run([f1, f2])
        assert seen == [[("handle", id(e)), None]] and f1.future.result().tolist() == [5, 2]
    finally:
        r.close()
