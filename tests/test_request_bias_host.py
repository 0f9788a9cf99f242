"""Per-request sequence bias, host side (sonicscribe_amd/reqbias.py): RequestBias.apply against HF's own SequenceBiasLogitsProcessor and
NoBadWordsLogitsProcessor, bit for bit; the chain order against HF's LogitsProcessorList; caps and validation; the hotword policy; the ABI surface; the Python
statement of the continuous dispatcher with stub engines."""
import threading

import numpy as np
import pytest

import abi_pins
from gpu_common import bits
from sonicscribe_amd import engine, reqbias
from sonicscribe_amd.genconfig import GenerationGuards
from sonicscribe_amd.reqbias import RequestBias


def hf_bias(sequence_bias, bad_words, eos, scores, hist):
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    s = torch.from_numpy(np.array(scores, np.float32))[None]
    ids = torch.tensor([list(hist)], dtype=torch.long)
    if sequence_bias:
        s = lp.SequenceBiasLogitsProcessor(dict(sequence_bias) if isinstance(sequence_bias, dict) else sequence_bias)(ids, s)
    if bad_words:
        s = lp.NoBadWordsLogitsProcessor(bad_words, eos_token_id=list(eos))(ids, s)
    return s[0].numpy()


def order_triple():
    """three fp32 values below 16 whose sum depends on the order they are added in"""
    rng = np.random.default_rng(7)
    while True:
        a, b, c = rng.uniform(-16, 16, 3).astype(np.float32)
        if np.float32(np.float32(a + b) + c) != np.float32(np.float32(a + c) + b):
            return float(a), float(b), float(c)


CASES = {
    "length 1": (dict([((3,), 1.5), ((9,), -0.75), ((0,), 2.0)]), None, [5, 6]),
    "multi-token match": ({(5, 6, 3): 2.25}, None, [1, 5, 6]),
    "multi-token miss": ({(6, 5, 3): 2.25}, None, [1, 5, 6]),
    "match reaching into the prompt": ({(1, 2, 3, 4, 5, 6, 7): 3.0, (7,): 0.5}, None, [9, 1, 2, 3, 4, 5, 6]),
    "L == len": ({(5, 6, 3): 4.0}, None, [9, 5, 6]),                               # three ids against a history of three: the longest entry that counts
    "L == len + 1 is ignored": ({(5, 6, 3): 4.0}, None, [5, 6]),                  # the prefix (5, 6) fits the history; HF skips the entry all the same
    "L == len + 2 cannot fit": ({(5, 6, 3): 4.0}, None, [6]),
    "duplicates, the last wins": ([[[4, 3], 1.0], [[3], 2.0], [[4, 3], -5.0], [[3], 0.125]], None, [8, 4]),
    "bad word equal to [eos] is filtered": (None, [[2], [7], [4, 7]], [8, 4]),
    "bad word and positive bias on one token": ({(7,): 9.0, (4, 7): 3.0}, [[7]], [8, 4]),
    "bad multi-token and positive single": ({(7,): 9.0}, [[4, 7]], [8, 4]),
}


@pytest.mark.parametrize("V", [64, 1024])
@pytest.mark.parametrize("name", list(CASES))
def test_apply_equals_hf(name, V):
    sb, bw, hist = CASES[name]
    rng = np.random.default_rng(V)
    scores = rng.standard_normal(V).astype(np.float32) * 4
    scores[11] = -0.0; scores[12] = 0.0; scores[13] = -np.inf
    eos = [2]
    rb = RequestBias(sb, bw, eos, vocab=V)
    got = rb.apply(scores, hist)
    want = hf_bias(sb, bw, eos, scores, hist)
    assert np.array_equal(bits(got), bits(want)), name
    if name == "bad word equal to [eos] is filtered":
        assert np.isfinite(got[2]) and np.isneginf(got[7]) and (2,) not in dict(rb.entries)
    if name == "L == len + 1 is ignored":
        assert got[3] == scores[3]
    if name == "L == len":
        assert got[3] == np.float32(scores[3] + np.float32(4.0))
    if name == "duplicates, the last wins":
        assert [list(i) for i, _ in rb.entries] == [[4, 3], [3]] and [float(b) for _, b in rb.entries] == [-5.0, 0.125]
    # the packed arrays round-trip
    ids, off, b = rb.table()
    assert ids.dtype == np.int32 and off.dtype == np.int32 and b.dtype == np.float32 and off[0] == 0 and len(off) == len(rb) + 1 and len(ids) == off[-1]
    assert [tuple(ids[off[i]:off[i + 1]]) for i in range(len(rb))] == [i for i, _ in rb.entries]


@pytest.mark.parametrize("V", [64, 1024])
def test_order_of_the_sum_is_hf_s(V):
    a, b, c = order_triple()
    s1 = np.float32(np.float32(np.float32(0) + np.float32(a)) + np.float32(b)) + np.float32(c)
    s2 = np.float32(np.float32(np.float32(0) + np.float32(a)) + np.float32(c)) + np.float32(b)
    assert max(abs(a), abs(b), abs(c)) < 16 and np.float32(s1) != np.float32(s2)              # the test has teeth
    hist = [8, 4, 5]
    scores = np.zeros(V, np.float32)
    for sb in ([[[3], a], [[5, 3], b], [[4, 5, 3], c]], [[[3], a], [[4, 5, 3], c], [[5, 3], b]], [[[4, 5, 3], c], [[5, 3], b], [[3], a]]):
        got = RequestBias(sb).apply(scores, hist)
        want = hf_bias(sb, None, [], scores, hist)
        assert np.array_equal(bits(got), bits(want))
    assert RequestBias([[[3], a], [[5, 3], b], [[4, 5, 3], c]]).apply(scores, hist)[3] != RequestBias([[[3], a], [[4, 5, 3], c], [[5, 3], b]]).apply(scores, hist)[3]


@pytest.mark.parametrize("V", [64, 1024])
def test_chain_order_equals_hf_processor_list(V):
    torch = pytest.importorskip("torch")
    lp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(3 + V)
    sb = {(5,): 6.0, (4, 5): -2.5, (9,): 3.0, (8, 4, 11): 5.0}
    bw = [[12], [4, 13], [2]]
    guards = GenerationGuards(1.5, 2, [14, 15])
    for trial in range(8):
        scores = rng.standard_normal(V).astype(np.float32) * 3
        hist = [int(t) for t in rng.integers(3, 14, 12)] + [8, 4]
        rb = RequestBias(sb, bw, [2], vocab=V)
        got = guards.apply(rb.apply(scores, hist), hist)
        procs = lp.LogitsProcessorList([lp.SequenceBiasLogitsProcessor(dict(sb)), lp.RepetitionPenaltyLogitsProcessor(1.5), lp.NoRepeatNGramLogitsProcessor(2),
                                        lp.NoBadWordsLogitsProcessor(bw, eos_token_id=[2]), lp.SuppressTokensLogitsProcessor([14, 15])])
        want = procs(torch.tensor([hist]), torch.from_numpy(scores)[None])[0].numpy()
        assert np.array_equal(bits(got), bits(want)), trial
        # the penalty sees the BIASED score: the other order is another number
        other = rb.apply(guards.apply(scores, hist), hist)
        if trial == 0:
            assert not np.array_equal(bits(other), bits(got))


def test_caps_and_validation():
    RequestBias([[[1 + k], 1.0] for k in range(256)])
    RequestBias([[[1] * 8, 1.0]])
    for bad in (dict(sequence_bias=[[[1 + k], 1.0] for k in range(257)]), dict(sequence_bias=[[[1] * 9, 1.0]]), dict(bad_words_ids=[[1] * 9]),
                dict(sequence_bias=[[[k], 1.0] for k in range(200)], bad_words_ids=[[300 + k] for k in range(57)]),
                dict(sequence_bias=[[[1], float("inf")]]), dict(sequence_bias=[[[1], float("-inf")]]), dict(sequence_bias=[[[1], float("nan")]]),
                dict(sequence_bias=[[[1], 1e39]]), dict(sequence_bias=[[[], 1.0]]), dict(sequence_bias=[[[-1], 1.0]]), dict(sequence_bias=[[[1.5], 1.0]]),
                dict(sequence_bias=[[1, 1.0]]), dict(sequence_bias=[[[1]]]), dict(bad_words_ids=[[]]), dict(bad_words_ids=[3]), dict(bad_words_ids="ab"),
                dict(sequence_bias=[[[64], 1.0]], vocab=64), dict(bad_words_ids=[[3, 64]], vocab=64)):
        with pytest.raises(ValueError):
            RequestBias(**bad)
    with pytest.raises(ValueError, match="vocabulary"):
        RequestBias([[[70], 1.0]]).apply(np.zeros(64, np.float32), [1])
    assert not RequestBias() and len(RequestBias(bad_words_ids=[[2]], eos_ids=[2])) == 0
    a, b = RequestBias([[[1], 1.0], [[2, 3], 2.0]]), RequestBias([[[2, 3], 5.0]], [[1]])
    c = reqbias.combine(a, None, b)
    assert [list(i) for i, _ in c.entries] == [[1], [2, 3]] and np.isneginf(c.entries[0][1]) and float(c.entries[1][1]) == 5.0
    with pytest.raises(ValueError, match="256"):
        reqbias.combine(RequestBias([[[k], 1.0] for k in range(200)]), RequestBias([[[300 + k], 1.0] for k in range(57)]))


def test_hotword_policy_with_a_stub_tokenizer():
    vocab = {}

    def encode(text):           # one id per character pair; a leading space gives another first piece, as a sentencepiece / BPE tokenizer does
        return [vocab.setdefault(text[i:i + 2], 10 + len(vocab)) for i in range(0, len(text), 2)]
    ent = reqbias.hotword_entries(["  Kubernetes ", "kubernetes", "MI355X", "", "  "], 2.5, encode)
    a, b = encode("kubernetes"), encode(" kubernetes")
    c, d = encode("mi355x"), encode(" mi355x")
    want = []
    for ids in (a, b, c, d):
        for n in range(1, min(len(ids), 8) + 1):
            if ids[:n] not in want:
                want.append(ids[:n])
    assert [e[0] for e in ent] == want and all(e[1] == 2.5 for e in ent)
    assert reqbias.hotword_entries(["x"], 0.0, encode) == [] and reqbias.hotword_entries(None, 3.0, encode) == []
    long_ids = reqbias.hotword_entries(["abcdefghijklmnopqrstuvwxyz"], 1.0, encode)
    assert max(len(e[0]) for e in long_ids) == 8                                     # prefixes of 1 .. 8 tokens: never a longer entry, never a truncated one
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="hotword_boost"):
            reqbias.hotword_entries(["x"], bad, encode)
    RequestBias(ent)                                                                 # ... and the entries are a valid table


def test_abi_surface():
    abi_pins.check_surface(names=("sonic_set_request_bias", "sonic_dispatch_submit", "sonic_test_greedy_bias"),
                           header_strings=("const int32_t* seq_ids; const int32_t* seq_off; const float* bias; int32_t n_seq;",),      # the dispatcher's way: fields of sonic_dispatch_request
                           engine_methods=("set_request_bias", "test_greedy_bias"))
    assert [f for f, _ in engine.DispatchRequest._fields_][10:14] == ["seq_ids", "seq_off", "bias", "n_seq"]
    ids, off, b, req = engine.pack_request_bias([None, RequestBias([[[5, 6], 1.0], [[7], 2.0]]), RequestBias(), RequestBias(bad_words_ids=[[9]])])
    assert req.tolist() == [0, 0, 2, 2, 3] and off.tolist() == [0, 2, 3, 4] and ids.tolist() == [5, 6, 7, 9] and b[:2].tolist() == [1.0, 2.0] and np.isneginf(b[2])


class _StubEngine:
    """records what the continuous dispatcher does with a request's table"""
    max_batch, max_ctx = 4, 64
    request_bias = True

    def __init__(self, log, name):
        self.log, self.name, self.pending, self.rows, self.seq, self.bias_rows = log, name, None, {}, 0, None

    def set_option(self, k, v): pass
    def service_begin(self): pass
    def service_end(self): pass
    def stage_pcm(self, segs, req_win): self.staged = len(req_win) - 1

    def set_request_bias(self, tables):
        self.pending = list(tables)

    def prefill(self, prompts, max_new, req_win):
        self.log.append((self.name, [p[0] for p in prompts], self.pending))
        self.batch = [(p[0], b) for p, b in zip(prompts, self.pending or [None] * len(prompts))]
        self.pending = None                              # consumed

    def splice_rows(self, src, src_rows, dst_rows):
        for s, d in zip(src_rows, dst_rows):
            self.rows[d] = src.batch[s]
        self.seq += 1
        return self.seq

    def service_step(self, n, top):
        self.seq += 1
        fin = np.zeros(self.max_batch, np.int32); nn = np.ones(self.max_batch, np.int32)
        for r in self.rows:
            fin[r] = 1
        return fin, nn, self.seq, 0

    def fetch_row(self, row, n):
        tag, b = self.rows.pop(row)
        return np.array([tag, -1 if b is None else len(b)], np.int32)

    def fetch_rows(self, rows, ns):
        return [self.fetch_row(r, n) for r, n in zip(rows, ns)]


def test_continuous_replica_carries_the_table_with_its_request():
    from sonicscribe_amd.dispatch import Dispatcher, _BulkReplica, Request
    log = []
    dec, pre = _StubEngine(log, "dec"), _StubEngine(log, "pre")
    disp = Dispatcher([dec], slots=[[pre]], continuous=True, native=False)
    t1, t3 = RequestBias([[[5], 1.0]]), RequestBias([[[6], 1.0], [[7, 8], 2.0], [[9], 3.0]])
    futs = [disp.submit([np.zeros(16, np.int16)], [100 + i], 4, bias=b) for i, b in enumerate([t1, None, t3, None, None])]
    res = [f.result(timeout=30) for f in futs]
    disp.close()
    # every request's result names its own table (its length; -1: none reached its row)
    assert [r.tolist() for r in res] == [[100, 1], [101, -1], [102, 3], [103, -1], [104, -1]]
    for name, tags, tables in log:                       # per prefill: the tables in the batch's order, or no call at all for a batch without any
        if tables is None:
            assert all(t in (101, 103, 104) for t in tags)
        else:
            assert len(tables) == len(tags)
            for tag, tb in zip(tags, tables):
                assert tb is {100: t1, 102: t3}.get(tag)
    assert all(tables is not None for _, _, tables in log)      # a handle with the option is told every batch's tables, None for a request without one
    # a replica whose handles lack the option refuses at put(), naming it
    dec2, pre2 = _StubEngine([], "dec"), _StubEngine([], "pre")
    pre2.request_bias = False
    disp = Dispatcher([dec2], slots=[[pre2]], continuous=True, native=False)
    with pytest.raises(ValueError, match="request_bias"):
        disp.submit([np.zeros(16, np.int16)], [1], 4, bias=t1)
    disp.close()
    # the bulk replica refuses, naming bulk (put() only: no pipeline is built)
    bulk = _BulkReplica.__new__(_BulkReplica)
    bulk.cv, bulk.stop, bulk.q = threading.Condition(), False, []
    with pytest.raises(ValueError, match="bulk"):
        bulk.put(Request([np.zeros(16, np.int16)], [1], 4, bias=t1))
    bulk.put(Request([np.zeros(16, np.int16)], [1], 4))
    assert len(bulk.q) == 1


def test_genconfig_still_refuses_the_fields_in_a_file():
    from sonicscribe_amd import genconfig
    for cfg in ({"sequence_bias": [[[5], 1.0]]}, {"bad_words_ids": [[5]]}):
        with pytest.raises(ValueError, match=list(cfg)[0]):
            genconfig.from_dict(cfg)
