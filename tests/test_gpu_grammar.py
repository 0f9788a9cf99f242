"""Grammar-constrained decoding end to end at TINY dims (option grammar): every step's token is the argmax of the masked chain over that step's raw
step_logits; the transcript is a path of its grammar; the same bits on every scheduler; rows with different grammars and free rows side by side; off is off and
the refusals; HF generate(prefix_allowed_tokens_fn=...) on the CPU against the fp32 engine through an HF-written checkpoint.

The synthetic model's free-running transcript repeats one id (304 or 10, tests/golden/tiny_bf16.npz) and never ends: none of the grammars below contains it."""
import itertools

import numpy as np
import pytest

from gpu_common import SEED, check_lp, flags, load_golden, make_engine, prompt_for, same_bits, six
from sonicscribe_amd import spec, synth
from sonicscribe_amd.genconfig import GenerationGuards
from sonicscribe_amd.grammar import Grammar

pytestmark = pytest.mark.gpu
D = spec.TINY
EOS = list(D.eos_ids)
LEVELS = ([205, 411, 500], [206, 412, 501], [207, 413, 502], [208, 414, 503], [209, 415, 504])


def grammar_a():
    """243 five-token transcripts, three choices at every step, then one of the EOS ids"""
    return Grammar.from_token_sequences([list(p) for p in itertools.product(*LEVELS)], EOS, vocab=D.vocab, audio_token_id=D.audio_token_id)


def grammar_b():
    """a phrase that is a prefix of another, one long phrase, one single token"""
    return Grammar.from_token_sequences([[600, 601], [600, 601, 602, 603], [610, 611, 612, 613, 614, 615, 616, 617], [620]], EOS, vocab=D.vocab, audio_token_id=D.audio_token_id)


def make(mode=0, max_batch=8, grammar=True, lp=True):
    return make_engine(D, mode, max_batch, 1024, flags((lp, "token_logprobs", 1), (grammar, "grammar", 1)))


def masked(raw, hist, g, state):
    s = GenerationGuards().apply(raw, hist)
    return s if g is None else g.apply(s, state, EOS)


def identity(ids, logits, prompts, grams, budgets, lps=None):
    """every row, every step: argmax(masked chain(dumped raw logits)) is the emitted id, the state walked by Grammar.step; the row ends on EOS or its budget"""
    for r in range(len(ids)):
        n, state = len(ids[r]), (0 if grams[r] is not None else -1)
        assert 1 <= n <= budgets[r] and (n == budgets[r] or int(ids[r][-1]) in EOS), (r, ids[r])
        for s in range(n):
            m = masked(logits[s, r], list(prompts[r]) + [int(t) for t in ids[r][:s]], grams[r], state)
            want = 0 if np.isneginf(m).all() else int(np.argmax(m))
            assert int(ids[r][s]) == want, (r, s, int(ids[r][s]), want)
            if lps is not None:
                check_lp(("e2e", r, s), lps[r][s], m, ids[r][s])
            if grams[r] is not None:
                state = grams[r].step(state, int(ids[r][s]))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g, segs, prompts = load_golden(golden_dir, int_prompts=True)
    return g, segs, prompts, int(g["n_new"])


# ------------------------------------------------------------------------------------------ 1. every step, every kind
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["bf16", "int8", "f16", "f32"])
def test_every_step_is_the_masked_argmax(golden, mode):
    _, segs, prompts, n_new = golden
    ga, gb = grammar_a(), grammar_b()
    e = make(mode=mode)
    try:
        da, db = e.grammar_create(ga), e.grammar_create(gb)
        plain, _ = e.transcribe_batch(segs, prompts, [n_new, n_new])
        assert ga.walk(plain[0]) == "left" and gb.walk(plain[1]) == "left", "the free-running transcripts follow neither grammar"
        ids, logits, lps = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True, want_logprobs=True, request_grammar=[da, db])
        identity(ids, logits, prompts, [ga, gb], [n_new, n_new], lps)
        print(f"mode {mode}: under the grammars {[i.tolist() for i in ids]} (free {plain[0][:3].tolist()} ..., {plain[1][:3].tolist()} ...)")
        assert ga.walk(ids[0]) == "accepted" and len(ids[0]) == 6 and gb.walk(ids[1]) == "accepted"
        # a budget that ends inside the grammar: incomplete; consumed: the next batch is free again
        short, lg = e.transcribe_batch(segs, prompts, [3, 1], want_logits=True, request_grammar=[da, db])
        identity(short, lg, prompts, [ga, gb], [3, 1])
        assert ga.walk(short[0]) == "incomplete" and np.array_equal(short[0], ids[0][:3]) and gb.walk(short[1]) in ("incomplete", "accepted")
        again, _ = e.transcribe_batch(segs, prompts, [n_new, n_new])
        assert all(np.array_equal(again[r], plain[r]) for r in range(2))
        # one constrained row beside a free one
        mixed, lg = e.transcribe_batch(segs, prompts, [n_new, 6], want_logits=True, request_grammar=[None, db])
        identity(mixed, lg, prompts, [None, gb], [n_new, 6])
        assert np.array_equal(mixed[0], plain[0]) and np.array_equal(mixed[1], ids[1][:6])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 2. the same bits on every path
def _six():
    return six() + ([9, 17, 11, 3, 13, 7],)


def test_invariance_all_paths():
    from sonicscribe_amd.dispatch import Dispatcher
    from sonicscribe_amd.grammar import CompiledGrammar
    segs, prompts, budgets = _six()
    ga, gb = grammar_a(), grammar_b()
    e = make(max_batch=8)
    try:
        ca, cb = CompiledGrammar(ga, [e]), CompiledGrammar(gb, [e])
        host = [ga, gb, None, ga, gb, None]                      # requests 3 (budget 3) ends inside its grammar
        comp = [ca, cb, None, ca, cb, None]
        dev = [None if c is None else c.on(e) for c in comp]
        plain = e.transcribe_batch(segs, prompts, budgets)[0]
        ids_e, logits_e, lp_e = e.transcribe_batch(segs, prompts, budgets, want_logits=True, want_logprobs=True, request_grammar=dev)      # one batch, eager
        identity(ids_e, logits_e, prompts, host, budgets, lp_e)
        st = [None if h is None else h.walk(ids_e[r]) for r, h in enumerate(host)]
        print("statuses", st, [i.tolist() for i in ids_e])
        assert st == ["accepted", "accepted", None, "incomplete", "accepted", None]
        for r in (2, 5):
            assert np.array_equal(ids_e[r], plain[r]), r
        ids_g, _, lp_g = e.transcribe_batch(segs, prompts, budgets, want_logprobs=True, request_grammar=dev)                               # one batch, hipGraph loop
        solo = [e.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]], want_logprobs=True, request_grammar=[dev[i]]) for i in range(6)]  # solo runs
        slot = e.slot()                                                                                                                     # a batch slot
        ids_s, _, lp_s = slot.transcribe_batch(segs, prompts, budgets, want_logprobs=True, request_grammar=dev)
        for r in range(6):
            assert np.array_equal(ids_g[r], ids_e[r]) and same_bits(lp_g[r], lp_e[r]), r
            assert np.array_equal(solo[r][0][0], ids_e[r]) and same_bits(solo[r][2][0], lp_e[r]), r
            assert np.array_equal(ids_s[r], ids_e[r]) and same_bits(lp_s[r], lp_e[r]), r
        slot.close()
        # prefill, then splice into a continuous handle: reference and state travel with the row.  Rows 0, 1, 2 of the loop are neighbours: grammar A, grammar B and a
        # free row; the second prefill's rows land beside them in another order than they were prefilled in
        pre = e.slot()
        e.service_begin()
        try:
            pre.stage_pcm(segs[:3]); pre.prefill(prompts[:3], budgets[:3], request_grammar=dev[:3])
            seq1 = e.splice_rows(pre, [0, 1, 2], [0, 1, 2])
            for _ in range(2):
                e.service_step(1, 8)
            pre.stage_pcm(segs[3:]); pre.prefill(prompts[3:], budgets[3:], request_grammar=dev[3:])
            seq = e.splice_rows(pre, [2, 0, 1], [3, 5, 4])
            rows, got = {0: 0, 1: 1, 2: 2, 3: 5, 5: 3, 4: 4}, {}
            for _ in range(300):
                fin, nn, s_, _ = e.service_step(1, 8)
                done = [r for r in rows if r not in got and s_ > max(seq, seq1) and fin[r]]
                if done:
                    a, b = e.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                    for r, x, y in zip(done, a, b):
                        got[r] = (x, y)
                if len(got) == 6:
                    break
            assert len(got) == 6
            for row, req in rows.items():
                assert np.array_equal(got[row][0], ids_e[req]) and same_bits(got[row][1], lp_e[req]), (row, req)
        finally:
            e.service_end()
            pre.close()
        # the Python dispatcher and the native one
        for native in (False, True):
            slots = [e.slot(), e.slot()]
            disp = Dispatcher([e], slots=[slots], continuous=True, native=native)
            assert type(disp.replicas[0]).__name__ == ("_NativeContinuousReplica" if native else "_ContinuousReplica")
            futs = [disp.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True, grammar=comp[i]) for i in range(6)]
            res = [f.result(timeout=120) for f in futs]
            disp.close()
            for s in slots:
                s.close()
            for i in range(6):
                assert np.array_equal(res[i][0], ids_e[i]) and same_bits(res[i][1], lp_e[i]), (native, i)
        # the batch dispatcher (no continuous loop)
        slots = [e.slot()]
        disp = Dispatcher([e], slots=[slots], continuous=False)
        res = [f.result(timeout=120) for f in [disp.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True, grammar=comp[i]) for i in range(6)]]
        disp.close()
        slots[0].close()
        for i in range(6):
            assert np.array_equal(res[i][0], ids_e[i]) and same_bits(res[i][1], lp_e[i]), ("batch dispatcher", i)
        ca.close(); cb.close()                                   # straight after the last result: every row that referred to them was fetched, handed over or has ended
    finally:
        e.close()


def test_model_entry_points_and_streams():
    """ASRModel: transcribe, submit, transcribe_batch (one grammar, one per audio) and the stream's submit calls give one request's ids on every entry point;
    detailed results and the debug dictionary carry grammar_status"""
    from sonicscribe_amd.asr import ASRModel
    m = ASRModel.from_synthetic(D, SEED, max_batch=8, max_ctx=1024, token_logprobs=True, grammar=True)
    try:
        ca, cb = m.compile_grammar(grammar_a()), m.compile_grammar(grammar_b())
        with pytest.raises(ValueError, match="tokenizer"):
            m.compile_grammar(["turn left", "turn right"])
        pcm = synth.synth_pcm(10, 80000)
        wav = pcm.astype(np.float32) / 32768.0
        info = m.transcribe(wav, max_new_tokens=12, return_debug_info=True, grammar=ca)
        assert info["grammar_status"] == "accepted" and ca.grammar.walk(info["token_ids"]) == "accepted" and len(info["token_ids"]) == 6
        free = m.transcribe(wav, max_new_tokens=12, return_debug_info=True)
        assert "grammar_status" not in free and ca.grammar.walk(free["token_ids"]) == "left"
        det = m.submit(wav, max_new_tokens=12, detailed=True, grammar=ca).result(timeout=120)
        assert det.grammar_status == "accepted" and np.array_equal(det.token_ids, info["token_ids"]) and same_bits(det.token_logprobs, info["token_logprobs"])
        short = m.submit(wav, max_new_tokens=3, detailed=True, grammar=ca).result(timeout=120)
        assert short.grammar_status == "incomplete" and np.array_equal(short.token_ids, det.token_ids[:3])
        assert m.transcribe(wav, max_new_tokens=12, grammar=ca) == info["transcript"]
        both = m.transcribe_batch([wav, wav, wav], max_new_tokens=12, grammar=[ca, cb, None])
        assert both[0] == info["transcript"] and both[2] == free["transcript"] and both[1] == m.transcribe(wav, max_new_tokens=12, grammar=cb)
        assert m.transcribe_batch([wav, wav], max_new_tokens=12, grammar=ca) == [info["transcript"]] * 2
        with pytest.raises(ValueError, match="2 audios but 1 grammars"):
            m.transcribe_batch([wav, wav], grammar=[ca])
        with pytest.raises(ValueError, match="compile_grammar"):
            m.transcribe(wav, grammar=grammar_a())
        st = m.open_stream("s0")
        try:
            raw = pcm.tobytes()
            for o in range(0, len(raw), 2048):
                st.add_audio_chunk(raw[o:o + 2048])
            sd = st.submit_chunks(0, st.next_chunk_id - 1, max_new_tokens=12, detailed=True, grammar=ca).result(timeout=120)
            assert sd.grammar_status == "accepted" and ca.grammar.walk(sd.token_ids) == "accepted"
            assert np.array_equal(sd.token_ids, det.token_ids) and same_bits(sd.token_logprobs, det.token_logprobs), "the stream's decode is submit()'s, bit for bit"
            first, n = st.chunk_range_samples(0, st.next_chunk_id - 1)
            ss = st.submit_samples(first, n, max_new_tokens=12, detailed=True, grammar=ca).result(timeout=120)
            assert np.array_equal(ss.token_ids, sd.token_ids) and same_bits(ss.token_logprobs, sd.token_logprobs)
        finally:
            st.close()
        assert m.get_model_info()["grammar"] is True
    finally:
        m.close()
    off = ASRModel.from_synthetic(D, SEED, max_batch=4, max_ctx=1024, token_logprobs=True)
    try:
        with pytest.raises(ValueError, match="grammar=True"):
            off.compile_grammar(grammar_a())
        with pytest.raises(ValueError, match="grammar=True"):
            off.transcribe(np.zeros(16000, np.float32), grammar=object())
    finally:
        off.close()


# ------------------------------------------------------------------------------------------ 3. off is off; refusals; memory
def test_off_is_off_and_refusals(golden):
    import ctypes as C
    from sonicscribe_amd.dispatch import Dispatcher
    from sonicscribe_amd.engine import DispatchRequest, SonicError
    from sonicscribe_amd.grammar import CompiledGrammar
    g, segs, prompts, n_new = golden
    ga = grammar_a()
    off = make(grammar=False)
    other = make(max_batch=2)
    try:
        with pytest.raises(SonicError, match="token_logprobs"):                # the option needs the log-probability kernels
            nolp = make(grammar=False, lp=False, max_batch=2)
            try:
                nolp.set_option("grammar", 1)
            finally:
                nolp.close()
        a0 = off.memory_info()[0]
        got = off.transcribe_batch(segs, prompts, [n_new, n_new])[0]
        for si in range(2):                                                    # the parent's fixture ids
            assert np.array_equal(got[si], g[f"s{si}_new_ids"][:len(got[si])])
        da = off.grammar_create(ga)                                            # a grammar may exist without the option ...
        a1 = off.memory_info()[0]
        assert a1 - a0 == 4 * (2 + ga.n_nodes + 1 + 2 * ga.n_edges), "the grammar's device bytes are the owner's"
        with pytest.raises(SonicError, match="option grammar is off"):        # ... but no request may name it
            off.set_request_grammar([da, None])
        slots = [off.slot(), off.slot()]
        disp = Dispatcher([off], slots=[slots], continuous=True, native=True)
        ca = CompiledGrammar(ga, [off])
        with pytest.raises(ValueError, match="grammar"):
            disp.submit([segs[0]], prompts[0], 4, grammar=ca)
        rep = disp.replicas[0]                                                 # ... and the library's own answer, not only the Python check in front of it
        tk = C.c_int64(0)
        pcm = np.ascontiguousarray(segs[0], np.int16); offs = np.array([0, len(pcm)], np.int64); pr = np.ascontiguousarray(prompts[0], np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        submit = lambda i: rep.lib.sonic_dispatch_submit(rep.h, C.byref(DispatchRequest(host_pcm=vp(pcm), host_off=vp(offs), W=1, prompt_ids=vp(pr), prompt_len=len(pr),
                                                                                          max_new=4, grammar_id=i)), C.byref(tk))
        assert submit(da.id) == 1 and b"option grammar is off" in rep.lib.sonic_last_error(None)      # a live grammar, handles without the option
        disp.close()
        for s in slots:
            s.close()
        ca.close()
        # the option: refused while rows are running, memory from sonic_memory_info, copied by slots
        off.stage_pcm(segs[:1]); off.prefill(prompts[:1], [8])
        with pytest.raises(SonicError, match="running"):
            off.set_option("grammar", 1)
        off.decode_step(100)
        off.set_option("grammar", 1)
        a2 = off.memory_info()[0]
        print(f"grammar: sonic_memory_info grows by {a2 - a1} bytes (history {64 * 1024 * 4}, references and states {96 * 8})")
        assert a2 - a1 == 64 * 1024 * 4 + 96 * 8
        with pytest.raises(SonicError, match="token_logprobs cannot be switched off"):
            off.set_option("token_logprobs", 0)
        slots = [off.slot(), off.slot()]                                       # with the option on, the dispatcher looks the id up on its own weight owner
        disp = Dispatcher([off], slots=[slots], continuous=True, native=True)
        rep = disp.replicas[0]
        assert submit(999) == 1 and b"grammar: 999 is not a live grammar" in rep.lib.sonic_last_error(None)
        disp.close()
        for s in slots:
            s.close()
        # a grammar of another weight owner is refused, by the setter and by the dispatcher
        foreign = other.grammar_create(ga)
        with pytest.raises(SonicError, match="weight owner"):
            off.set_request_grammar([foreign, None])
        off.set_option("request_grammar_begin", 2)                             # ... and in the library: an id that names no live grammar of this owner
        with pytest.raises(SonicError, match="not a live grammar of this handle's weight owner"):
            off.set_option("request_grammar", (0 << 16) | 999)
        # validation in the library itself, by message
        lib = off.lib
        i32 = lambda *v: np.array(v, np.int32)

        def create(o, t, n, N=None, E=None):
            w = np.concatenate([[len(o) - 1 if N is None else N, len(t) if E is None else E], o, t, n]).astype(np.int32)
            return lib.sonic_load_tensor(off.h, b"grammar:77", vp(w), 2, (C.c_int64 * 1)(len(w)), 1)
        for msg, (o, t, n) in {b"node 0 has no edge": (i32(0, 0, 1), i32(5), i32(0)), b"audio placeholder": (i32(0, 1), i32(D.audio_token_id), i32(0)),
                               b"out of vocabulary": (i32(0, 1), i32(D.vocab), i32(0)), b"leads to node": (i32(0, 1), i32(5), i32(1)),
                               b"not sorted and unique": (i32(0, 2), i32(6, 6), i32(0, 0)), b"node_off[0] is 1": (i32(1, 1), i32(5), i32(0)),
                               b"not the edge count": (i32(0, 2), i32(5), i32(0)), b"not monotone": (i32(0, 2, 1, 3), i32(5, 6, 7), i32(0, 0, 0))}.items():
            rc = create(o, t, n)
            assert rc == 1 and msg in lib.sonic_last_error(None), (msg, lib.sonic_last_error(None))
        assert create(i32(0, 1), i32(5), i32(0), N=65537) == 1 and b"65537 nodes" in lib.sonic_last_error(None)
        assert create(i32(0, 1), i32(5), i32(0), E=1048577) == 1 and b"1048577 edges" in lib.sonic_last_error(None)
        assert create(i32(0, 1, 2), i32(5), i32(0), N=1) == 1 and b"words" in lib.sonic_last_error(None)           # a length that does not fit the counts
        w = np.zeros(4, np.float32)
        assert lib.sonic_load_tensor(off.h, b"grammar:77", vp(w), 0, (C.c_int64 * 1)(4), 1) == 1 and b"SONIC_DTYPE_I32" in lib.sonic_last_error(None)
        # grammars for one request, a batch of two: refused, and consumed
        off.set_request_grammar([da])
        with pytest.raises(SonicError, match="requests"):
            off.transcribe_batch(segs, prompts, [4, 4])
        ids, _ = off.transcribe_batch(segs, prompts, [n_new, n_new])
        for si in range(2):
            assert np.array_equal(ids[si], g[f"s{si}_new_ids"][:len(ids[si])])
        # destroy while in use: a staged request, then a running row, hold the grammar; the handle's next prefill lets go of it
        off.set_request_grammar([da, None])
        with pytest.raises(SonicError, match="in use"):
            da.close()
        off.stage_pcm(segs); off.prefill(prompts, [n_new, n_new])
        with pytest.raises(SonicError, match="in use"):
            da.close()
        off.decode_step(100)
        under = off.fetch_tokens(2, n_new)
        assert ga.walk(under[0]) == "accepted" and np.array_equal(under[1], g["s1_new_ids"][:len(under[1])])
        da.close()                                                             # the run has ended and its ids are fetched: the rows let go; straight after the result
        da = off.grammar_create(ga)
        # a scoring handle refuses staged grammars, and consumes them
        sc = off.slot()
        sc.set_option("forced_parallel", 1)
        sc.set_request_grammar([da])
        with pytest.raises(SonicError, match="grammars"):
            sc.score_batch([segs[0]], [prompts[0]], [[205, 206, EOS[0]]])
        lp0 = sc.score_batch([segs[0]], [prompts[0]], [[205, 206, EOS[0]]])[2][0]
        assert np.isfinite(lp0).all()
        sc.close()
        # a splice between handles whose options differ is refused, the message naming the option
        pre = off.slot()
        assert pre.grammar
        pre.set_option("grammar", 0)
        off.service_begin()
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [4])
        with pytest.raises(SonicError, match="option grammar"):
            off.splice_rows(pre, [0], [0])
        off.service_end()
        pre.decode_step(100)
        # a continuous loop: the spliced row holds the grammar until it is fetched
        pre.set_option("grammar", 1)
        off.service_begin()
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [n_new], request_grammar=[da])
        seq = off.splice_rows(pre, [0], [1])
        with pytest.raises(SonicError, match="in use"):
            da.close()
        for _ in range(300):
            fin, nn, s_, _ = off.service_step(1, 2)
            if s_ > seq and fin[1]:
                break
        row = off.fetch_row(1, int(nn[1]))
        assert np.array_equal(row, under[0])
        off.service_end()
        before = off.memory_info()[0]
        da.close()                                                             # fetched: released
        assert before - off.memory_info()[0] == a1 - a0
        pre.close()
        foreign.close()
    finally:
        off.close()
        other.close()


def test_bulk_refuses():
    from sonicscribe_amd.dispatch import Dispatcher
    from sonicscribe_amd.grammar import CompiledGrammar
    e = make(max_batch=32)                               # (a pipeline block holds 32 rows)
    try:
        slots = [e.slot(), e.slot()]
        bulk = Dispatcher([e], slots=[slots], bulk=True, decoders=1)
        c = CompiledGrammar(grammar_a(), [e])
        with pytest.raises(ValueError, match="bulk"):
            bulk.submit([synth.synth_pcm(1, 48000)], prompt_for(D, 48000), 4, grammar=c)
        bulk.close()
        c.close()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 4. live HF
def test_live_hf_generate_with_prefix_allowed_tokens_fn_vs_fp32_engine_through_checkpoint(tmp_path):
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    from tests import hf_helpers as G
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.engine import MODE_F32
    n_new = 12
    model, _ = G.build_tiny(torch.float32)
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    pcm = synth.synth_pcm(10, 80000)
    feats, mask = G.mel_case(G.feature_extractor(), pcm)
    ids = G.PROMPT_PREFIX + [D.audio_token_id] * spec.audio_token_count(int(mask.sum())) + G.PROMPT_SUFFIX
    input_ids = torch.tensor([ids], dtype=torch.long)
    kw = dict(input_ids=input_ids, input_features=torch.from_numpy(feats)[None], input_features_mask=torch.from_numpy(mask)[None].long(),
              attention_mask=torch.ones_like(input_ids), max_new_tokens=n_new, do_sample=False, return_dict_in_generate=True, output_scores=True)
    ga = grammar_a()
    with torch.no_grad():
        base = model.generate(**kw).sequences[0, len(ids):].tolist()
        gen = model.generate(**kw, prefix_allowed_tokens_fn=ga.prefix_allowed_tokens_fn(len(ids)))
    ref_ids = gen.sequences[0, len(ids):].numpy().astype(np.int32)
    scores = torch.stack([s[0] for s in gen.scores]).numpy()
    # chosen on the CPU: unconstrained, HF emits 304 at every step; under grammar A it emits 500 206 502 208 504 992, three allowed ids at every step, and the
    # smallest top-1 / top-2 margin among the allowed ids is 0.136 (step 2) - three orders of magnitude above the fp32 engine's distance from HF's fp32 logits
    state, margins = 0, []
    for n, t in enumerate(ref_ids):
        al = ga.allowed(state, EOS)
        assert np.isneginf(np.delete(scores[n], al)).all() and len(al) == 3
        v = np.sort(scores[n][al])
        margins.append(float(v[-1] - v[-2]))
        state = ga.step(state, int(t))
    print(f"live HF under grammar A: {ref_ids.tolist()} (unconstrained {base[:3]} ...), margins among the allowed ids {[round(x, 3) for x in margins]}")
    assert ga.walk(ref_ids) == "accepted" and ga.walk(base) == "left" and min(margins) > 1e-2, "no step may be excused"
    m = ASRModel(str(tmp_path), max_batch=2, max_ctx=1024, slots=1, continuous=False, _allow_synthetic_prompt=True, _engine_mode=MODE_F32, token_logprobs=True, grammar=True)
    try:
        c = m.compile_grammar(ga)
        got, _ = m.model.transcribe_batch([pcm], [ids], [n_new], request_grammar=[c.on(m.model)])
        assert np.array_equal(got[0], ref_ids), (got[0].tolist(), ref_ids.tolist())
        assert m.prompt.decode(got[0]) == m.prompt.decode(ref_ids)
    finally:
        m.close()
