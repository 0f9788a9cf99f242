"""Shallow fusion end to end at TINY dims (options lm / lm_weight): every step's token is the argmax of raw step logits + the reference's vector at the
reference's state; the same bits solo, in a batch, on a slot, spliced into a continuous loop beside rows at other states, through both dispatchers and a stream; a
sharply peaked model at a large weight pulls the transcript onto its sequence; off is off; the refusals; HF generate(logits_processor=...) on the CPU against the fp32
kind.

The synthetic model's free-running transcript repeats one id (304 or 10, tests/golden/tiny_bf16.npz) and never ends."""
import numpy as np
import pytest

from gpu_common import SEED, check_lp, load_golden, make_engine, same_bits, six
from sonicscribe_amd import spec, synth
from sonicscribe_amd.ngram import NGramLM

pytestmark = pytest.mark.gpu
D = spec.TINY
EOS = list(D.eos_ids)
PATH = [205, 411, 500, 206, 412, EOS[0]]


def peaked():
    """a bigram model that all but dictates PATH: the listed continuation at -0.01, everything else three nats of backoff and more below it"""
    grams = {(t,): (-5.0, -3.0) for t in PATH}
    grams[(PATH[0],)] = (-0.01, -3.0)
    for a, b in zip(PATH, PATH[1:]):
        grams[(a, b)] = (-0.01, 0.0)
    return NGramLM.from_ngrams(D.vocab, grams, floor=-20.0)


def forked():
    """two dictated paths behind the model's own first choice, 304 or 10 (equal under the language model); the one behind 304 is longer than most budgets below, so
    rows end at different nodes and are in the middle of it when others are spliced in beside them"""
    a, b = [304, 411, 500, 206, 412, 207, 413, 501, 208, 414, 502, 209, EOS[0]], [10, 601, 602, 603, EOS[0]]
    grams = {(t,): (-5.0, -3.0) for t in a + b}
    grams[(304,)] = grams[(10,)] = (-0.01, -3.0)
    for p in (a, b):
        for x, y in zip(p, p[1:]):
            grams[(x, y)] = (-0.01, 0.0)
    return NGramLM.from_ngrams(D.vocab, grams, floor=-20.0)


def corpus_lm():
    """a trigram model over sequences that hold the free-running ids and their neighbours: it tilts near-ties without dictating anything"""
    rng = np.random.default_rng(SEED)
    pool = [304, 10, 305, 11, 303, 9, 205, 411]
    seqs = [[pool[i] for i in rng.integers(0, len(pool), size=rng.integers(3, 12))] for _ in range(80)]
    return NGramLM.from_corpus(seqs, D.vocab, order=3, eos_ids=EOS)


def make(mode=0, max_batch=8, lm=None, weight=0.0, lp=True):
    e = make_engine(D, mode, max_batch, 1024, [("token_logprobs", 1)] if lp else [])
    dev = None
    if lm is not None:
        dev = e.lm_create(lm)
        e.set_lm(dev, weight)
    return e, dev


def identity(lm, weight, ids, logits, budgets, lps=None):
    """every row, every step: argmax(raw + scores(state, weight)) is the emitted id, the state walked by NGramLM.step from the start node"""
    for r in range(len(ids)):
        n, state = len(ids[r]), lm.start
        assert 1 <= n <= budgets[r] and (n == budgets[r] or int(ids[r][-1]) in EOS), (r, ids[r])
        for s in range(n):
            m = (logits[s, r] + lm.scores(state, weight)).astype(np.float32)
            assert int(ids[r][s]) == int(np.argmax(m)), (r, s, int(ids[r][s]), int(np.argmax(m)), state)
            if lps is not None:
                check_lp(("e2e", r, s), lps[r][s], m, ids[r][s])
            state = lm.step(state, int(ids[r][s]))


@pytest.fixture(scope="module")
def golden(golden_dir):
    g, segs, prompts = load_golden(golden_dir, int_prompts=True)
    return g, segs, prompts, int(g["n_new"])


# ------------------------------------------------------------------------------------------ 1. every step, every kind
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["bf16", "int8", "f16", "f32"])
def test_every_step_is_the_fused_argmax(golden, mode):
    _, segs, prompts, n_new = golden
    for name, lm, weight in (("corpus", corpus_lm(), 0.6), ("peaked", peaked(), 40.0)):
        e, dev = make(mode=mode, lm=lm, weight=weight)
        try:
            ids, logits, lps = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True, want_logprobs=True)      # eager: the step logits are wanted
            identity(lm, weight, ids, logits, [n_new, n_new], lps)
            ids_g, _, lps_g = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)                          # the captured loop
            print(f"mode {mode} {name}: {[i.tolist() for i in ids]}")
            for r in range(2):
                assert np.array_equal(ids_g[r], ids[r]) and same_bits(lps_g[r], lps[r]), (name, r)
            if name == "peaked":
                assert all(i.tolist() == PATH for i in ids), "the model's own choice (304 / 10 for ever) gives way to the language model's sequence"
        finally:
            e.close()


# ------------------------------------------------------------------------------------------ 2. the same bits on every path
def test_invariance_all_paths():
    from sonicscribe_amd.dispatch import Dispatcher
    segs, prompts = six()
    budgets = [9, 17, 11, 3, 13, 7]
    lm, weight = forked(), 40.0
    e, dev = make(max_batch=8, lm=lm, weight=weight)
    try:
        ids_e, logits_e, lp_e = e.transcribe_batch(segs, prompts, budgets, want_logits=True, want_logprobs=True)
        identity(lm, weight, ids_e, logits_e, budgets, lp_e)
        states = [lm.walk(i)[0] for i in ids_e]
        print("ids", [i.tolist() for i in ids_e], "final states", states)
        assert len(set(states)) >= 4 and all(len(i) >= 3 for i in ids_e), "the rows end at different states, several tokens into the language model's path"
        ids_g, _, lp_g = e.transcribe_batch(segs, prompts, budgets, want_logprobs=True)
        solo = [e.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]], want_logprobs=True) for i in range(6)]
        slot = e.slot()
        ids_s, _, lp_s = slot.transcribe_batch(segs, prompts, budgets, want_logprobs=True)
        for r in range(6):
            assert np.array_equal(ids_g[r], ids_e[r]) and same_bits(lp_g[r], lp_e[r]), r
            assert np.array_equal(solo[r][0][0], ids_e[r]) and same_bits(solo[r][2][0], lp_e[r]), r
            assert np.array_equal(ids_s[r], ids_e[r]) and same_bits(lp_s[r], lp_e[r]), r
        slot.close()
        # prefill, then splice into a continuous handle: the two words travel with the row, which lands beside rows that are several tokens into other states
        pre = e.slot()
        e.service_begin()
        try:
            pre.stage_pcm(segs[:3]); pre.prefill(prompts[:3], budgets[:3])
            seq1 = e.splice_rows(pre, [0, 1, 2], [0, 1, 2])
            for _ in range(2):
                e.service_step(1, 8)
            pre.stage_pcm(segs[3:]); pre.prefill(prompts[3:], budgets[3:])
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
        for native in (False, True):                              # the Python dispatcher and the native one
            slots = [e.slot(), e.slot()]
            disp = Dispatcher([e], slots=[slots], continuous=True, native=native)
            res = [f.result(timeout=120) for f in [disp.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True) for i in range(6)]]
            disp.close()
            for s in slots:
                s.close()
            for i in range(6):
                assert np.array_equal(res[i][0], ids_e[i]) and same_bits(res[i][1], lp_e[i]), (native, i)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 3. the model: a peaked language model pulls the transcript
def test_a_peaked_lm_at_a_large_weight_pulls_the_transcript_onto_its_sequence():
    """fails without the feature: ASRModel takes no lm=, and the free-running transcript never leaves 304 / 10"""
    from sonicscribe_amd.asr import ASRModel
    lm = peaked()
    pcm = synth.synth_pcm(10, 80000)
    wav = pcm.astype(np.float32) / 32768.0
    plain = ASRModel.from_synthetic(D, SEED, max_batch=4, max_ctx=1024, token_logprobs=True)
    try:
        free = plain.transcribe(wav, max_new_tokens=12, return_debug_info=True)
        assert plain.get_model_info()["lm"] is False
        assert len(free["token_ids"]) == 12 and not set(int(t) for t in free["token_ids"]) & set(PATH) and "lm_logprob" not in free
        with pytest.raises(ValueError, match="lm_score needs a model built with lm="):
            plain.lm_score([1, 2])
    finally:
        plain.close()
    m = ASRModel.from_synthetic(D, SEED, max_batch=4, max_ctx=1024, token_logprobs=True, lm=lm, lm_weight=40.0)
    try:
        assert m.get_model_info()["lm"] is True and m.get_model_info()["lm_weight"] == 40.0
        info = m.transcribe(wav, max_new_tokens=12, return_debug_info=True)
        print("free", [int(t) for t in free["token_ids"]], "under the language model", [int(t) for t in info["token_ids"]])
        assert [int(t) for t in info["token_ids"]] == PATH
        assert info["lm_weight"] == 40.0 and abs(info["lm_logprob"] - len(PATH) * float(np.float32(-0.01))) < 1e-5 and info["lm_logprob"] == m.lm_score(PATH)
        det = m.submit(wav, max_new_tokens=12, detailed=True).result(timeout=120)
        assert np.array_equal(det.token_ids, info["token_ids"]) and same_bits(det.token_logprobs, info["token_logprobs"])
        assert m.transcribe_batch([wav, wav], max_new_tokens=12) == [info["transcript"]] * 2
        short = m.submit(wav, max_new_tokens=3, detailed=True).result(timeout=120)
        assert [int(t) for t in short.token_ids] == PATH[:3]
        st = m.open_stream("s0")                                  # a stream entry point: submit()'s decode, bit for bit
        try:
            raw = pcm.tobytes()
            for o in range(0, len(raw), 2048):
                st.add_audio_chunk(raw[o:o + 2048])
            sd = st.submit_chunks(0, st.next_chunk_id - 1, max_new_tokens=12, detailed=True).result(timeout=120)
            assert np.array_equal(sd.token_ids, det.token_ids) and same_bits(sd.token_logprobs, det.token_logprobs)
        finally:
            st.close()
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 4. off is off; refusals; memory
def test_off_is_off_and_refusals(golden):
    from sonicscribe_amd.engine import SonicError
    g, segs, prompts, n_new = golden
    lm = corpus_lm()
    never, _ = make(max_batch=4)
    e, dev = make(max_batch=4, lm=lm, weight=0.6)
    other = None
    try:
        want = never.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)
        for si in range(2):                                                    # the parent's fixture ids
            assert np.array_equal(want[0][si], g[f"s{si}_new_ids"][:len(want[0][si])])
        under = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)
        a_on = e.memory_info()[0]
        e.set_lm(None)                                                         # lm = 0: the outputs of a handle that never had the option
        off = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)
        for r in range(2):
            assert np.array_equal(off[0][r], want[0][r]) and same_bits(off[2][r], want[2][r]), r
        assert any(not np.array_equal(under[0][r], want[0][r]) or not same_bits(under[2][r], want[2][r]) for r in range(2)), "the model changed nothing"
        # memory: the automaton on the owner, two words per row and max_batch x V floats (and the history) on the handle
        a_never = never.memory_info()[0]
        words = len(lm.pack()) - 5 + 8
        print(f"lm: sonic_memory_info {a_on - a_never} bytes above a handle without it: automaton {4 * words}, vectors {4 * 4 * D.vocab}, words {128 * 4}, history {64 * 1024 * 4}")
        assert a_on - a_never == 4 * words + 4 * 4 * D.vocab + 128 * 4 + 64 * 1024 * 4
        # the destroy is refused by name while a handle refers to the model
        e.set_lm(dev, 0.6)
        with pytest.raises(SonicError, match="is in use: option lm of 1 handle refers to it"):
            dev.close()
        slot = e.slot()                                                        # a slot copies the option: two handles
        with pytest.raises(SonicError, match="option lm of 2 handles refer to it"):
            dev.close()
        again = slot.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)
        for r in range(2):
            assert np.array_equal(again[0][r], under[0][r]) and same_bits(again[2][r], under[2][r]), r
        # the splice refuses handles whose lm or lm_weight differ
        e.service_begin()
        try:
            slot.set_option("lm_weight", int(np.array([0.7], np.float32).view(np.int32)[0]))
            slot.stage_pcm(segs[:1]); slot.prefill(prompts[:1], [4])
            with pytest.raises(SonicError, match="differ in option lm_weight"):
                e.splice_rows(slot, [0], [0])
            slot.decode_step(100)
            slot.set_lm(None)
            slot.stage_pcm(segs[:1]); slot.prefill(prompts[:1], [4])
            with pytest.raises(SonicError, match="differ in option lm:"):
                e.splice_rows(slot, [0], [0])
            slot.decode_step(100)
        finally:
            e.service_end()
        slot.close()
        # beside a grammar, draft_verify and row forks; without token_logprobs; an id that names nothing; a weight that is no weight
        with pytest.raises(SonicError, match="grammar: option lm is on"):
            e.set_option("grammar", 1)
        with pytest.raises(SonicError, match="draft_verify: option lm is on"):
            e.set_option("draft_verify", 1)
        with pytest.raises(SonicError, match="request_forks: option lm is on"):
            e._arm_forks(np.array([2, 1], np.int32))
        with pytest.raises(SonicError, match="token_logprobs cannot be switched off while option lm is on"):
            e.set_option("token_logprobs", 0)
        with pytest.raises(SonicError, match="999 is not a live language model"):
            e.set_option("lm", 999)
        with pytest.raises(SonicError, match="lm_weight: the value carries the bits of an fp32 weight"):
            e.set_option("lm_weight", int(np.array([-1.0], np.float32).view(np.int32)[0]))
        never.set_option("grammar", 1)
        nd = never.lm_create(lm)
        with pytest.raises(SonicError, match="lm: option grammar is on"):
            never.set_lm(nd, 0.5)
        nolp, _ = make(max_batch=2, lp=False)
        try:
            with pytest.raises(SonicError, match="lm: option token_logprobs must be on first"):
                nolp.set_lm(nolp.lm_create(lm), 0.5)
        finally:
            nolp.close()
        # the bulk pipeline refuses such a handle
        from sonicscribe_amd.pipeline import NativePipeline
        pre = e.slot()
        try:
            with pytest.raises(RuntimeError, match="sonic_pipeline_create: option lm is on"):
                NativePipeline([e], [pre], block=4)
        finally:
            pre.close()
        # a scoring handle ignores the option: the forced run's log-probabilities are the raw model's
        sc, ref = e.slot(), never.slot()
        for h in (sc, ref):
            h.set_option("forced_parallel", 1)
        forced = [want[0][0][:4], want[0][1][:4]]
        a = sc.score_batch(segs, prompts, forced)
        b = ref.score_batch(segs, prompts, forced)
        for r in range(2):
            assert same_bits(np.asarray(a[r], np.float32), np.asarray(b[r], np.float32)), r
        sc.close(); ref.close()
        # the library validates at the load, by message
        bad = lm.pack().copy(); bad[3] = 9
        import ctypes as C
        rc = e.lib.sonic_load_tensor(e.h, b"lm:77", bad.ctypes.data_as(C.c_void_p), 2, (C.c_int64 * 1)(len(bad)), 1)
        assert rc == 1 and b"lm: order 9 is outside 1 .. 8" in e.lib.sonic_last_error(None)
        e.set_lm(None)
        dev.close()                                                            # no handle refers to it any more
    finally:
        e.close(); never.close()


# ------------------------------------------------------------------------------------------ 5. live HF
def test_live_hf_generate_with_a_logits_processor_vs_fp32_engine_through_checkpoint(tmp_path):
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    from tests import hf_helpers as G
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.engine import MODE_F32
    n_new = 10
    lm, weight = peaked(), 40.0
    model, _ = G.build_tiny(torch.float32)
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    pcm = synth.synth_pcm(10, 80000)
    feats, mask = G.mel_case(G.feature_extractor(), pcm)
    ids = G.PROMPT_PREFIX + [D.audio_token_id] * spec.audio_token_count(int(mask.sum())) + G.PROMPT_SUFFIX
    input_ids = torch.tensor([ids], dtype=torch.long)

    class Fusion(transformers.LogitsProcessor):
        """scores + NGramLM.scores at the state behind the ids generated so far"""
        def __call__(self, seq, scores):
            state = lm.walk([int(t) for t in seq[0, len(ids):]])[0]
            return scores + torch.from_numpy(lm.scores(state, weight))[None]

    kw = dict(input_ids=input_ids, input_features=torch.from_numpy(feats)[None], input_features_mask=torch.from_numpy(mask)[None].long(),
              attention_mask=torch.ones_like(input_ids), max_new_tokens=n_new, do_sample=False, return_dict_in_generate=True, output_scores=True)
    with torch.no_grad():
        base = model.generate(**kw).sequences[0, len(ids):].tolist()
        gen = model.generate(**kw, logits_processor=transformers.LogitsProcessorList([Fusion()]))
    ref_ids = gen.sequences[0, len(ids):].numpy().astype(np.int32)
    scores = torch.stack([s[0] for s in gen.scores]).numpy()
    margins = [float(np.sort(s)[-1] - np.sort(s)[-2]) for s in scores[:len(ref_ids)]]
    print(f"live HF under the language model: {ref_ids.tolist()} (without {base[:3]} ...), top-1 / top-2 margins {[round(x, 2) for x in margins]}")
    assert ref_ids.tolist()[:len(PATH)] == PATH and base[:len(PATH)] != PATH and min(margins[:len(PATH)]) > 1.0, "no step may be excused"
    m = ASRModel(str(tmp_path), max_batch=2, max_ctx=1024, slots=1, continuous=False, _allow_synthetic_prompt=True, _engine_mode=MODE_F32, token_logprobs=True, lm=lm, lm_weight=weight)
    try:
        got, _ = m.model.transcribe_batch([pcm], [ids], [n_new])
        assert np.array_equal(got[0], ref_ids[:len(got[0])]) and got[0].tolist() == PATH, (got[0].tolist(), ref_ids.tolist())
    finally:
        m.close()
