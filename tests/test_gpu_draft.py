"""Draft-verified decoding on the GPU (option draft_verify, sonic_load_tensor "request_draft"; csrc/rows.hip): a request brings a draft of its
transcript, the prefill runs over prompt || draft, every draft position is decided from the lm_head GEMM's row by rows_kernel under the handle's processors,
the longest agreeing prefix is accepted and the unchanged head and greedy loop carry on from the first disagreement.

Fixture margins (tests/golden/tiny_bf16.npz, checked in test_fixture_margins on the host side of this file): s1's greedy margins are 0.172 at step 0 and >= 0.859
afterwards, s0's >= 0.219 over its first ten steps - above twice the 0.0625 logit tolerance the project holds the prefill and the step path to, so a draft of the
fixture's own ids must be accepted in full whichever of the two paths decides a position."""
import numpy as np
import pytest

from gpu_common import SEED, bits, flags, load_golden, make_engine
from sonicscribe_amd import spec
from sonicscribe_amd.genconfig import GenerationGuards

pytestmark = pytest.mark.gpu
TOL = 0.0625
ALL3 = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[304, 10])      # tests/test_gpu_generation_guards.py: they bind on the fixture's rows


def make(mode=0, max_batch=4, max_ctx=1024, lp=True, guards=None, draft=True, top=0, opts=()):
    first = flags((lp, "token_logprobs", 1), (top, "top_logprobs", top), (guards, "generation", guards))
    return make_engine(spec.TINY, mode, max_batch, max_ctx, first + list(opts) + flags((draft, "draft_verify", 1)))


def _same(a, b):
    if isinstance(a, tuple):                                              # TokenScores: lp, top_logprobs, top_ids
        return all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return np.array_equal(a, b)


@pytest.fixture(scope="module")
def golden(golden_dir):
    g, segs, prompts = load_golden(golden_dir, int_prompts=True)
    return g, segs, prompts, int(g["n_new"])


@pytest.fixture(scope="module")
def eng():
    e = make()
    yield e
    e.close()


def test_fixture_margins(golden):
    g = golden[0]
    assert g["s1_margins"][0] > 2 * TOL and g["s1_margins"][1:].min() > 2 * TOL and g["s0_margins"][:10].min() > 2 * TOL


# ------------------------------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("k", [1, 12, 23])
def test_fixture_prefix_is_accepted(eng, golden, k):
    g, segs, prompts, n_new = golden
    ref = g["s1_new_ids"]
    ids, logits, lp = eng.transcribe_batch([segs[1]], [prompts[1]], [n_new], want_logits=True, want_logprobs=True, request_draft=[ref[:k]])
    assert int(eng.draft_accepted(1)[0]) == k
    assert np.array_equal(ids[0], ref)
    err = np.abs(logits[:n_new, 0] - g["s1_step_logits"]).max(axis=1)
    print(f"s1 draft {k}: max |dlogit| per step: verify rows {err[:k].max():.4f}, head and loop {err[k:].max():.4f}")
    assert err.max() <= TOL
    assert lp[0].shape == (n_new,) and np.all(np.isfinite(lp[0])) and np.all(lp[0] <= 0)


def test_fixture_wrong_id_stops_the_draft(eng, golden):
    g, segs, prompts, n_new = golden
    ref = g["s1_new_ids"]
    d = ref[:12].copy(); d[7] = 845
    ids, _ = eng.transcribe_batch([segs[1]], [prompts[1]], [n_new], request_draft=[d])
    assert int(eng.draft_accepted(1)[0]) == 7 and np.array_equal(ids[0], ref)


def test_fixture_short_budget(eng, golden):
    g, segs, prompts, _ = golden
    ref = g["s0_new_ids"]
    ids, _ = eng.transcribe_batch([segs[0]], [prompts[0]], [10], request_draft=[ref[:5]])
    assert int(eng.draft_accepted(1)[0]) == 5 and np.array_equal(ids[0], ref[:10])


# ------------------------------------------------------------------------------------------ 2. acceptance against the scoring handle, exact
def test_acceptance_against_the_scoring_route(golden):
    g, segs, prompts, n_new = golden
    G = GenerationGuards(**ALL3)
    e = make(guards=ALL3)
    sc = make(draft=False, opts=(("forced_parallel", 1),))
    try:
        plain, _ = e.transcribe_batch(segs, prompts, [n_new, n_new])
        rng = np.random.default_rng(3)
        for trial, k in enumerate((0, 3, 9)):
            drafts = []
            for r in range(2):
                tail = [int(t) for t in rng.integers(0, 900, 8)]                  # arbitrary ids: no EOS (990 ..), no placeholder (1000)
                drafts.append([int(t) for t in plain[r][:k]] + tail)
            ids, dump, lp = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True, want_logprobs=True, request_draft=drafts)
            acc = e.draft_accepted(2)
            # the independent route: the same prefill sequence and the same GEMM on a scoring handle; one more id so that every draft position has a row
            _, lg, _ = sc.score_batch(segs, prompts, np.asarray([d + [1] for d in drafts], np.int32), want_logits=True)
            for r in range(2):
                D = len(drafts[r])
                want = D
                for n in range(D):
                    t = int(np.argmax(G.apply(lg[n, r], prompts[r] + drafts[r][:n])))
                    if t != drafts[r][n]:
                        want = n
                        break
                assert int(acc[r]) == want, (trial, r, int(acc[r]), want)
                print(f"  dumped verify rows equal the scoring run's rows bit for bit: {np.array_equal(dump[:want, r].view(np.uint32), lg[:want, r].view(np.uint32))}")
                for s in range(len(ids[r])):
                    assert int(np.argmax(G.apply(dump[s, r], prompts[r] + [int(t) for t in ids[r][:s]]))) == int(ids[r][s]), (trial, r, s)
                assert [int(t) for t in ids[r][:want]] == drafts[r][:want]
                same = int(np.sum(np.asarray(ids[r][:min(len(ids[r]), len(plain[r]))]) == np.asarray(plain[r][:min(len(ids[r]), len(plain[r]))])))
                print(f"trial {trial} request {r}: accepted {want} of {D}; {same} of {len(plain[r])} ids equal the plain run's")
            assert k == 0 or acc.max() >= 1
    finally:
        e.close(); sc.close()


# ------------------------------------------------------------------------------------------ 3. nothing behind the first rejected token matters
def test_rejected_tail_does_not_matter(golden):
    g, segs, prompts, n_new = golden
    e = make(guards=dict(suppress_tokens=[5, 6]))
    try:
        base, _ = e.transcribe_batch([segs[1]], [prompts[1]], [n_new])
        gd = [int(t) for t in base[0][:12]]
        X, Y = [77, 78, 79, 80, 81], [500, 3, 3, 640, 2]
        a_ids, _, a_lp = e.transcribe_batch([segs[1]], [prompts[1]], [n_new], want_logprobs=True, request_draft=[gd + [5] + X])
        a_acc = int(e.draft_accepted(1)[0])
        b_ids, _, b_lp = e.transcribe_batch([segs[1]], [prompts[1]], [n_new], want_logprobs=True, request_draft=[gd + [6] + Y])
        b_acc = int(e.draft_accepted(1)[0])
        assert a_acc == b_acc == 12
        assert np.array_equal(a_ids[0], b_ids[0]) and _same(a_lp[0], b_lp[0])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 4. an undrafted request keeps its bits
def test_undrafted_request_keeps_its_bits(eng, golden):
    g, segs, prompts, n_new = golden
    plain = make(draft=False)
    try:
        want_ids, _, want_lp = plain.transcribe_batch([segs[0]], [prompts[0]], [n_new], want_logprobs=True)
        mem0 = eng.memory_info()[0]
        ids, _, lp = eng.transcribe_batch([segs[0]], [prompts[0]], [n_new], want_logprobs=True)                  # option on, nothing staged
        assert np.array_equal(ids[0], want_ids[0]) and _same(lp[0], want_lp[0])
        assert np.array_equal(eng.draft_accepted(1), [0])
        alone_ids, _, alone_lp = eng.transcribe_batch([segs[0]], [prompts[0]], [n_new], want_logprobs=True, request_draft=[None])   # an empty draft: the same launches
        assert np.array_equal(alone_ids[0], want_ids[0]) and _same(alone_lp[0], want_lp[0])
        ids2, _, lp2 = eng.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True, request_draft=[None, g["s1_new_ids"][:12]])   # beside a drafted request
        assert np.array_equal(eng.draft_accepted(2), [0, 12])
        assert np.array_equal(ids2[0], want_ids[0]) and _same(lp2[0], want_lp[0])
        assert np.array_equal(ids2[1], g["s1_new_ids"])
        assert eng.memory_info()[0] >= mem0                                                                        # (the buffers came with the first drafted prefill)
    finally:
        plain.close()


def test_buffers_come_with_the_first_drafted_prefill(golden):
    g, segs, prompts, n_new = golden
    e = make()
    try:
        m0 = e.memory_info()[0]
        e.transcribe_batch([segs[1]], [prompts[1]], [n_new])
        assert e.memory_info()[0] == m0
        e.transcribe_batch([segs[1]], [prompts[1]], [n_new], request_draft=[g["s1_new_ids"][:4]])
        m1 = e.memory_info()[0]
        tc, V = e.tok_cap, spec.TINY.vocab
        want = 256 * V * 2 + (5 * tc + 256) * 4 + tc * 4 + tc * 4 + 64 * 4      # chunk logits, plan, choices, records (K = 0), accepted counts
        print(f"draft_verify buffers: {m1 - m0} bytes (expected {want})")
        assert m1 - m0 == want
        e.transcribe_batch([segs[1]], [prompts[1]], [n_new], request_draft=[g["s1_new_ids"][:9]])
        assert e.memory_info()[0] == m1
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 5. every scheduler of the engine: whole batch, eager, spliced into a continuous loop
def _requests(golden):
    g, segs, prompts, n_new = golden
    ref = g["s1_new_ids"]
    wrong = ref[:6].copy(); wrong[3] = 845
    #        segment  budget  draft
    return [(1, n_new, ref[:12]),          # a + 1 > 1: several records out of the prefill
            (1, 8, ref[:7]),               # max_new = D + 1: ends at the prefill
            (0, 10, None),                 # no draft
            (1, n_new, wrong)]             # stops at 3


@pytest.mark.parametrize("top", [0, 3])
def test_every_engine_path(golden, top):
    g, segs, prompts, n_new = golden
    reqs = _requests(golden)
    S = [segs[i] for i, _, _ in reqs]; P = [prompts[i] for i, _, _ in reqs]; B = [b for _, b, _ in reqs]; Dr = [d for _, _, d in reqs]
    e = make(top=top)
    try:
        ids_e, _, lp_e = e.transcribe_batch(S, P, B, want_logits=True, want_logprobs=True, request_draft=Dr)            # eager loop
        acc = e.draft_accepted(4)
        assert list(acc) == [12, 7, 0, 3]
        assert np.array_equal(ids_e[0], g["s1_new_ids"]) and np.array_equal(ids_e[1], g["s1_new_ids"][:8]) and np.array_equal(ids_e[2], g["s0_new_ids"][:10])
        assert np.array_equal(ids_e[3], g["s1_new_ids"])
        if top:
            for r in range(4):
                assert np.array_equal(lp_e[r].top_ids[:acc[r], 0], ids_e[r][:acc[r]])                                # alternative 0 of an accepted record is the token
                assert _same(lp_e[r].top_logprobs[:acc[r], 0], lp_e[r].lp[:acc[r]])
        ids_g, _, lp_g = e.transcribe_batch(S, P, B, want_logprobs=True, request_draft=Dr)                               # hipGraph loop
        for r in range(4):
            assert np.array_equal(ids_g[r], ids_e[r]) and _same(lp_g[r], lp_e[r]), r
        for r in range(4):                                                                                           # alone
            i1, _, l1 = e.transcribe_batch([S[r]], [P[r]], [B[r]], want_logprobs=True, request_draft=[Dr[r]])
            assert np.array_equal(i1[0], ids_e[r]) and _same(l1[0], lp_e[r]), r
        # a prefill slot and a continuous loop: the splice carries every accepted token's id and record
        pre = e.slot()
        e.service_begin()
        try:
            pre.stage_pcm(S); pre.prefill(P, B, request_draft=Dr)
            seq = e.splice_rows(pre, [0, 1, 2, 3], [3, 0, 1, 2])
            rows, got = {3: 0, 0: 1, 1: 2, 2: 3}, {}
            for _ in range(200):
                fin, nn, s_, _ = e.service_step(1, 4)
                done = [r for r in rows if r not in got and s_ > seq and fin[r]]
                if done:
                    a, b = e.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                    for r, x, y in zip(done, a, b):
                        got[r] = (x, y)
                if len(got) == 4:
                    break
            assert len(got) == 4
            for row, req in rows.items():
                assert np.array_equal(got[row][0], ids_e[req]) and _same(got[row][1], lp_e[req]), (row, req)
        finally:
            e.service_end()
            pre.close()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 6. refusals, by message
def test_refusals(golden):
    from sonicscribe_amd.engine import Engine, SonicError
    g, segs, prompts, n_new = golden
    d = spec.TINY
    ref = [int(t) for t in g["s1_new_ids"]]
    one = dict(segments=[segs[1]], prompts=[prompts[1]], max_new=[n_new])
    off = make(draft=False)
    try:
        with pytest.raises(SonicError, match="option draft_verify is off"):
            off.set_request_draft([ref[:3]])
        with pytest.raises(SonicError, match="draft_verify"):
            off.draft_accepted(1)
    finally:
        off.close()
    for mode, word in ((1, "int8"), (3, "fp32")):
        e = Engine(d, 0, mode, max_batch=2, max_ctx=512)
        try:
            with pytest.raises(SonicError, match=f"draft_verify.*{word}"):
                e.set_option("draft_verify", 1)
        finally:
            e.close()
    sc = make(draft=False, opts=(("forced_parallel", 1),))
    try:
        with pytest.raises(SonicError, match="draft_verify.*forced_parallel"):
            sc.set_option("draft_verify", 1)
    finally:
        sc.close()
    e = make(max_batch=2, opts=(("request_bias", 1), ("sampling", 1), ("grammar", 1)))
    try:
        with pytest.raises(SonicError, match="forced_parallel.*draft_verify"):
            e.set_option("forced_parallel", 1)
        for bad, what in (([d.vocab], "out of vocabulary"), ([-1], "out of vocabulary"), ([d.audio_token_id], "audio placeholder"), ([d.eos_ids[1]], "EOS id")):
            with pytest.raises(SonicError, match=what):
                e.set_request_draft([ref[:2] + bad])
        with pytest.raises(SonicError, match=r"holds 24 ids, its budget of 24 tokens leaves room for 23"):
            e.transcribe_batch(**one, request_draft=[ref])
        ids, _ = e.transcribe_batch(**one)                                                                           # ... and the refusal consumed the draft
        assert np.array_equal(e.draft_accepted(1), [0]) and np.array_equal(ids[0], ref)
        with pytest.raises(SonicError, match="drafts for 2 requests, the batch has 1"):
            e.transcribe_batch(**one, request_draft=[ref[:3], None])
        many = [7] * 900                                                                                             # more tokens than one prefill of this handle holds
        assert 2 * (260 + 900) > e.tok_cap
        with pytest.raises(SonicError, match=rf"asks for {2 * (260 + 900)} tokens \(prompts and drafts\), {e.tok_cap} fit"):
            e.transcribe_batch([segs[1]] * 2, [prompts[1]] * 2, [1000, 1000], request_draft=[many, many])
        e.set_forced_ids(np.asarray([ref], np.int32))
        try:
            with pytest.raises(SonicError, match="forced ids are set"):
                e.transcribe_batch(**one, request_draft=[ref[:3]])
        finally:
            e.set_forced_ids(None)
        from sonicscribe_amd.reqbias import RequestBias
        with pytest.raises(SonicError, match="a draft and a request bias table"):
            e.transcribe_batch(**one, request_draft=[ref[:3]], request_bias=[RequestBias({(7,): 1.0})])
        with pytest.raises(SonicError, match="a draft and a temperature"):
            e.transcribe_batch(**one, request_draft=[ref[:3]], request_sampling=[(0.8, 1)])
        from sonicscribe_amd.grammar import Grammar
        gr = e.grammar_create(Grammar.from_token_sequences([[10, 10]], d.eos_ids, vocab=d.vocab, audio_token_id=d.audio_token_id))
        try:
            with pytest.raises(SonicError, match="a draft and a grammar"):
                e.transcribe_batch(**one, request_draft=[ref[:3]], request_grammar=[gr])
            # an undrafted request of the same batch may carry them
            two = dict(segments=[segs[1], segs[0]], prompts=[prompts[1], prompts[0]], max_new=[n_new, 6])
            ids, _ = e.transcribe_batch(**two, request_draft=[ref[:3], None], request_bias=[None, RequestBias({(7,): 1.0})], request_sampling=[None, (0.8, 1)],
                                        request_grammar=[None, gr])
            assert np.array_equal(e.draft_accepted(2), [3, 0]) and np.array_equal(ids[0], ref)
        finally:
            gr.close()
        # while the handle has work in hand
        e.stage_pcm([segs[1]]); e.prefill([prompts[1]], [n_new])
        with pytest.raises(SonicError, match="draft_verify.*still running"):
            e.set_option("draft_verify", 0)
        while e.decode_step(8)[0]:
            pass
        e.fetch_tokens(1, n_new)
        # the splice refuses handles that differ in the option
        pre = e.slot()
        pre.set_option("draft_verify", 0)
        e.service_begin()
        try:
            pre.stage_pcm([segs[1]]); pre.prefill([prompts[1]], [n_new])
            with pytest.raises(SonicError, match="differ in option draft_verify"):
                e.splice_rows(pre, [0], [0])
        finally:
            e.service_end(); pre.close()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 5b. ... and every scheduler above the engine
def test_every_dispatcher(golden):
    from sonicscribe_amd.dispatch import Dispatcher
    g, segs, prompts, n_new = golden
    reqs = _requests(golden)
    S = [segs[i] for i, _, _ in reqs]; P = [prompts[i] for i, _, _ in reqs]; B = [b for _, b, _ in reqs]; Dr = [d for _, _, d in reqs]
    e = make(top=3)
    try:
        ids_e, _, lp_e = e.transcribe_batch(S, P, B, want_logprobs=True, request_draft=Dr)
        assert list(e.draft_accepted(4)) == [12, 7, 0, 3]
        for name, kw in (("python continuous", dict(continuous=True, native=False)), ("native continuous", dict(continuous=True, native=True)), ("batch", dict(continuous=False))):
            slots = [e.slot(), e.slot()]
            disp = Dispatcher([e], slots=[slots], **kw)
            res = [f.result(timeout=120) for f in [disp.submit([S[i]], P[i], B[i], want_logprobs=True, draft=Dr[i]) for i in range(4)]]
            disp.close()
            for s in slots:
                s.close()
            for i in range(4):
                assert np.array_equal(res[i][0], ids_e[i]) and _same(res[i][1], lp_e[i]), (name, i)
    finally:
        e.close()


def test_asrmodel_submit_and_streams(golden):
    from sonicscribe_amd import asr, frontend
    g, segs, prompts, n_new = golden
    m = asr.ASRModel.from_synthetic(spec.TINY, SEED, max_batch=4, max_ctx=1024, token_logprobs=True, top_logprobs=3, draft_verify=True)
    try:
        assert m.get_model_info()["draft_verify"] is True
        wav = segs[1].astype(np.float32) / 32768.0
        base = m.submit(wav, max_new_tokens=n_new, detailed=True).result(timeout=120)
        assert (base.draft_len, base.draft_matched) == (0, 0)
        dr = [int(t) for t in base.token_ids[:12]]
        det = m.submit(wav, max_new_tokens=n_new, detailed=True, draft=dr + [spec.TINY.eos_ids[0], 5]).result(timeout=120)      # cut in front of the EOS id
        # the same drafted request as a whole batch on a handle of the model's weights
        ref = m.model.slot()
        try:
            _, wins, n_audio = m._prepare(wav, 16000)
            prompt = m.prompt.build(frontend.build_instruction(None), n_audio)
            ids_r, _, lp_r = ref.transcribe_batch(wins, [prompt], [n_new], req_win=[0, len(wins)], want_logprobs=True, request_draft=[dr])
            acc = int(ref.draft_accepted(1)[0])
        finally:
            ref.close()
        assert np.array_equal(det.token_ids, ids_r[0]) and _same(det.token_logprobs, lp_r[0].lp) and _same(det.top_logprobs, lp_r[0].top_logprobs)
        assert det.draft_len == 12 and det.draft_matched == asr.draft_matched(det.token_ids, dr) >= acc
        print(f"ASRModel.submit: draft of 12, accepted {acc}, matched {det.draft_matched}; {int(np.sum(det.token_ids[:len(base.token_ids)] == base.token_ids[:len(det.token_ids)]))} of {len(base.token_ids)} ids equal the undrafted run's")
        info = m.transcribe(wav, max_new_tokens=n_new, return_debug_info=True, draft=dr)
        assert info["draft_len"] == 12 and info["draft_matched"] == det.draft_matched and np.array_equal(info["token_ids"], det.token_ids)
        texts = m.transcribe_batch([wav, wav], max_new_tokens=n_new, drafts=[dr, None])
        assert texts[0] == det.text and texts[1] == base.text
        st = m.open_stream("s")
        try:
            raw = segs[1].tobytes()
            for o in range(0, len(raw), 2048):
                st.add_audio_chunk(raw[o:o + 2048])
            a = st.submit_samples(0, len(segs[1]), n_new, detailed=True).result(timeout=120)
            b = st.submit_samples(0, len(segs[1]), n_new, detailed=True, draft=[int(t) for t in a.token_ids[:10]]).result(timeout=120)
            assert b.draft_len == 10 and b.draft_matched == asr.draft_matched(b.token_ids, a.token_ids[:10])
        finally:
            st.close()
    finally:
        m.close()
    off = asr.ASRModel.from_synthetic(spec.TINY, SEED, max_batch=4, max_ctx=1024)
    try:
        with pytest.raises(ValueError, match="draft= needs a model built with draft_verify=True"):
            off.transcribe(np.zeros(16000, np.float32), draft=[5])
    finally:
        off.close()


def test_dispatcher_and_pipeline_refusals(golden):
    import ctypes as C
    from sonicscribe_amd.dispatch import Dispatcher
    from sonicscribe_amd.engine import DispatchRequest
    g, segs, prompts, n_new = golden
    ref = [int(t) for t in g["s1_new_ids"]]
    off = make(draft=False)
    try:
        slots = [off.slot(), off.slot()]
        disp = Dispatcher([off], slots=[slots], continuous=True, native=True)
        with pytest.raises(ValueError, match="draft_verify"):
            disp.submit([segs[1]], prompts[1], n_new, draft=ref[:3])
        rep = disp.replicas[0]                                                 # ... and the library's own answer, not only the Python check in front of it
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        pcm = np.ascontiguousarray(segs[1], np.int16); offs = np.array([0, len(pcm)], np.int64); pr = np.ascontiguousarray(prompts[1], np.int32)
        w = np.asarray([10, 10], np.int32); tk = C.c_int64(0)
        rec = DispatchRequest(host_pcm=vp(pcm), host_off=vp(offs), W=1, prompt_ids=vp(pr), prompt_len=len(pr), max_new=n_new, draft_ids=vp(w), n_draft=2)
        assert rep.lib.sonic_dispatch_submit(rep.h, C.byref(rec), C.byref(tk)) == 1
        assert b"option draft_verify is off" in rep.lib.sonic_last_error(None)
        disp.close()
    finally:
        off.close()
    e = make(max_batch=32)                                                      # (a pipeline block holds 32 rows)
    try:
        slots = [e.slot(), e.slot()]
        disp = Dispatcher([e], slots=[slots], continuous=True, native=True)
        with pytest.raises(ValueError, match="holds 5 ids, the request's budget of 4 tokens leaves room for 3"):
            disp.submit([segs[1]], prompts[1], 4, draft=ref[:5])
        with pytest.raises(ValueError, match="EOS id"):
            disp.submit([segs[1]], prompts[1], n_new, draft=[10, spec.TINY.eos_ids[0]])
        ok = disp.submit([segs[1]], prompts[1], n_new, draft=ref[:5]).result(timeout=120)      # the refusals left nothing armed
        assert np.array_equal(ok, ref)
        disp.close()
        with pytest.raises(Exception, match="option draft_verify is on on a handle"):
            Dispatcher([e], slots=[slots], bulk=True, decoders=1)
    finally:
        e.close()


def test_refused_records_leave_nothing_behind(golden):
    """every value's option on: three records refused from one thread - each with its own message - leave nothing for the plain request that thread submits next"""
    import ctypes as C
    from sonicscribe_amd.dispatch import Dispatcher
    from sonicscribe_amd.engine import DispatchRequest
    g, segs, prompts, n_new = golden
    ref = [int(t) for t in g["s1_new_ids"]]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    e = make(opts=(("sampling", 1), ("truncation", 1), ("grammar", 1)))
    try:
        slots = [e.slot(), e.slot()]
        disp = Dispatcher([e], slots=[slots], continuous=True, native=True)
        rep = disp.replicas[0]
        pcm = np.ascontiguousarray(segs[1], np.int16); offs = np.array([0, len(pcm)], np.int64); pr = np.ascontiguousarray(prompts[1], np.int32)
        w = np.asarray(ref[:5], np.int32); tk = C.c_int64(0)
        record = lambda max_new=n_new, **kw: DispatchRequest(host_pcm=vp(pcm), host_off=vp(offs), W=1, prompt_ids=vp(pr), prompt_len=len(pr), max_new=max_new, **kw)
        for rec, msg in ((record(grammar_id=999), b"grammar: 999 is not a live grammar"),
                         (record(cut=1, top_k=5, top_p=0.9), b"truncation: the request is not sampled"),
                         (record(4, draft_ids=vp(w), n_draft=5), b"draft: the draft holds 5 ids, the request's budget of 4 tokens leaves room for 3")):
            assert rep.lib.sonic_dispatch_submit(rep.h, C.byref(rec), C.byref(tk)) == 1 and msg in rep.lib.sonic_last_error(None), (msg, rep.lib.sonic_last_error(None))
        plain = disp.submit([segs[1]], prompts[1], n_new).result(timeout=120)
        assert np.array_equal(plain, ref)                                      # the fixture's solo ids: no grammar, no cut, no draft came along
        assert rep.free_rows == rep.n_rows and rep.load() == 0
        disp.close()
    finally:
        e.close()
