"""Word timestamps on the parallel forced run (option forced_align, Engine.score_batch(align=True), ASRModel(timestamps=True)): the decoder's attention
onto the audio placeholder run at the selected heads (align_probs_kernel behind the layer's RoPE), normalised over tokens, median-filtered and averaged over heads
(align_reduce_kernel), then DTW (align_dtw_kernel) - t_n per scored token, as one more float behind every log-probability record.  TINY, synthetic weights, the
tiny fixtures' audio.

References and tolerances:
  * align_probs against the float64 softmax of the handle's own roped queries (debug buffer dq) and keys (dqkv's k columns through tests/glue_ref.py's RoPE, which
    restates the append kernel bit for bit - checked here on the query columns, whose roped form dq holds): the bound tests/align_ref.py derives (rho p + 2^-126)
  * align_matrix against the float64 restatement from align_probs: the same derivation from p on (no softmax error: rho = 0), thin columns left out
  * t_n against the restated fp32 DTW of align_matrix: exactly
  * everything about batching, chunking, fan-out and slots: bit equality
  * live transformers (eager attention, output_attentions): the rule of tests/test_gpu_fp32_distance.py with its factor 1.25
"""
import os
from functools import partial

import numpy as np
import pytest

import align_ref as R
import glue_ref as G
import gpu_common
from gpu_common import bits, flags, forced_ids, load_golden, make_engine
from sonicscribe_amd import frontend, spec, synth

pytestmark = pytest.mark.gpu
D = spec.TINY
N = 24
F = np.float32
PRE, SUF = [1, 17, 23, 5], [7, 301, 302, 303, 9, 11]
FACTOR = 1.25      # tests/test_gpu_fp32_distance.py's: no further from the fp32 truth than 1.25 x the reference's own bf16 path
prompt_for = partial(gpu_common.prompt_for, D, prefix=PRE, suffix=SUF)


def make(mode=0, max_batch=4, heads=(), align=True, K=0, lp=True):
    opts = flags((lp, "token_logprobs", 1), (K, "top_logprobs", K), (True, "forced_parallel", 1), (align, "forced_align", 1))
    return make_engine(D, mode, max_batch, 1024, opts + [("align_head", l * 256 + h) for l, h in heads])


@pytest.fixture(scope="module")
def golden(golden_dir):
    g, segs, prompts = load_golden(golden_dir, "tiny_forced_bf16.npz")
    return segs, prompts, forced_ids(g)


@pytest.fixture(scope="module")
def eng():
    e = make()
    yield e
    e.close()


def read_align(e, L, A):
    """(align_probs [heads][S][A_max], align_matrix [S][A_max]) of the last run: L the sequences' row counts, A their audio runs"""
    S, Am = int(sum(L)), int(max(A))
    M = e.debug_read("align_matrix", S * Am).reshape(S, Am)
    return M, S, Am


@pytest.fixture(scope="module")
def base(eng, golden):
    """the two fixture sequences aligned once with the default heads: (ids, scores, M, row offsets).  Shared, never changed"""
    segs, prompts, force = golden
    ids, _, sc = eng.score_batch(segs, prompts, force, align=True)
    A = [int((np.asarray(p) == D.audio_token_id).sum()) for p in prompts]
    M, S, Am = read_align(eng, [N, N], A)
    return ids, sc, M, A


# ------------------------------------------------------------------------------------------ 1. the last layer's heads against the handle's own q and k
def test_last_layer_probs_matrix_and_times(golden):
    segs, prompts, force = golden
    Hq, Hkv, last = D.dec_heads, D.dec_kv_heads, D.dec_layers - 1
    e = make(heads=[(last, h) for h in range(Hq)])
    try:
        ids, _, sc = e.score_batch(segs, prompts, force, align=True)
        P_len = [len(p) for p in prompts]
        A = [int((np.asarray(p) == D.audio_token_id).sum()) for p in prompts]
        a0 = [int(np.argmax(np.asarray(p) == D.audio_token_id)) for p in prompts]
        n_tok = sum(P + N - 1 for P in P_len)
        S, Am = 2 * N, max(A)
        dq = e.debug_read("dq", n_tok * Hq * 128).reshape(n_tok, Hq, 128)
        dqkv = e.debug_read("dqkv", n_tok * (Hq + 2 * Hkv) * 128).reshape(n_tok, Hq + 2 * Hkv, 128)
        P = e.debug_read("align_probs", Hq * S * Am).reshape(Hq, S, Am)
        M = e.debug_read("align_matrix", S * Am).reshape(S, Am)
        cs = engine_rope_table(1024)
        off = 0
        for r in range(2):
            rows = off + P_len[r] - 1 + np.arange(N)                       # the rows whose attention produced target n
            pos = P_len[r] - 1 + np.arange(N)
            q = dq[rows]
            # the restated RoPE is the append kernel's: the query columns of dqkv through it give dq bit for bit
            krows = off + a0[r] + np.arange(A[r])
            for rr, pp in ((rows, pos), (krows, a0[r] + np.arange(A[r]))):   # ... at the scored rows and at the audio positions the keys sit at
                assert np.array_equal(bits(G.rope(dqkv[rr, :Hq], cs[pp][:, None, :], 128, "bf16")), bits(dq[rr])), r
            k = G.rope(dqkv[krows, Hq:Hq + Hkv], cs[a0[r] + np.arange(A[r])][:, None, :], 128, "bf16")
            ref = R.matrix_bound(q, k)
            got = P[:, r * N:(r + 1) * N, :A[r]].astype(np.float64)
            ratio = float((np.abs(got - ref["p"]) / ref["p_bound"]).max())
            print(f"align s{r}: worst |align_probs - p64(own q, k)| / bound = {ratio:.3f}; rows sum to 1 within {np.abs(got.sum(-1) - 1).max():.2e}")
            assert ratio <= 1.0
            # the matrix from the probabilities the kernel itself wrote: the normalisation's part of the bound alone
            Mr = M[r * N:(r + 1) * N, :A[r]]
            mb = matrix_from_probs_bound(got)
            live = mb["ok"]
            ratio_m = float((np.abs(Mr.astype(np.float64) - mb["M"])[live] / mb["bound"][live]).max())
            print(f"align s{r}: worst |align_matrix - M64(align_probs)| / bound = {ratio_m:.3f} over {live.mean():.3f} of the entries")
            assert ratio_m <= 1.0 and live.mean() >= 1 - 7 * R.THIN_CAP
            t = R.times_of(Mr)
            assert np.array_equal(sc[r].times, t) and np.all(np.diff(t) >= 0) and 0 <= t.min() and t.max() < A[r]
            off += P_len[r] + N - 1
    finally:
        e.close()


def engine_rope_table(ctx, theta=10000.0, hd=128):
    """the decoder's cos | sin table as the engine builds it (engine.cpp: fp32 powf / cosf / sinf of the C library, rounded to the activation type) - through the
    same C library, because numpy's own float32 cos differs from it in the last bit often enough to flip a bf16 rounding (30 of 65536 entries)"""
    import ctypes
    import ctypes.util
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for fn, n in ((m.powf, 2), (m.cosf, 1), (m.sinf, 1)):
        fn.restype = ctypes.c_float; fn.argtypes = [ctypes.c_float] * n
    half = hd // 2
    t = np.zeros((ctx, hd), F)
    for i in range(half):
        inv = F(1.0) / F(m.powf(theta, float(F(2 * i) / F(hd))))
        for p_ in range(ctx):
            ang = float(F(inv * F(p_)))
            t[p_, i] = m.cosf(ang); t[p_, half + i] = m.sinf(ang)
    return synth.round_bf16(t)


def matrix_from_probs_bound(p):
    """tests/align_ref.py's derivation from the normalisation on, for probabilities p [H][L][A] that are the kernel's own (no softmax error)"""
    H, L, A = p.shape
    U, gamma = R.U, R.gamma
    mu = p.mean(axis=1, keepdims=True)
    d = p - mu
    sd = np.sqrt((d ** 2).mean(axis=1, keepdims=True))
    e_mu = gamma(L + 1) * p.max(axis=1, keepdims=True)
    e_d = e_mu + U * np.abs(d).max(axis=1, keepdims=True)
    e_sd = e_d + gamma(L + 6) * (sd + e_d)
    thin = sd < R.THIN_FACTOR * e_sd
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd > 0, d / sd, 0.0)
        zb = (e_d + np.abs(z) * e_sd) / (sd - e_sd)
        zb = zb + U * (np.abs(z) + zb)
    zb = np.broadcast_to(np.where(thin, np.inf, zb), p.shape)
    win = R.reflect_index(A)
    zf = np.sort(z[..., win], axis=-1)[..., 3]
    zfb = zb[..., win].max(axis=-1)
    ok = np.isfinite(zfb).all(axis=0)
    M = sum(zf[h] / H for h in range(H))
    bound = np.where(ok, np.where(np.isfinite(zfb), zfb, 0.0).mean(axis=0) + gamma(H + 1) * np.abs(zf).mean(axis=0), np.inf)
    return {"M": M, "bound": bound, "ok": ok}


# ------------------------------------------------------------------------------------------ 2. same bits, whatever the batching
def test_same_bits_whatever_the_batching(eng, golden, base):
    segs, prompts, force = golden
    _, sc0, M0, A = base
    want_M, want_t = bits(M0[N:2 * N, :A[1]]), sc0[1].times

    def same(tag, e, sc, r, row0, n_rows, amax):
        M = e.debug_read("align_matrix", n_rows * amax).reshape(n_rows, amax)
        assert np.array_equal(bits(M[row0:row0 + N, :A[1]]), want_M), tag
        assert np.array_equal(sc[r].times, want_t) and np.array_equal(bits(sc[r].lp), bits(sc0[1].lp)), tag
    _, _, sc = eng.score_batch([segs[1]], [prompts[1]], force[1:2], align=True)                       # alone
    same("alone", eng, sc, 0, 0, N, A[1])
    other = synth.synth_pcm(700, 48000)                                                                # 3 s: another audio length in front
    rng = np.random.default_rng(3)
    f3 = [rng.integers(0, 900, 7).astype(np.int32), force[0], force[1]]
    _, _, sc = eng.score_batch([other, segs[0], segs[1]], [prompt_for(len(other)), prompts[0], prompts[1]], f3, align=True)
    same("3 of 3, other lengths beside it", eng, sc, 2, 7 + N, 7 + 2 * N, max(A))
    _, _, sc = eng.score_batch([segs[1]], [prompts[1]] * 3, [f3[0], force[1], force[0]], fanout=3, align=True)   # candidates of one audio
    same("forced_fanout", eng, sc, 1, 7, 7 + 2 * N, A[1])
    eng.set_option("score_chunk_rows", 16)
    try:
        _, _, sc = eng.score_batch(segs, prompts, force, align=True)
    finally:
        eng.set_option("score_chunk_rows", 256)
    same("chunks of 16", eng, sc, 1, N, 2 * N, max(A))
    s = eng.slot()                                                                                     # a slot copies the options and the heads
    _, _, sc = s.score_batch(segs, prompts, force, align=True)
    same("slot", s, sc, 1, N, 2 * N, max(A))


# ------------------------------------------------------------------------------------------ 3. the records' first floats keep their bits
@pytest.mark.parametrize("K", [0, 8])
def test_records_keep_their_bits(golden, K):
    from sonicscribe_amd.engine import AlignedScores
    segs, prompts, force = golden
    on, off = make(K=K), make(K=K, align=False)
    try:
        _, _, a = on.score_batch(segs, prompts, force, align=True)
        _, _, b = off.score_batch(segs, prompts, force)
        _, _, c = on.score_batch(segs, prompts, force)                      # scores alone from an align handle: what a plain handle returns
        for r in range(2):
            assert isinstance(a[r], AlignedScores) and a[r].times.shape == (N,)
            lp_b = b[r].lp if K else b[r]
            assert np.array_equal(bits(a[r].lp), bits(lp_b)) and np.array_equal(bits(c[r].lp if K else c[r]), bits(lp_b))
            if K:
                assert np.array_equal(bits(a[r].top_logprobs), bits(b[r].top_logprobs)) and np.array_equal(a[r].top_ids, b[r].top_ids)
        # the raw records: W = 1 + 2K + 1 floats, t_n last and exact
        on.set_forced_ids(force)
        try:
            ids, _ = on.transcribe_batch(segs, prompts, [N, N])
            W = 1 + 2 * K + 1
            raw = np.full((2, N * W), np.nan, F)
            on._check(on.lib.sonic_fetch_logprobs(on.h, raw.ctypes.data_as(__import__("ctypes").c_void_p), raw.shape[1]))
        finally:
            on.set_forced_ids(None)
        for r in range(2):
            rec = raw[r].reshape(N, W)
            assert np.array_equal(rec[:, W - 1], a[r].times.astype(F)) and np.array_equal(bits(rec[:, 0]), bits(a[r].lp))
    finally:
        on.close(); off.close()


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals(golden):
    from sonicscribe_amd.engine import Engine, MODE_F32, SonicError
    segs, prompts, force = golden
    e = make(align=False)
    try:
        with pytest.raises(SonicError, match="align=True.*forced_align"):
            e.score_batch(segs, prompts, force, align=True)
        e.set_option("forced_parallel", 0)
        with pytest.raises(SonicError, match="forced_align: option forced_parallel must be on first"):
            e.set_option("forced_align", 1)
        e.stage_pcm(segs)
        e.prefill(prompts, [8, 8])                                            # a batch in hand
        with pytest.raises(SonicError, match="forced_align.*still running"):
            e.set_option("forced_align", 1)
        with pytest.raises(SonicError, match="align_head.*still running"):
            e.set_option("align_head", 0)
        e.decode_step(8)
        e.set_option("forced_parallel", 1)
        e.set_option("forced_align", 1)
        with pytest.raises(SonicError, match="forced_parallel cannot be switched off while option forced_align is on"):
            e.set_option("forced_parallel", 0)
        for bad in (D.dec_layers * 256, D.dec_heads, -2, 256 * 256):
            with pytest.raises(SonicError, match="align_head: .* is outside"):
                e.set_option("align_head", bad)
        e.set_option("align_head", 256 + 1); e.set_option("align_head", 0); e.set_option("align_head", 256 + 1)      # twice: once
        _, _, sc = e.score_batch(segs, prompts, force, align=True)
        assert e.debug_read("align_probs", 1 * 2 * N * 1).shape == (2 * N,)   # the last selected layer (1) contributes one head
        e.set_option("align_head", -1)                                        # back to the default
        # the audio placeholders must be one run, and there must be one
        split = list(prompts[0]); split.insert(len(PRE) + 3, 7)
        with pytest.raises((SonicError, ValueError), match="not one contiguous run|do not match"):
            e.score_batch(segs, [split, prompts[1]], force, align=True)
        with pytest.raises(SonicError, match="out_ld too small"):
            e.set_forced_ids(force)
            try:
                e.transcribe_batch(segs, prompts, [N, N], want_logprobs=True)  # the narrow buffer of a caller that does not know the handle aligns
            finally:
                e.set_forced_ids(None)
    finally:
        e.close()
    f = Engine(D, 0, MODE_F32, max_batch=2, max_ctx=1024)
    try:
        f.set_option("forced_parallel", 1)
        with pytest.raises(SonicError, match="forced_align: the fp32 kind has no alignment kernels"):
            f.set_option("forced_align", 1)
    finally:
        f.close()


def test_head_list_is_capped():
    from dataclasses import replace
    from sonicscribe_amd.engine import Engine, SonicError
    e = Engine(replace(D, dec_layers=129), 0, 0, max_batch=1, max_ctx=256)   # 258 heads to choose from (no weights needed to set options)
    try:
        e.set_option("forced_parallel", 1)
        e.set_option("forced_align", 1)
        for c in range(256):
            e.set_option("align_head", (c // 2) * 256 + c % 2)
        with pytest.raises(SonicError, match="align_head: the list already holds 256 heads"):
            e.set_option("align_head", 128 * 256)
        e.set_option("align_head", 5 * 256 + 1)                               # one it already holds: nothing to add, nothing to refuse
    finally:
        e.close()


def test_int8_mode_handle(golden):
    """the fp16 instantiation behind an int8-mode prefill: the times are the restated DTW of the handle's own matrix"""
    segs, prompts, force = golden
    A = [int((np.asarray(p) == D.audio_token_id).sum()) for p in prompts]
    e = make(mode=1)
    try:
        _, _, sc = e.score_batch(segs, prompts, force, align=True)
        M = e.debug_read("align_matrix", 2 * N * max(A)).reshape(2 * N, max(A))
        for r in range(2):
            assert np.all(np.isfinite(M[r * N:(r + 1) * N, :A[r]])) and np.array_equal(sc[r].times, R.times_of(M[r * N:(r + 1) * N, :A[r]]))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 5. the two-window request
def test_two_window_request(golden_dir):
    m = np.load(os.path.join(golden_dir, "tiny_multi_bf16.npz"))
    pcm = synth.synth_pcm(int(m["seg_index"]), int(m["n_samples"]))
    wins = [pcm[s:e_] for s, e_ in frontend.split_windows(len(pcm), D)]
    total, per_win = frontend.request_audio_tokens(len(pcm), D)
    assert len(wins) == 2 and total == sum(per_win) == int(m["n_audio"])
    e = make(max_batch=2)
    try:
        from sonicscribe_amd import timestamps
        _, _, sc = e.score_batch(wins, [m["prompt_ids"]], m["force_ids"][None].astype(np.int32), req_win=[0, 2], align=True)
        t = sc[0].times
        sec = timestamps.audio_index_seconds(t, per_win, total, D.chunk_seconds)
        assert np.all(np.diff(t) >= 0) and np.all(np.diff(sec) >= 0) and t.min() >= 0 and t.max() < total
        assert np.array_equal(sec >= 30.0, t >= per_win[0])                 # beyond 30 s exactly where the index lies in the second window's range
        M = e.debug_read("align_matrix", len(t) * total).reshape(len(t), total)
        assert np.array_equal(t, R.times_of(M))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 6. ASRModel
def test_asrmodel_timestamps():
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.timestamps import Alignment
    from sonicscribe_amd import vad_net
    from sonicscribe_amd.vad import VADProcessor
    wavs = [synth.synth_pcm(31 + i, n).astype(np.float32) / 32768.0 for i, n in enumerate((80000, 120000))]
    m = ASRModel.from_synthetic(D, max_batch=8, max_ctx=1024, token_logprobs=True, scoring=True, timestamps=True)
    try:
        assert m.get_model_info()["timestamps"] is True

        def check(al_or_t, n_tokens, duration, offset=0.0):
            s, e_, words = al_or_t.token_start, al_or_t.token_end, al_or_t.words
            assert len(s) == len(e_) == n_tokens                             # one time per token
            assert np.all(np.diff(s) >= 0) and s.min() >= offset and s.max() <= offset + duration and np.array_equal(e_[:-1], s[1:]) and e_[-1] == pytest.approx(offset + duration)
            assert sorted(sum((w.tokens for w in words), [])) == list(range(n_tokens))      # the words partition the tokens
            assert all(0 <= w.probability <= 1 and w.start <= w.end for w in words)
        ids = [5, 17, 250, 33, 90, 412, 8]
        al = m.align(wavs[0], ids)
        assert isinstance(al, Alignment) and al.token_ids.tolist() == ids     # the appended EOS is dropped again
        check(al, len(ids), 5.0)
        both = m.align_batch(wavs, [ids, ids[:4]])
        assert np.array_equal(both[0].audio_index, al.audio_index) and np.array_equal(bits(both[0].token_logprobs), bits(al.token_logprobs))
        check(both[1], 4, 7.5)
        r = m.transcribe(wavs[0], max_new_tokens=12, word_timestamps=True)
        n = len(r.token_ids) - (1 if int(r.token_ids[-1]) in D.eos_ids else 0)
        check(r, n, 5.0)
        info = m.transcribe(wavs[1], max_new_tokens=12, word_timestamps=True, return_debug_info=True)
        assert len(info["token_start"]) == len(info["words"]) and {"word", "start", "end", "probability"} <= set(info["words"][0])
        plain = m.transcribe(wavs[0], max_new_tokens=12)
        assert plain == r.text                                               # the decode itself is unchanged
        rb = m.transcribe_batch(wavs, max_new_tokens=12, word_timestamps=True)
        assert rb[0].text == r.text and np.array_equal(rb[0].token_start, r.token_start)
        with pytest.raises(ValueError, match="word_timestamps is not supported on submit"):
            m.submit(wavs[0], word_timestamps=True)
        st = m.open_stream("s")
        try:
            with pytest.raises(ValueError, match="word_timestamps is not supported on submit"):
                st.submit_samples(0, 16000, word_timestamps=True)
        finally:
            st.close()
        # file mode: the words of every record are on the file's clock
        pcm = np.concatenate([np.zeros(16000, np.int16), synth.synth_pcm(5, 48000), np.zeros(24000, np.int16), synth.synth_pcm(6, 40000)])
        vad = VADProcessor(weights=vad_net.synthetic_weights(20260128, **vad_net.RESPONSIVE))
        try:
            recs = list(m.transcribe_file(pcm, vad, vad_enabled=False, max_segment_duration=3.0, max_new_tokens=8, word_timestamps=True))
        finally:
            vad.close()
        segs = [x for x in recs if x["type"] == "segment_result"]
        assert len(segs) >= 2 and not [x for x in recs if x["type"] == "segment_error"]
        for x in segs:
            assert x["words"] and all(x["start_time"] - 1e-9 <= w["start"] <= w["end"] <= x["end_time"] + 1e-6 for w in x["words"])
        assert segs[1]["words"][0]["start"] >= segs[1]["start_time"] > 0
    finally:
        m.close()
    m = ASRModel.from_synthetic(D, max_batch=4, max_ctx=1024, token_logprobs=True, scoring=True)
    try:
        with pytest.raises(ValueError, match="timestamps=True"):
            m.align(wavs[0], [1, 2, 3])
        with pytest.raises(ValueError, match="timestamps=True"):
            m.transcribe(wavs[0], word_timestamps=True)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 7. live transformers
def test_live_attention_distance(golden):
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    from tests import hf_helpers as H
    segs, prompts, force = golden
    si = 0
    pcm, prompt, f = segs[si], [int(t) for t in prompts[si]], force[si]
    A = int((np.asarray(prompt) == D.audio_token_id).sum()); a0 = prompt.index(D.audio_token_id)
    feats, mask = H.mel_case(H.feature_extractor(), pcm)
    ids = torch.tensor([prompt + [int(t) for t in f[:-1]]], dtype=torch.long)
    rows = len(prompt) - 1 + np.arange(N)
    ref = {}
    for tag, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        model, _ = H.build_tiny(dt)
        model.set_attn_implementation("eager")
        with torch.no_grad():
            out = model(input_ids=ids, input_features=torch.from_numpy(feats)[None].to(dt), input_features_mask=torch.from_numpy(mask)[None].long(),
                        attention_mask=torch.ones_like(ids), output_attentions=True)
        att = out.attentions[-1][0].float().numpy().astype(np.float64)       # the last decoder layer [H][T][T]
        p = att[:, rows, a0:a0 + A]
        ref[tag] = p / p.sum(axis=-1, keepdims=True)                         # renormalised over the audio run
    e = make(heads=[(D.dec_layers - 1, h) for h in range(D.dec_heads)])
    try:
        e.score_batch([pcm], [prompt], f[None], align=True)
        got = e.debug_read("align_probs", D.dec_heads * N * A).reshape(D.dec_heads, N, A).astype(np.float64)
    finally:
        e.close()
    d_ref, d_got = np.abs(ref["bf16"] - ref["fp32"]), np.abs(got - ref["fp32"])
    print(f"align_probs against live transformers: max |HIP - fp32| {d_got.max():.3e} vs reference bf16 {d_ref.max():.3e} (ratio {d_got.max() / d_ref.max():.2f}); "
          f"mean {d_got.mean():.3e} vs {d_ref.mean():.3e} (ratio {d_got.mean() / d_ref.mean():.2f})")
    assert d_got.max() <= FACTOR * d_ref.max() and d_got.mean() <= FACTOR * d_ref.mean()
