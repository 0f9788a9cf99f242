"""Transcript scoring in one prefill pass (option forced_parallel, Engine.score_batch, ASRModel.score).  With forced ids set and the option on, a run
is ONE prefill of prompt || forced ids, the tied lm_head over every forced position as a GEMM per chunk of score rows, and rows_kernel (csrc/rows.hip) per row.

References and tolerances:
  * tests/golden/tiny_forced_{bf16,fp32}.npz: two segments (5 s, 20 s), 24 forced ids each, HF's per-step logits under teacher forcing.  bf16: the project's logit
    tolerance 4 * 2^-6 (tests/test_gpu_parity.py) and twice that for log-probabilities (log-sum-exp is 1-Lipschitz in the sup norm: tests/test_gpu_logprobs.py);
    fp32 kind: 1e-3 (tests/test_gpu_fp32_mode.py) and 2e-3 by the same argument - the tight check: an off-by-one in the score-row positions or the causal mask
    cannot pass it.
  * the handle's own returned logits: the bound derived for the row kernel (tests/test_gpu_score_kernel.py states it).
  * everything else is bit equality.

Figures printed for DESIGN.md 6.8 (one MI355X): the first 12 records of the 24-token run were bit-equal to a 12-token run on both segments; the parallel run against
the step-by-step forced run: max |d lp| = 0.015, max |d logit| = 0.031."""
from functools import partial

import numpy as np
import pytest

import gpu_common
from gpu_common import bits, flags, forced_ids, load_golden, make_engine, ref_logprob, score_bound
from sonicscribe_amd import spec, synth

pytestmark = pytest.mark.gpu
D = spec.TINY
TOL_LOGIT = 4 * 2.0 ** -6
TOL_FIXTURE = 2 * 4 * 2.0 ** -6
N = 24
prompt_for = partial(gpu_common.prompt_for, D)


def make(mode=0, max_batch=4, max_ctx=1024, lp=True, parallel=True, opts=()):
    return make_engine(D, mode, max_batch, max_ctx, flags((lp, "token_logprobs", 1)) + list(opts) + flags((parallel, "forced_parallel", 1)))


def load(golden_dir, name):
    g, segs, prompts = load_golden(golden_dir, name)
    force = forced_ids(g)
    assert force.shape == (2, N)
    return g, segs, prompts, force


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load(golden_dir, "tiny_forced_bf16.npz")


@pytest.fixture(scope="module")
def eng():
    e = make()
    yield e
    e.close()


@pytest.fixture(scope="module")
def base(eng, golden):
    """the two fixture sequences scored once (with logits): shared by the tests below, never changed"""
    _, segs, prompts, force = golden
    return eng.score_batch(segs, prompts, force, want_logits=True)


def check_own_bound(tag, lps, logits, force):
    V = logits.shape[-1]
    ref = ref_logprob(logits, force)
    err = np.abs(np.asarray(lps, np.float64) - ref)
    ratio = float((err / score_bound(V, ref)).max())
    print(f"{tag}: worst |lp - ref64(own logits)| / bound = {ratio:.3f} (max err {err.max():.3e})")
    assert np.all(np.isfinite(lps)) and ratio <= 1.0, (tag, ratio)


# ------------------------------------------------------------------------------------------ 1 / 2. against the reference
def test_reference_bf16(eng, golden, base):
    g, segs, prompts, force = golden
    ids, logits, lps = base
    assert logits.shape == (N, 2, D.vocab)
    for si in range(2):
        assert len(ids[si]) == N and np.array_equal(ids[si], force[si])
        dl = np.abs(logits[:, si] - g[f"s{si}_step_logits"]).max()
        ref_lp = ref_logprob(g[f"s{si}_step_logits"], force[si])
        dp = np.abs(lps[si] - ref_lp).max()
        print(f"score bf16 s{si}: max |logit - fixture| = {dl:.4f} (tol {TOL_LOGIT}), max |lp - fixture| = {dp:.4f} (tol {TOL_FIXTURE})")
        assert dl <= TOL_LOGIT and dp <= TOL_FIXTURE
        check_own_bound(f"score bf16 s{si}", lps[si], logits[:, si], force[si])
    assert eng.decode_step(4) == (0, 0)                                  # a finished batch: nothing active, nothing left to run
    t = eng.timings()
    assert t["decode_steps"] == 0 and t["prefill_ms"] > 0 and t["encoder_ms"] > 0


def test_reference_fp32_kind(golden_dir):
    from sonicscribe_amd.engine import MODE_F32
    from sonicscribe_amd.engine import Engine
    g, segs, prompts, force = load(golden_dir, "tiny_forced_fp32.npz")
    e = Engine(D, 0, MODE_F32, max_batch=2, max_ctx=1024)                 # the fixture's fp32 weights, as tests/test_gpu_fp32_mode.py loads them
    e.set_option("token_logprobs", 1)
    e.set_option("forced_parallel", 1)
    e.load_state_dict(synth.synth_state_dict(D, int(g["seed"]), bf16=False))
    try:
        ids, logits, lps = e.score_batch(segs, prompts, force, want_logits=True)
        for si in range(2):
            assert np.array_equal(ids[si], force[si])
            dl = np.abs(logits[:, si] - g[f"s{si}_step_logits"]).max()
            dp = np.abs(lps[si] - ref_logprob(g[f"s{si}_step_logits"], force[si])).max()
            print(f"score fp32 kind s{si}: max |logit - fixture| = {dl:.2e} (tol 1e-3), max |lp - fixture| = {dp:.2e} (tol 2e-3)")
            assert dl <= 1e-3 and dp <= 2e-3
            check_own_bound(f"score fp32 kind s{si}", lps[si], logits[:, si], force[si])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 3. the other kinds
@pytest.mark.parametrize("mode", [1, 2])
def test_modes_bound(mode, golden):
    _, segs, prompts, force = golden
    e = make(mode=mode)
    try:
        ids, logits, lps = e.score_batch(segs, prompts, force, want_logits=True)
        for si in range(2):
            assert np.array_equal(ids[si], force[si]) and len(lps[si]) == N
            check_own_bound(f"score mode {mode} s{si}", lps[si], logits[:, si], force[si])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 4. same bits, whatever the batching
def test_same_bits_whatever_the_batching(eng, golden, base):
    _, segs, prompts, force = golden
    ids0, logits0, lps0 = base
    want_lp, want_lg = bits(lps0[1]), bits(logits0[:, 1])

    def same(tag, lps, logits, r):
        assert np.array_equal(bits(lps[r]), want_lp), tag
        assert np.array_equal(bits(logits[:N, r]), want_lg), tag
    _, lg, lp = eng.score_batch([segs[1]], [prompts[1]], force[1:2], want_logits=True)                  # alone
    same("alone", lp, lg, 0)
    other = synth.synth_pcm(700, 48000)
    rng = np.random.default_rng(3)
    f3 = np.stack([rng.integers(0, 900, N), rng.integers(0, 900, N), force[1]]).astype(np.int32)
    _, lg, lp = eng.score_batch([other, segs[0], segs[1]], [prompt_for(len(other)), prompts[0], prompts[1]], f3, want_logits=True)   # sequence 2 of 3, other audio in front
    same("2 of 3", lp, lg, 2)
    eng.set_option("score_chunk_rows", 16)                                # 2 x 24 rows: the sequence's rows 24 .. 47 straddle the chunks [16, 32) and [32, 48)
    try:
        _, lg, lp = eng.score_batch(segs, prompts, force, want_logits=True)
    finally:
        eng.set_option("score_chunk_rows", 256)
    same("chunks of 16", lp, lg, 1)
    assert np.array_equal(bits(lp[0]), bits(lps0[0]))
    s = eng.slot()                                                        # a slot copies the option
    _, lg, lp = s.score_batch(segs, prompts, force, want_logits=True)
    same("slot", lp, lg, 1)


def test_alternatives_ride_along(golden, base):
    _, segs, prompts, force = golden
    e = make(opts=(("top_logprobs", 3),))
    try:
        ids, logits, sc = e.score_batch(segs, prompts, force, want_logits=True)
        for si in range(2):
            lp, top_lp, top_ids = sc[si]
            assert np.array_equal(bits(lp), bits(base[2][si]))            # the alternatives change no bit of the token's own value
            assert top_lp.shape == (N, 3) and top_ids.shape == (N, 3)
            for n in range(N):
                order = np.lexsort((np.arange(D.vocab), -logits[n, si].astype(np.float64)))[:3]
                assert np.array_equal(top_ids[n], order)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 5. fan-out
def test_fanout_shares_the_encoder(golden):
    _, segs, prompts, force = golden
    rng = np.random.default_rng(11)
    f3 = np.stack([force[1], rng.integers(0, 900, N), np.roll(force[1], 5)]).astype(np.int32)
    e = make(opts=(("gemm_timing", 1),))
    try:
        ids_a, lg_a, lp_a = e.score_batch([segs[1]], [prompts[1]] * 3, f3, fanout=3, want_logits=True)
        t_a = e.timings()
        ids_b, lg_b, lp_b = e.score_batch([segs[1]] * 3, [prompts[1]] * 3, f3, want_logits=True)
        t_b = e.timings()
        for r in range(3):
            assert np.array_equal(ids_a[r], ids_b[r]) and np.array_equal(ids_a[r], f3[r])
            assert np.array_equal(bits(lp_a[r]), bits(lp_b[r]))
        assert np.array_equal(bits(lg_a), bits(lg_b))
        # one encoder pass's worth: the encoder's GEMM work is counted per staged window (sonic_timings.enc_gemm_flops, option gemm_timing)
        assert t_a["enc_gemm_flops"] > 0 and t_b["enc_gemm_flops"] == 3 * t_a["enc_gemm_flops"]
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 6. the EOS rule
def test_eos_rule(eng, golden, base):
    _, segs, prompts, force = golden
    f = force.copy()
    f[1, 9] = D.eos_ids[1]
    full_ids, full_lg, full_lp = eng.score_batch(segs, prompts, force, want_logits=True)      # fills the handle's step-logits buffer with the 24-token run
    ids, lg, lp = eng.score_batch(segs, prompts, f, want_logits=True)
    assert len(ids[1]) == 10 and len(lp[1]) == 10 and np.array_equal(ids[1], f[1, :10]) and len(ids[0]) == N
    cut_ids, cut_lg, cut_lp = eng.score_batch(segs, prompts, [f[0], f[1, :10]], want_logits=True)
    assert len(cut_ids[1]) == 10
    assert np.array_equal(bits(lp[1]), bits(cut_lp[1])) and np.array_equal(bits(lg[:10, 1]), bits(cut_lg[:10, 1]))
    assert np.array_equal(bits(lg[10:, 1]), bits(full_lg[10:, 1]))        # nothing is written beyond: the buffer still holds the earlier run's rows


# ------------------------------------------------------------------------------------------ 7. prefix property
def test_prefix_property(eng, golden, base):
    _, segs, prompts, force = golden
    ids, lg, lp = eng.score_batch(segs, prompts, force[:, :12].copy(), want_logits=True)
    for si in range(2):
        assert len(lp[si]) == 12
        d = np.abs(lp[si] - base[2][si][:12]).max()
        same = np.array_equal(bits(lp[si]), bits(base[2][si][:12]))
        print(f"score prefix s{si}: first 12 of 24 against a 12-token run: max |d lp| = {d:.3e}, bit-equal: {same}")
        assert d <= TOL_FIXTURE


# ------------------------------------------------------------------------------------------ 8. beside the step-by-step path
def test_beside_the_step_by_step_path(eng, golden, base):
    _, segs, prompts, force = golden
    eng.set_option("forced_parallel", 0)
    eng.set_forced_ids(force)
    try:
        ids, logits, lps = eng.transcribe_batch(segs, prompts, [N, N], want_logits=True, want_logprobs=True)
    finally:
        eng.set_forced_ids(None)
        eng.set_option("forced_parallel", 1)
    for si in range(2):
        assert np.array_equal(ids[si], force[si])
        d = np.abs(lps[si] - base[2][si]).max()
        dl = np.abs(logits[:N, si] - base[1][:, si]).max()
        print(f"score s{si}: parallel against step by step: max |d lp| = {d:.4f} (tol {2 * TOL_FIXTURE}), max |d logit| = {dl:.4f}")
        assert d <= 2 * TOL_FIXTURE


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(golden):
    from sonicscribe_amd.engine import SonicError
    _, segs, prompts, force = golden
    e = make(parallel=False, opts=(("request_bias", 1),))
    try:
        e.stage_pcm(segs)
        e.prefill(prompts, [8, 8])                                        # a batch in hand
        with pytest.raises(SonicError, match="forced_parallel"):
            e.set_option("forced_parallel", 1)
        e.decode_step(8)
        e.set_option("forced_parallel", 1)
        with pytest.raises(SonicError, match="forced_fanout"):            # R not divisible by the fan-out
            e.score_batch([segs[0]], [prompts[0]] * 3, np.stack([force[0]] * 3), fanout=2)
        bad = force.copy(); bad[0, 3] = D.audio_token_id
        with pytest.raises(SonicError, match="placeholder"):
            e.score_batch(segs, prompts, bad)
        e.set_request_bias([None, None])                                  # staged tables: the parallel run applies no processors
        with pytest.raises(SonicError, match="no processors"):
            e.score_batch(segs, prompts, force)
        ids, _, lps = e.score_batch(segs, prompts, force)                 # ... and the refusal consumed them
        assert np.array_equal(ids[1], force[1])
        with pytest.raises(SonicError, match="forced_parallel"):
            e.service_begin()
        e.stage_pcm(segs)
        with pytest.raises(SonicError, match="forced_parallel"):
            e.prefill(prompts, [8, 8])
        with pytest.raises(SonicError, match="forced_parallel"):
            e.prefill(prompts, [8, 8], wait=False)
    finally:
        e.close()
    o = make(parallel=False)
    try:
        s = o.slot()
        s.set_option("forced_parallel", 1)                                # on a slot alone
        o.service_begin()
        with pytest.raises(SonicError, match="forced_parallel.*source"):
            o.splice_rows(s, [0], [0])
        with pytest.raises(SonicError, match="forced_parallel.*destination"):
            s.splice_rows(o, [0], [0])
        o.service_end()
        ids, _, lps = s.score_batch(segs, prompts, force)                 # the slot scores beside its owner
        assert np.array_equal(ids[0], force[0]) and len(lps[0]) == N
    finally:
        o.close()
    big = make(max_batch=1, max_ctx=1024, lp=False)                       # tok_cap = 1 x (375 audio rows + 256) = 631
    try:
        seg = synth.synth_pcm(5, 480000)
        p = prompt_for(len(seg))
        assert len(p) + 260 <= 1024 and len(p) + 259 > big.tok_cap
        with pytest.raises(SonicError, match=r"tokens.*tok_cap"):
            big.score_batch([seg], [p], np.full((1, 260), 5, np.int32))
        ids, _, lps = big.score_batch([segs[0]], [prompts[0]], force[:1])
        assert lps is None and np.array_equal(ids[0], force[0])
        with pytest.raises(SonicError, match="token_logprobs"):           # log-probabilities need their option, as today
            big._fetch_logprobs([N], N)
    finally:
        big.close()
    plain = make(parallel=False)
    try:
        with pytest.raises(SonicError, match="forced_parallel"):
            plain.score_batch(segs, prompts, force)
    finally:
        plain.close()


# ------------------------------------------------------------------------------------------ 10. the runs' shared prologue, one kind of run after the other
def test_greedy_score_greedy_on_one_handle(golden):
    """run_to_first_token and run_forced_parallel begin and end through the same helpers (staging-buffer pick, step-logits dump, closing state): a greedy run, a
    parallel forced run and the greedy run again on ONE handle.  Each comparison is one deterministic path run twice: bit equality."""
    _, segs, prompts, force = golden
    e, fresh = make(max_batch=2), make(max_batch=2)
    try:
        ids1, lg1 = e.transcribe_batch(segs, prompts, [4, 4], want_logits=True)
        ids2, lg2, lp2 = e.score_batch(segs, prompts, force, want_logits=True)
        ids3, lg3 = e.transcribe_batch(segs, prompts, [4, 4], want_logits=True)
        ids0, lg0, lp0 = fresh.score_batch(segs, prompts, force, want_logits=True)
        assert lg1.shape == (4, 2, D.vocab) and lg2.shape == (N, 2, D.vocab)
        for si in range(2):
            assert np.array_equal(ids3[si], ids1[si])
            assert np.array_equal(ids2[si], ids0[si]) and np.array_equal(bits(lp2[si]), bits(lp0[si]))
        assert np.array_equal(bits(lg3), bits(lg1))
        assert np.array_equal(bits(lg2), bits(lg0))
    finally:
        e.close()
        fresh.close()


# ------------------------------------------------------------------------------------------ 11. ASRModel
def test_asrmodel_score():
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.scoring import Score
    wavs = [synth.synth_pcm(31 + i, n).astype(np.float32) / 32768.0 for i, n in enumerate((80000, 120000))]
    with pytest.raises(ValueError, match="token_logprobs"):
        ASRModel.from_synthetic(D, max_batch=8, max_ctx=1024, scoring=True)
    m = ASRModel.from_synthetic(D, max_batch=8, max_ctx=1024, token_logprobs=True, scoring=True, top_logprobs=2)
    try:
        assert m.get_model_info()["scoring"] is True
        r = m.submit(wavs[0], max_new_tokens=16, detailed=True).result(timeout=60)
        n = len(r.token_ids)
        other = r.token_ids.copy(); other[n // 2] = (int(other[n // 2]) + 1) % 900
        sc = m.score(wavs[0], [r.token_ids, other], append_eos=False)
        assert len(sc) == 2 and all(isinstance(s, Score) for s in sc)
        assert np.array_equal(sc[0].token_ids, r.token_ids) and sc[0].text == r.text
        d = np.abs(sc[0].token_logprobs - r.token_logprobs).max()
        print(f"ASRModel.score of the greedy transcript against its own token_logprobs: max |d lp| = {d:.4f} (tol {2 * TOL_FIXTURE})")
        assert d <= 2 * TOL_FIXTURE
        for s in sc:
            k = len(s.token_ids)
            assert s.token_logprobs.shape == (k,) and s.top_token_ids.shape == (k, 2) and s.top_logprobs.shape == (k, 2)
            assert s.sum_logprob == float(np.sum(s.token_logprobs, dtype=np.float64)) and abs(s.avg_logprob - s.sum_logprob / k) <= 1e-12
        with pytest.raises(ValueError, match="tokenizer"):
            m.score(wavs[0], ["a text candidate"])
        # 2 audios x 3 candidates of unequal length: the same bits as six single calls
        rng = np.random.default_rng(2)
        cands = [[list(map(int, rng.integers(0, 900, k))) for k in ks] for ks in ((5, 9, 3), (7, 2, 11))]
        both = m.score_batch(wavs, cands)
        idle = {}
        for a in range(2):
            for c in range(3):
                one = m.score(wavs[a], [cands[a][c]])[0]
                idle[(a, c)] = one
                assert np.array_equal(one.token_ids, both[a][c].token_ids) and one.token_ids[-1] == D.eos_ids[0] and len(one.token_ids) == len(cands[a][c]) + 1
                assert np.array_equal(bits(one.token_logprobs), bits(both[a][c].token_logprobs))
                assert np.array_equal(one.top_token_ids, both[a][c].top_token_ids) and np.array_equal(bits(one.top_logprobs), bits(both[a][c].top_logprobs))
        uneven = m.score_batch(wavs, [cands[0], cands[1][:1]])             # unequal candidate counts: dummies, cut again
        assert [len(x) for x in uneven] == [3, 1] and np.array_equal(bits(uneven[1][0].token_logprobs), bits(idle[(1, 0)].token_logprobs))
        # four requests in flight while score() runs: the same bits as the idle call, and the transcripts are unchanged
        quiet = [m.submit(w, max_new_tokens=24).result(timeout=60) for w in (wavs[0], wavs[1], wavs[0], wavs[1])]
        futs = [m.submit(w, max_new_tokens=24) for w in (wavs[0], wavs[1], wavs[0], wavs[1])]
        busy = m.score(wavs[1], cands[1])
        assert [f.result(timeout=60) for f in futs] == quiet
        for c in range(3):
            assert np.array_equal(bits(busy[c].token_logprobs), bits(idle[(1, c)].token_logprobs))
    finally:
        m.close()
    m = ASRModel.from_synthetic(D, max_batch=4, max_ctx=1024, token_logprobs=True)
    try:
        assert m.get_model_info()["scoring"] is False
        with pytest.raises(ValueError, match="scoring"):
            m.score(wavs[0], [[1, 2, 3]])
    finally:
        m.close()
