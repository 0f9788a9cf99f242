"""The candidates of one audio share ONE prefill of their prompt (option forced_share_prompt, Engine.score_batch(share_prompt=True), ASRModel.score(share_prompt=True);
DESIGN.md 6.14).  The first sequence of a group packs prompt || forced[0 .. L - 1) as ever; every other one packs only its forced[0 .. L - 1) at positions P on of its
own cache row, and its attention reads keys [0, P) from the first one's row (csrc/attn.hip, flash_attn_kernel<.., PFX>).

References and tolerances (TINY, tests/golden/tiny_forced_bf16.npz; the values of tests/test_gpu_score.py):
  * the fixture: TOL_LOGIT = 4 * 2^-6 on the logits, TOL_FIXTURE = 2 * TOL_LOGIT on the log-probabilities;
  * the unshared run on the same handle: twice those - the cross-path margin test_beside_the_step_by_step_path uses (two paths, each within the tolerance of the truth);
  * the handle's own returned logits: the row kernel's derived bound (gpu_common.score_bound);
  * everything else is bit equality.  The shared form is NOT bit-equal to the unshared one: its attention takes the key tile that holds P twice, once per row.

Figures printed for DESIGN.md 6.14 (one MI355X): see the table there."""
from functools import partial

import numpy as np
import pytest

import gpu_common
from gpu_common import bits, flags, forced_ids, load_golden, make_engine, ref_logprob, score_bound
from sonicscribe_amd import spec, synth
from sonicscribe_amd.engine import MODE_F32, MODE_INT8, SonicError

pytestmark = pytest.mark.gpu
D = spec.TINY
TOL_LOGIT = 4 * 2.0 ** -6
TOL_FIXTURE = 2 * TOL_LOGIT
N = 24
prompt_for = partial(gpu_common.prompt_for, D)


def make(mode=0, max_batch=4, parallel=True, opts=()):
    return make_engine(D, mode, max_batch, 1024, [("token_logprobs", 1)] + list(opts) + flags((parallel, "forced_parallel", 1)))


def rand_ids(rng, n):
    """n ids that are neither an EOS id nor the audio placeholder"""
    ids = rng.integers(0, 900, n)
    ids[np.isin(ids, list(D.eos_ids) + [D.audio_token_id])] = 5
    return ids.astype(np.int32)


@pytest.fixture(scope="module")
def golden(golden_dir):
    g, segs, prompts = load_golden(golden_dir, "tiny_forced_bf16.npz", int_prompts=True)
    force = forced_ids(g)
    assert force.shape == (2, N)
    return g, segs, prompts, force


@pytest.fixture(scope="module")
def eng():
    e = make()
    yield e
    e.close()


def group_of(force_s, seed):
    """three candidates, the fixture's not first"""
    return np.stack([rand_ids(np.random.default_rng(seed), N), force_s, np.roll(force_s, 5)]).astype(np.int32)


@pytest.fixture(scope="module")
def runs(eng, golden):
    """per fixture segment a group of three, shared and unshared on the same handle (with logits): computed once, never changed"""
    _, segs, prompts, force = golden
    out = []
    for s in range(2):
        f3 = group_of(force[s], 40 + s)
        shared = eng.score_batch([segs[s]], [prompts[s]] * 3, f3, fanout=3, want_logits=True, share_prompt=True)
        tokens = int(eng.debug_read("score_tokens", (1,))[0])
        plain = eng.score_batch([segs[s]], [prompts[s]] * 3, f3, fanout=3, want_logits=True)
        out.append((f3, shared, plain, tokens, int(eng.debug_read("score_tokens", (1,))[0])))
    return out


# ------------------------------------------------------------------------------------------ 1. the fixture
def test_fixture(golden, runs):
    g, _, _, force = golden
    for s in range(2):
        f3, (ids, logits, lps), _, _, _ = runs[s]
        assert logits.shape == (N, 3, D.vocab) and np.array_equal(ids[1], force[s]) and len(lps[1]) == N
        dl = np.abs(logits[:, 1] - g[f"s{s}_step_logits"]).max()
        dp = np.abs(lps[1] - ref_logprob(g[f"s{s}_step_logits"], force[s])).max()
        print(f"share_prompt s{s}: the fixture sequence as sequence 1 of 3: max |logit - fixture| = {dl:.4f} (tol {TOL_LOGIT}), max |lp - fixture| = {dp:.4f} (tol {TOL_FIXTURE})")
        assert dl <= TOL_LOGIT and dp <= TOL_FIXTURE


# ------------------------------------------------------------------------------------------ 2. shared against unshared
def test_shared_against_unshared(runs):
    for s in range(2):
        f3, (ids, logits, lps), (ids0, logits0, lps0), _, _ = runs[s]
        for r in range(3):
            assert np.array_equal(ids[r], ids0[r]) and np.array_equal(ids[r], f3[r])
            dl = np.abs(logits[:, r] - logits0[:, r]).max()
            dp = np.abs(lps[r] - lps0[r]).max()
            print(f"share_prompt s{s} sequence {r}: shared against unshared: max |d logit| = {dl:.4f} (tol {2 * TOL_LOGIT}), max |d lp| = {dp:.4f} (tol {2 * TOL_FIXTURE}), "
                  f"bit-equal: {np.array_equal(bits(lps[r]), bits(lps0[r]))}")
            assert dl <= 2 * TOL_LOGIT and dp <= 2 * TOL_FIXTURE


# ------------------------------------------------------------------------------------------ 3. token 0 is one hidden row
def test_token_0_is_one_row(runs):
    for s in range(2):
        _, (_, logits, _), _, _, _ = runs[s]
        for r in (1, 2):
            assert np.array_equal(bits(logits[0, r]), bits(logits[0, 0])), (s, r)


# ------------------------------------------------------------------------------------------ 4. the handle's own bound
def test_own_bound(runs):
    for s in range(2):
        f3, (_, logits, lps), _, _, _ = runs[s]
        for r in range(3):
            ref = ref_logprob(logits[:, r], f3[r])
            err = np.abs(np.asarray(lps[r], np.float64) - ref)
            ratio = float((err / score_bound(D.vocab, ref)).max())
            print(f"share_prompt s{s} sequence {r}: worst |lp - ref64(own logits)| / bound = {ratio:.3f}")
            assert np.all(np.isfinite(lps[r])) and ratio <= 1.0


# ------------------------------------------------------------------------------------------ 5. same bits inside the shared form
def test_same_bits_inside_the_shared_form(eng, golden, runs):
    _, segs, prompts, force = golden
    f3, (_, logits, lps), _, _, _ = runs[1]
    want_lp, want_lg = bits(lps[1]), bits(logits[:, 1])

    def same(tag, e, targets, r, **kw):
        _, lg, lp = e.score_batch([segs[1]], [prompts[1]] * len(targets), targets, fanout=len(targets), want_logits=True, share_prompt=True, **kw)
        assert np.array_equal(bits(lp[r]), want_lp), tag
        assert np.array_equal(bits(lg[:N, r]), want_lg), tag
    rng = np.random.default_rng(77)
    same("position 2, other neighbours", eng, [rand_ids(rng, N), rand_ids(rng, N), force[1]], 2)
    same("position 1, a shorter owner and a one-token neighbour", eng, [rand_ids(rng, 7), force[1], rand_ids(rng, 1)], 1)
    same("position 1 of 2", eng, [rand_ids(rng, 16), force[1]], 1)
    for rows in (16, 256):
        eng.set_option("score_chunk_rows", rows)
        try:
            same(f"chunks of {rows}", eng, f3, 1)
        finally:
            eng.set_option("score_chunk_rows", 256)
    same("slot", eng.slot(), f3, 1)                                        # a slot copies the options the run reads


def test_suffix_rows_append_the_bits_of_an_unshared_run(eng, golden, runs):
    """layer 0's K / V cache: a sharer's suffix tokens, appended at positions P .. P + L - 2 of its own row from tiles that start at P, hold the bits the unshared run
    writes for those tokens at those positions (layer 0: their inputs are embedding rows, so nothing upstream differs); below P the sharer's row is left alone"""
    _, segs, prompts, force = golden
    f3 = runs[0][0]
    P = len(prompts[0])
    shape = (4, D.dec_kv_heads, 1024, D.dec_head_dim)
    eng.score_batch([segs[0]], [prompts[0]] * 3, f3, fanout=3)
    k0, v0 = eng.debug_read("kcache", shape), eng.debug_read("vcache", shape)
    eng.score_batch([segs[0]], [prompts[0]] * 3, f3, fanout=3, share_prompt=True)
    k1, v1 = eng.debug_read("kcache", shape), eng.debug_read("vcache", shape)
    for r in range(3):
        assert np.array_equal(bits(k1[r, :, P:P + N - 1]), bits(k0[r, :, P:P + N - 1])) and np.array_equal(bits(v1[r, :, P:P + N - 1]), bits(v0[r, :, P:P + N - 1])), r
    assert np.array_equal(bits(k1[0, :, :P]), bits(k0[0, :, :P])) and np.array_equal(bits(v1[0, :, :P]), bits(v0[0, :, :P]))       # the owner's prompt rows
    assert np.array_equal(bits(k1[1:3, :, :P]), bits(k0[1:3, :, :P]))                                                             # not rewritten: still the unshared run's


# ------------------------------------------------------------------------------------------ 6. mixed lengths
def test_mixed_lengths(eng, golden):
    _, segs, prompts, force = golden
    cut = force[0].copy(); cut[9] = D.eos_ids[1]
    rng = np.random.default_rng(8)
    for order in ([0, 1, 2], [2, 0, 1]):                                   # the 24-token one first, then the one-token candidate first (an owner without suffix rows)
        targets = [[force[0], rand_ids(rng, 1), cut][i] for i in order]
        ids, lg, lp = eng.score_batch([segs[0]], [prompts[0]] * 3, targets, fanout=3, want_logits=True, share_prompt=True)
        ids0, lg0, lp0 = eng.score_batch([segs[0]], [prompts[0]] * 3, targets, fanout=3, want_logits=True)
        assert [len(x) for x in ids] == [[N, 1, 10][i] for i in order] and [len(x) for x in lp] == [len(x) for x in ids]
        for r in range(3):
            n = len(ids[r])
            assert np.array_equal(ids[r], ids0[r]) and np.array_equal(ids[r], np.asarray(targets[r])[:n])
            assert np.abs(lg[:n, r] - lg0[:n, r]).max() <= 2 * TOL_LOGIT and np.abs(lp[r] - lp0[r]).max() <= 2 * TOL_FIXTURE


# ------------------------------------------------------------------------------------------ 7. two audios of different P
def test_two_audios(eng, golden):
    g, segs, prompts, force = golden
    assert len(prompts[0]) != len(prompts[1])
    rng = np.random.default_rng(12)
    targets = [rand_ids(rng, 13), force[0], rand_ids(rng, N), force[1]]
    run_prompts = [prompts[0], prompts[0], prompts[1], prompts[1]]
    ids, lg, lp = eng.score_batch(segs, run_prompts, targets, fanout=2, want_logits=True, share_prompt=True)
    assert int(eng.debug_read("score_tokens", (1,))[0]) == len(prompts[0]) + len(prompts[1]) + 12 + 3 * (N - 1)
    ids0, lg0, lp0 = eng.score_batch(segs, run_prompts, targets, fanout=2, want_logits=True)
    for r in range(4):
        n = len(targets[r])
        assert np.array_equal(ids[r], targets[r]) and np.abs(lg[:n, r] - lg0[:n, r]).max() <= 2 * TOL_LOGIT and np.abs(lp[r] - lp0[r]).max() <= 2 * TOL_FIXTURE
    for s, r in ((0, 1), (1, 3)):
        assert np.abs(lg[:, r] - g[f"s{s}_step_logits"]).max() <= TOL_LOGIT
        assert np.abs(lp[r] - ref_logprob(g[f"s{s}_step_logits"], force[s])).max() <= TOL_FIXTURE
    assert np.array_equal(bits(lg[0, 0]), bits(lg[0, 1])) and np.array_equal(bits(lg[0, 2]), bits(lg[0, 3]))


# ------------------------------------------------------------------------------------------ 8. token accounting
def test_token_accounting(eng, golden, runs):
    _, segs, prompts, force = golden
    for s in range(2):
        P = len(prompts[s])
        assert runs[s][3] == P + 3 * (N - 1) and runs[s][4] == 3 * (P + N - 1)
    eng.set_option("forced_share_prompt", 1)                              # a slot created now inherits the option, as it inherits forced_fanout
    try:
        slot = eng.slot()
    finally:
        eng.set_option("forced_share_prompt", 0)
    _, _, lp = slot.score_batch([segs[1]], [prompts[1]] * 3, runs[1][0], fanout=3)
    assert int(slot.debug_read("score_tokens", (1,))[0]) == runs[1][3] and np.array_equal(bits(lp[1]), bits(runs[1][1][2][1]))
    # a run that only the shared form holds: 4 candidates of L targets on a 30 s audio, 4 (P + L - 1) > tok_cap >= P + 4 (L - 1)
    seg = synth.synth_pcm(5, 480000)
    p = prompt_for(len(seg))
    P, L, cap = len(p), 260, eng.tok_cap
    assert 4 * (P + L - 1) > cap >= P + 4 * (L - 1) and P + L <= 1024
    targets = np.stack([rand_ids(np.random.default_rng(20 + r), L) for r in range(4)])
    with pytest.raises(SonicError, match=r"tokens.*tok_cap"):
        eng.score_batch([seg], [p] * 4, targets, fanout=4)
    ids, _, lps = eng.score_batch([seg], [p] * 4, targets, fanout=4, share_prompt=True)
    assert int(eng.debug_read("score_tokens", (1,))[0]) == P + 4 * (L - 1)
    assert all(np.array_equal(ids[r], targets[r]) and len(lps[r]) == L and np.all(np.isfinite(lps[r])) for r in range(4))
    one, _, lp1 = eng.score_batch([seg], [p], targets[2:3])                 # ... and what it returns for a sequence is what that sequence scores alone
    assert np.abs(lps[2] - lp1[0]).max() <= 2 * TOL_FIXTURE


# ------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(golden):
    _, segs, prompts, force = golden
    f2 = np.stack([force[0], np.roll(force[0], 3)])
    e = make(parallel=False)
    try:
        with pytest.raises(SonicError, match="forced_share_prompt.*forced_parallel"):
            e.set_option("forced_share_prompt", 1)
        e.set_option("forced_parallel", 1)
        e.set_option("forced_share_prompt", 1)
        with pytest.raises(SonicError, match="forced_share_prompt"):
            e.set_option("forced_parallel", 0)
        with pytest.raises(SonicError, match="forced_share_prompt"):
            e.set_option("forced_align", 1)
        e.set_option("forced_share_prompt", 0)
        e.set_option("forced_align", 1)
        with pytest.raises(SonicError, match="forced_share_prompt.*forced_align"):       # (the setter inside score_batch refuses: no run is started)
            e.score_batch([segs[0]], [prompts[0]] * 2, f2, fanout=2, share_prompt=True)
        e.set_option("forced_align", 0)
        other = list(prompts[0]); other[1] += 1
        with pytest.raises(SonicError, match="forced_share_prompt: sequences 2 and 3 .*different prompts"):
            e.score_batch(segs[:1] * 2, [prompts[0], prompts[0], prompts[0], other], np.concatenate([f2, f2]), fanout=2, share_prompt=True)
        ids, _, lps = e.score_batch([segs[0]], [prompts[0]] * 2, f2, fanout=2, share_prompt=True)      # every refusal left the handle usable, the option restored
        assert np.array_equal(ids[1], f2[1]) and len(lps[1]) == N
        ids, _, lps = e.score_batch(segs[:1] * 2, [prompts[0], other], f2)                              # ... and off: different prompts are the ordinary case
        assert np.array_equal(ids[1], f2[1])
    finally:
        e.close()
    for mode, why in ((MODE_INT8, "int8"), (MODE_F32, "fp32")):
        from sonicscribe_amd.engine import Engine
        h = Engine(D, 0, mode, max_batch=2, max_ctx=1024)
        try:
            h.set_option("forced_parallel", 1)
            with pytest.raises(SonicError, match="forced_share_prompt.*" + why):
                h.set_option("forced_share_prompt", 1)
        finally:
            h.close()


# ------------------------------------------------------------------------------------------ 10. ASRModel
def test_asrmodel_share_prompt():
    from sonicscribe_amd.asr import ASRModel
    wav = synth.synth_pcm(31, 80000).astype(np.float32) / 32768.0
    with pytest.raises(ValueError, match="scoring=True"):
        ASRModel.from_synthetic(D, max_batch=4, max_ctx=1024, token_logprobs=True, score_share_prompt=True)
    with pytest.raises(ValueError, match="share_prompt.*int8"):
        ASRModel.from_synthetic(D, mode="int8", max_batch=4, max_ctx=1024, token_logprobs=True, scoring=True, score_share_prompt=True)
    rng = np.random.default_rng(3)
    cands = [list(map(int, rand_ids(rng, k))) for k in (5, 9, 3, 1, 12, 7)]                # six candidates on max_batch = 4: two runs, the second padded with dummies
    m = ASRModel.from_synthetic(D, max_batch=4, max_ctx=1024, token_logprobs=True, scoring=True)
    try:
        plain = m.score(wav, cands)
        shared = m.score(wav, cands, share_prompt=True)
        for a, b in zip(plain, shared):
            d = np.abs(a.token_logprobs - b.token_logprobs).max()
            print(f"ASRModel.score share_prompt against the default, {len(a.token_ids)} tokens: max |d lp| = {d:.4f} (tol {2 * TOL_FIXTURE})")
            assert np.array_equal(a.token_ids, b.token_ids) and d <= 2 * TOL_FIXTURE
        again = m.score(wav, cands)                                                        # the option went back: the default path, the default's bits
        assert all(np.array_equal(bits(a.token_logprobs), bits(b.token_logprobs)) for a, b in zip(plain, again))
    finally:
        m.close()
    m = ASRModel.from_synthetic(D, max_batch=4, max_ctx=1024, token_logprobs=True, scoring=True, score_share_prompt=True)
    try:
        dflt = m.score(wav, cands)                                                         # the model's default: shared
        assert all(np.array_equal(bits(a.token_logprobs), bits(b.token_logprobs)) for a, b in zip(dflt, shared))
        off = m.score(wav, cands, share_prompt=False)
        assert all(np.array_equal(bits(a.token_logprobs), bits(b.token_logprobs)) for a, b in zip(off, plain))
    finally:
        m.close()
    m = ASRModel.from_synthetic(D, max_batch=4, max_ctx=1024, token_logprobs=True, scoring=True, timestamps=True)
    try:
        with pytest.raises(ValueError, match="share_prompt.*timestamps"):
            m.score(wav, cands[:2], share_prompt=True)
    finally:
        m.close()
