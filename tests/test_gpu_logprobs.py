"""Per-token log-probabilities (option token_logprobs; greedy_kernel<T, true>): for every emitted token the engine returns
log_softmax(l)[tok] of the logits l that step's argmax compared - HF compute_transition_scores(..., normalize_logits=True) of a greedy generate().

Accuracy is asserted against a bound DERIVED from the kernel, not measured: tests/gpu_common.py lp_bound, with its derivation (DESIGN.md 6.3 goes through the
kernel line by line).  The tests print the worst observed error / bound (a report; DESIGN.md quotes it).  Against the reference fixtures the bound is the
project's own logit tolerance (tests/test_gpu_parity.py: 4 * 2^-6) twice, because log-sum-exp is 1-Lipschitz in the sup norm: 0.125."""
import math
import os

import numpy as np
import pytest

from gpu_common import U, flags, load_golden, lp_bound, make_engine, prompt_for, ref_logprob, same_bits, slabs
from sonicscribe_amd import spec, synth

pytestmark = pytest.mark.gpu
TOL_FIXTURE = 2 * 4 * 2.0 ** -6
WORST = {}


def check_bound(tag, lp, logits, tok):
    V = logits.shape[-1]
    ref = ref_logprob(logits, tok)
    err = np.abs(np.asarray(lp, np.float64) - ref)
    ratio = float((err / lp_bound(V, ref)).max())
    WORST[tag] = max(WORST.get(tag, 0.0), ratio)
    print(f"{tag}: worst |lp - ref64| / bound = {ratio:.3f} (max err {err.max():.3e}, V = {V}, lp in [{np.min(lp):.3f}, {np.max(lp):.3f}])")
    assert np.all(np.isfinite(lp)) and ratio <= 1.0, (tag, ratio)
    return ref


def make(d=spec.TINY, mode=0, max_batch=4, max_ctx=1024, lp=True):
    return make_engine(d, mode, max_batch, max_ctx, flags((lp, "token_logprobs", 1)))


@pytest.fixture(scope="module")
def eng():
    e = make()
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    g, segs, prompts = load_golden(golden_dir)
    return g, segs, prompts, int(g["n_new"])


@pytest.fixture(scope="module")
def eager_run(eng, golden):
    """the fixture batch once through the eager loop (want_logits): ids, step logits and log-probabilities, shared by the tests below"""
    g, segs, prompts, n_new = golden
    ids, logits, lps = eng.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True, want_logprobs=True)
    return ids, logits, lps


# ------------------------------------------------------------------------------------------ 1. the kernel hook
def _rows(V, rng):
    i = np.arange(V)
    equal = np.full(V, 1.5, np.float32)
    ramp = (-3.0 + i * np.float32(60.0 / 59264)).astype(np.float32)                  # strictly ascending: every trip of every thread moves its maximum
    spike = rng.uniform(-2, 2, V).astype(np.float32); spike[int(rng.integers(0, V))] += 60.0
    far = (-3.0e4 + rng.uniform(-300, 300, V)).astype(np.float32)
    dup = rng.uniform(-2, 2, V).astype(np.float32)
    p1, p2 = 1, (300 if V > 304 else 5)                                              # threads 0 and 75 (waves 0 and 1); V = 8: threads 0 and 1
    dup[p1] = dup[p2] = 5.0
    masked = rng.uniform(-2, 2, V).astype(np.float32)                                # -inf logits: whole first trips of every thread (V > 16384), or whole
    masked[:min(16384, V // 2)] = -np.inf                                            # threads and waves; the sum must skip them, never form -inf - -inf
    return {"equal": equal, "ramp": ramp, "spike": spike, "far": far, "dup": dup, "masked": masked}, p1


@pytest.mark.parametrize("V", [8, 1024, 16388, 59264])
def test_kernel_hook_bound(eng, V):
    rng = np.random.default_rng(V)
    rows, p1 = _rows(V, rng)
    for ks in (1, 2, 3):
        for names in (("equal", "ramp", "spike"), ("far", "dup", "spike"), ("masked", "equal", "dup")):
            s = slabs([rows[n] for n in names], ks)
            tok, lg, lp = eng.test_greedy_lp(s, 3)
            tok0, lg0 = eng.test_greedy(s, 3, want_logits=True)
            assert np.array_equal(tok, tok0) and np.array_equal(lg.view(np.uint32), lg0.view(np.uint32)), (V, ks, names)
            assert np.array_equal(tok, lg.argmax(axis=1))                            # (first maximum)
            check_bound(f"hook V={V}", lp, lg, tok)
            for b, n in enumerate(names):
                if n == "equal":
                    assert abs(float(lp[b]) + math.log(V)) <= 2 * U * math.log(V), (V, ks, lp[b])     # exactly V terms of 1: -log V, rounded once
                if n == "dup":
                    assert tok[b] == p1
        # forced ids that are not the maximum: l[forced] - logsumexp, the forced logit recomputed from the slabs
        names = ("spike", "far", "dup")
        s = slabs([rows[n] for n in names], ks)
        force = ((s.sum(axis=0)[:3].argmax(axis=1) + V // 2 + 1) % V).astype(np.int32)
        tok, lg, lp = eng.test_greedy_lp(s, 3, force_ids=force)
        assert np.array_equal(tok, force) and np.all(force != lg.argmax(axis=1))
        ref = check_bound(f"hook V={V} forced", lp, lg, force)
        assert np.all(ref <= 0) and ref[0] < -50                                     # (the spike row: the forced token sits 60 below the maximum)


# ------------------------------------------------------------------------------------------ 2. end to end at TINY
def _comparable_steps(ids, ref_ids):
    """steps whose generated prefix equals the fixture's (the step after the first difference still saw the same history)"""
    n = len(ref_ids)
    same = n if np.array_equal(ids[:n], ref_ids) else int(np.argmin(ids[:n] == ref_ids))
    return min(same + 1, n)


def test_end_to_end_eager(eng, golden, eager_run):
    g, segs, prompts, n_new = golden
    ids, logits, lps = eager_run
    off = make(lp=False)
    ids_off, _ = off.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True)
    off.close()
    for si, need in ((0, 16), (1, 24)):
        assert np.array_equal(ids[si], ids_off[si])                                  # the option changes no token
        assert lps[si].dtype == np.float32 and len(lps[si]) == len(ids[si]) == n_new
        check_bound(f"tiny eager s{si}", lps[si], logits[:n_new, si], ids[si])
        ref_ids, ref_logits = g[f"s{si}_new_ids"], g[f"s{si}_step_logits"]
        assert np.array_equal(ref_ids, ref_logits.argmax(axis=1))
        n_cmp = _comparable_steps(ids[si], ref_ids)
        assert n_cmp >= need, (si, n_cmp)
        ref_lp = ref_logprob(ref_logits[:n_cmp], ids[si][:n_cmp])
        d = np.abs(lps[si][:n_cmp] - ref_lp)
        print(f"tiny s{si}: {n_cmp} comparable steps, max |lp - fixture| = {d.max():.4f} (fixture lp in [{ref_lp.min():.2f}, {ref_lp.max():.2f}])")
        assert d.max() <= TOL_FIXTURE


# ------------------------------------------------------------------------------------------ 3. the hipGraph loop
def test_graph_loop_same_bits(eng, golden, eager_run):
    g, segs, prompts, n_new = golden
    ids, _, lps = eager_run
    ids_g, logits_g, lps_g = eng.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)
    assert logits_g is None
    assert eng.timings()["host_decode_launches"] < n_new - 1                         # chunks of captured steps, not one launch per token
    for si in range(2):
        assert np.array_equal(ids_g[si], ids[si])
        assert np.array_equal(lps_g[si].view(np.uint32), lps[si].view(np.uint32))


# ------------------------------------------------------------------------------------------ 4. teacher forcing
def test_teacher_forcing(eng, golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_forced_bf16.npz"))
    segs = [synth.synth_pcm(int(g[f"s{i}_seg_index"]), int(g[f"s{i}_n_samples"])) for i in range(2)]
    prompts = [g[f"s{i}_prompt_ids"] for i in range(2)]
    force = np.stack([g[f"s{i}_force_ids"] for i in range(2)]).astype(np.int32)
    n = force.shape[1]
    eng.set_forced_ids(force)
    try:
        ids, logits, lps = eng.transcribe_batch(segs, prompts, [n, n], want_logits=True, want_logprobs=True)
    finally:
        eng.set_forced_ids(None)
    for si in range(2):
        assert np.array_equal(ids[si], force[si])
        assert not np.array_equal(force[si], logits[:n, si].argmax(axis=1))          # the forced ids are not the argmax: the two readings differ
        check_bound(f"tiny forced s{si}", lps[si], logits[:n, si], force[si])
        ref_lp = ref_logprob(g[f"s{si}_step_logits"], force[si])
        d = np.abs(lps[si] - ref_lp)
        print(f"tiny forced s{si}: max |lp - fixture| = {d.max():.4f} (fixture lp in [{ref_lp.min():.2f}, {ref_lp.max():.2f}])")
        assert d.max() <= TOL_FIXTURE


# ------------------------------------------------------------------------------------------ 5. invariance, bit for bit
def test_invariance_engine_paths(eng):
    d = spec.TINY
    segs = [synth.synth_pcm(700 + i, n) for i, n in enumerate((48000, 200000, 80000))]
    prompts = [prompt_for(d, len(s)) for s in segs]
    budgets = [5, 17, 11]
    ids1, _, lp1 = eng.transcribe_batch([segs[2]], [prompts[2]], [budgets[2]], want_logprobs=True)                # alone
    ids3, _, lp3 = eng.transcribe_batch(segs, prompts, budgets, want_logprobs=True)                                # row 2 of 3, unequal budgets
    assert np.array_equal(ids1[0], ids3[2]) and same_bits(lp1[0], lp3[2])
    for r in range(3):
        assert len(lp3[r]) == len(ids3[r]) == budgets[r] and np.all(np.isfinite(lp3[r]))
    # entries at or beyond a row's n_new are not written on the host
    buf = np.full((3, 20), np.nan, np.float32)
    eng._check(eng.lib.sonic_fetch_logprobs(eng.h, buf.ctypes.data, 20))
    for r in range(3):
        assert same_bits(buf[r, :budgets[r]].copy(), lp3[r]) and np.all(np.isnan(buf[r, budgets[r]:]))
    ids_f, lp_f = eng.fetch_tokens(3, 20, want_logprobs=True)
    assert all(np.array_equal(ids_f[r], ids3[r]) and same_bits(lp_f[r], lp3[r]) for r in range(3))
    # spliced into a continuous loop: the first token's entry comes from the prefill handle
    pre = eng.slot()
    eng.service_begin()
    try:
        pre.stage_pcm([segs[0], segs[2]]); pre.prefill([prompts[0], prompts[2]], [budgets[0], budgets[2]])
        seq = eng.splice_rows(pre, [1, 0], [3, 1])
        got = {}
        rows = {3: 2, 1: 0}
        for _ in range(200):
            fin, nn, s_, _ = eng.service_step(1, 4)
            done = [r for r in rows if r not in got and s_ > seq and fin[r]]
            if done:
                a, b = eng.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                for r, x, y in zip(done, a, b):
                    got[r] = (x, y)
            if len(got) == 2:
                break
        assert len(got) == 2
        for row, req in rows.items():
            assert np.array_equal(got[row][0], ids3[req]) and same_bits(got[row][1], lp3[req]), (row, req)
    finally:
        eng.service_end()
        pre.close()


# ------------------------------------------------------------------------------------------ 6. modes
@pytest.mark.parametrize("mode", [1, 2, 3], ids=["int8", "f16", "f32"])
def test_modes_bound(mode, golden):
    g, segs, prompts, n_new = golden
    e = make(mode=mode)
    try:
        ids, logits, lps = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True, want_logprobs=True)
        for si in range(2):
            assert len(lps[si]) == len(ids[si]) == n_new
            assert np.array_equal(ids[si], logits[:n_new, si].argmax(axis=1))
            check_bound(f"tiny mode {mode} s{si}", lps[si], logits[:n_new, si], ids[si])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 7. surface
def test_option_off_refuses(golden):
    from sonicscribe_amd.engine import SonicError
    g, segs, prompts, n_new = golden
    off = make(lp=False, max_batch=16)
    on = make(max_batch=16)
    try:
        a0 = off.memory_info()[0]
        assert on.memory_info()[0] > a0                                              # the buffer is counted
        off.transcribe_batch(segs[:1], prompts[:1], [4])
        with pytest.raises(SonicError, match="token_logprobs"):
            off.transcribe_batch(segs[:1], prompts[:1], [4], want_logprobs=True)
        with pytest.raises(SonicError, match="token_logprobs"):
            off.fetch_tokens(1, 4, want_logprobs=True)
        # a splice from an option-off source into an option-on loop is refused; fetch_rows_lp on an option-off loop too
        off.stage_pcm(segs[:1]); off.prefill(prompts[:1], [4])
        on.service_begin()
        with pytest.raises(SonicError):
            on.splice_rows(off, [0], [0])                                            # (not one weight copy either: refused before anything is queued)
        on.service_end()
        slot_off = off.slot()
        off.service_begin()
        slot_off.stage_pcm(segs[:1]); slot_off.prefill(prompts[:1], [4])
        seq = off.splice_rows(slot_off, [0], [0])
        for _ in range(100):
            fin, nn, s_, _ = off.service_step(1, 1)
            if s_ > seq and fin[0]:
                break
        with pytest.raises(SonicError, match="token_logprobs"):
            off.fetch_rows([0], [int(nn[0])], want_logprobs=True)
        assert len(off.fetch_rows([0], [int(nn[0])])[0]) == 4
        off.service_end()
        # same weights, option switched on for the loop only: the slot prefilled without it
        off.set_option("token_logprobs", 1)
        off.service_begin()
        slot_off.stage_pcm(segs[:1]); slot_off.prefill(prompts[:1], [4])
        with pytest.raises(SonicError, match="token_logprobs"):
            off.splice_rows(slot_off, [0], [0])
        off.service_end()
        slot_off.close()
    finally:
        off.close(); on.close()


def test_invariance_native_dispatcher_and_bulk_pipeline():
    """the same request through csrc/dispatch.cpp (rows join a running loop) and through csrc/pipeline.cpp (blocks of a bulk batch): the bits of its solo run"""
    from sonicscribe_amd.dispatch import Dispatcher
    d = spec.TINY
    segs = [synth.synth_pcm(700 + i, n) for i, n in enumerate((48000, 200000, 80000))]
    prompts = [prompt_for(d, len(s)) for s in segs]
    budgets = [5, 17, 11]
    e = make(max_batch=32)
    try:
        solo = [e.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]], want_logprobs=True) for i in range(3)]
        slots = [e.slot(), e.slot()]
        assert all(s.token_logprobs for s in slots)
        disp = Dispatcher([e], slots=[slots], continuous=True)
        assert type(disp.replicas[0]).__name__ == "_NativeContinuousReplica" and disp.replicas[0].lp
        futs = [disp.submit([segs[i]], prompts[i], budgets[i], want_logprobs=(i != 1)) for i in range(3)]
        res = [f.result(timeout=60) for f in futs]
        disp.close()
        for i in (0, 2):
            assert np.array_equal(res[i][0], solo[i][0][0]) and same_bits(res[i][1], solo[i][2][0]), i
        assert isinstance(res[1], np.ndarray) and np.array_equal(res[1], solo[1][0][0])
        bulk = Dispatcher([e], slots=[slots], bulk=True, decoders=1)
        futs = [bulk.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True) for i in range(3)]
        res = [f.result(timeout=60) for f in futs]
        plain = bulk.submit([segs[2]], prompts[2], budgets[2]).result(timeout=60)
        bulk.close()
        for i in range(3):
            assert np.array_equal(res[i][0], solo[i][0][0]) and same_bits(res[i][1], solo[i][2][0]), i
        assert np.array_equal(plain, solo[2][0][0])
    finally:
        e.close()
    # handles without the option: the dispatcher refuses the request, the pipeline the submission
    off = make(lp=False, max_batch=32)
    try:
        slots = [off.slot(), off.slot()]
        disp = Dispatcher([off], slots=[slots], continuous=True)
        with pytest.raises(ValueError, match="token_logprobs"):
            disp.submit([segs[0]], prompts[0], 4, want_logprobs=True)
        assert len(disp.submit([segs[0]], prompts[0], 4).result(timeout=60)) == 4
        # the library's own refusal (the Python check above fires before it is reached): SONIC_ERR_INVALID, no ticket, the message names the option
        import ctypes as C
        rep = disp.replicas[0]
        t, st, n = C.c_int64(7), C.c_int32(0), C.c_int32(0)
        ids_b, lp_b, err = np.zeros(16, np.int32), np.zeros(16, np.float32), C.create_string_buffer(512)
        rc = rep.lib.sonic_dispatch_next_lp(rep.h, 0, C.byref(t), C.byref(st), ids_b.ctypes.data_as(C.c_void_p), 16, C.byref(n), err, 512,
                                            lp_b.ctypes.data_as(C.c_void_p))
        assert rc == 1 and t.value == 0 and "token_logprobs" in err.value.decode()      # 1 = SONIC_ERR_INVALID
        disp.close()
        from sonicscribe_amd.pipeline import NativePipeline
        pipe = NativePipeline([off], slots, 32)
        with pytest.raises(RuntimeError, match="token_logprobs"):
            pipe.submit([prompts[0]], [4], segments=[segs[0]], req_win=[0, 1], want_logprobs=True)
        pipe.close()
    finally:
        off.close()


def test_asrmodel_surface():
    from sonicscribe_amd.asr import ASRModel, Transcription
    wav = synth.synth_pcm(31, 80000).astype(np.float32) / 32768.0
    plain = ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024)
    try:
        info0 = plain.transcribe(wav, max_new_tokens=12, return_debug_info=True)
        assert sorted(info0) == sorted(["transcript", "processing_time", "audio_length_sec", "mode", "device", "gpu_memory_allocated_mb", "gpu_memory_reserved_mb"])
        with pytest.raises(ValueError, match="token_logprobs"):
            plain.submit(wav, max_new_tokens=12, detailed=True)
    finally:
        plain.close()
    m = ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, token_logprobs=True)
    try:
        info = m.transcribe(wav, max_new_tokens=12, return_debug_info=True)
        assert sorted(info) == sorted(list(info0) + ["token_ids", "token_logprobs", "avg_logprob", "confidence"])
        assert info["transcript"] == info0["transcript"]
        assert info["token_logprobs"].dtype == np.float32 and len(info["token_logprobs"]) == len(info["token_ids"]) >= 1
        assert np.all(info["token_logprobs"] <= 0) and info["avg_logprob"] == pytest.approx(float(np.mean(info["token_logprobs"], dtype=np.float64)))
        assert info["confidence"] == math.exp(info["avg_logprob"]) and 0 < info["confidence"] <= 1
        r = m.submit(wav, max_new_tokens=12, detailed=True).result(timeout=60)
        assert isinstance(r, Transcription) and r.text == info["transcript"] and same_bits(r.token_logprobs, info["token_logprobs"])
        assert m.submit(wav, max_new_tokens=12).result(timeout=60) == info["transcript"]
        st = m.open_stream("s")
        pcm = synth.synth_pcm(31, 80000)
        for i in range(0, len(pcm), 1024):
            st.add_audio_chunk(pcm[i:i + 1024].tobytes())
        a = st.submit_chunks(0, st.next_chunk_id - 1, max_new_tokens=12, detailed=True).result(timeout=60)
        b = st.submit_chunks(0, st.next_chunk_id - 1, max_new_tokens=12).result(timeout=60)
        assert isinstance(a, Transcription) and a.text == b and len(a.token_logprobs) == len(a.token_ids) and np.isfinite(a.avg_logprob)
        st.close()
    finally:
        m.close()
