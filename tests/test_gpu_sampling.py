"""Temperature sampling end to end on the GPU (option sampling, sonic_set_request_sampling), on TINY with `token_logprobs` and `sampling` on:
greedy decoding unchanged, every step replayed from the raw logits against the definition (sonicscribe_amd/sampling.py), the same bits on every path, seeds,
the fallback ladder through ASRModel, refusals, memory."""
import numpy as np
import pytest

from gpu_common import SEED, flags, lp_bound, make_engine, same_bits, six
from sonicscribe_amd import sampling, spec, synth

pytestmark = pytest.mark.gpu
FIXED_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)


def make(mode=0, max_batch=8, max_ctx=1024, lp=True, samp=True):
    return make_engine(spec.TINY, mode, max_batch, max_ctx, flags((lp, "token_logprobs", 1), (samp, "sampling", 1)))


@pytest.fixture(scope="module")
def eng():
    e = make()
    yield e
    e.close()


def test_greedy_unchanged(eng):
    """temperature 0 - stated per request, or no values at all - gives the ids and log-probability bits of a handle without the option"""
    segs, prompts = six()
    budgets = [12] * 6
    off = make(samp=False)
    try:
        ids0, _, lp0 = off.transcribe_batch(segs, prompts, budgets, want_logprobs=True)
    finally:
        off.close()
    ids1, _, lp1 = eng.transcribe_batch(segs, prompts, budgets, want_logprobs=True)
    ids2, _, lp2 = eng.transcribe_batch(segs, prompts, budgets, want_logprobs=True, request_sampling=[(0.0, 9 + r) for r in range(6)])
    ids3, _, lp3 = eng.transcribe_batch(segs, prompts, budgets, want_logprobs=True, request_sampling=[None, (0.0, 1), None, None, (0.0, 2), None])
    for r in range(6):
        for ids, lp in ((ids1, lp1), (ids2, lp2), (ids3, lp3)):
            assert np.array_equal(ids[r], ids0[r]) and same_bits(lp[r], lp0[r]), r


def test_replay_against_the_definition(eng):
    """every step of sampled runs at t = 1 and t = 0.2, replayed from the dumped raw logits: the emitted id lies in {i : y64_i >= max y64 - 2 eps_g - u}, y64 the
    contract's y with exact noise, u one fp32 spacing at max |y| (the kernel's y = q + g is rounded once per candidate: half a spacing on either side of the
    compare).  Steps where that set has more than one member may be at most 2 % of the steps checked: the definition alone gives a top-two gap below 1e-2 in about
    0.5 % of draws at the full vocabulary, and the window here is some 1e-5 wide.  At least 100 steps are checked."""
    segs, prompts = six()
    budgets = [20] * 6
    checked = ambiguous = 0
    for t in (1.0, 0.2):
        seeds = [1000 + 7 * r for r in range(6)]
        ids, logits, lps = eng.transcribe_batch(segs, prompts, budgets, want_logits=True, want_logprobs=True, request_sampling=[(t, s) for s in seeds])
        for r in range(6):
            for step in range(len(ids[r])):
                raw = logits[step, r]
                y = sampling.perturbed(raw, t, seeds[r], step)
                top = y.max()
                tol = 2 * sampling.EPS_G + float(np.spacing(np.float32(np.abs(y[np.isfinite(y)]).max())))
                cand = np.flatnonzero(y >= top - tol)
                assert int(ids[r][step]) in cand, (t, r, step, int(ids[r][step]), cand.tolist(), float(top - y[int(ids[r][step])]))
                checked += 1
                ambiguous += len(cand) > 1
                # the log-probability is log_softmax of the raw scores at temperature 1, whatever t
                l = raw.astype(np.float64)
                ref = l[int(ids[r][step])] - (l.max() + np.log(np.exp(l - l.max()).sum()))
                assert abs(float(lps[r][step]) - ref) <= lp_bound(len(raw), ref), (t, r, step, float(lps[r][step]), ref)
        assert any(int(ids[r][s]) != int(np.argmax(logits[s, r])) for r in range(6) for s in range(len(ids[r]))), "a sampled run that never left the argmax"
    print(f"replay: {checked} steps checked, {ambiguous} with more than one candidate")
    assert checked >= 100 and ambiguous <= 0.02 * checked, (checked, ambiguous)


def test_invariance_all_paths(eng):
    """the same (audio, t, seed): alone; as row 5 of a batch of other requests with other seeds; through the continuous schedulers; after sonic_splice_rows"""
    from sonicscribe_amd.dispatch import Dispatcher
    segs, prompts = six()
    budgets = [5, 17, 11, 9, 13, 15]
    samp = [(0.7, 11), (1.0, 12), (0.0, 13), (0.3, 14), (1.5, 15), (1.0, 0x123456789ABCDEF0)]
    want_ids, _, want_lp = eng.transcribe_batch([segs[5]], [prompts[5]], [budgets[5]], want_logprobs=True, request_sampling=[samp[5]])      # alone
    want_ids, want_lp = want_ids[0], want_lp[0]
    greedy, _ = eng.transcribe_batch([segs[5]], [prompts[5]], [budgets[5]])
    assert not np.array_equal(greedy[0], want_ids), "t = 1 left the greedy path nowhere: the test shows nothing"
    ids_b, _, lp_b = eng.transcribe_batch(segs, prompts, budgets, want_logprobs=True, request_sampling=samp)                                 # row 5 of a batch (hipGraph loop)
    assert np.array_equal(ids_b[5], want_ids) and same_bits(lp_b[5], want_lp)
    ids_e, _, lp_e = eng.transcribe_batch(segs, prompts, budgets, want_logits=True, want_logprobs=True, request_sampling=samp)               # ... and eager
    for r in range(6):
        assert np.array_equal(ids_e[r], ids_b[r]) and same_bits(lp_e[r], lp_b[r]), r
    # prefill on a slot, then splice into a continuous handle: the words travel with the row, into another row than the one it was prefilled in
    pre = eng.slot()
    assert pre.sampling
    eng.service_begin()
    try:
        pre.stage_pcm(segs[3:]); pre.prefill(prompts[3:], budgets[3:], request_sampling=samp[3:])
        seq = eng.splice_rows(pre, [2, 0, 1], [1, 6, 4])
        rows, got = {1: 5, 6: 3, 4: 4}, {}
        for _ in range(300):
            fin, nn, s_, _ = eng.service_step(1, 8)
            done = [r for r in rows if r not in got and s_ > seq and fin[r]]
            if done:
                a, b = eng.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                for r, x, y in zip(done, a, b):
                    got[r] = (x, y)
            if len(got) == 3:
                break
        assert len(got) == 3
        for row, req in rows.items():
            assert np.array_equal(got[row][0], ids_b[req]) and same_bits(got[row][1], lp_b[req]), (row, req)
    finally:
        eng.service_end()
        pre.close()
    # the Python scheduler and the native one
    for native in (False, True):
        slots = [eng.slot(), eng.slot()]
        disp = Dispatcher([eng], slots=[slots], continuous=True, native=native)
        assert type(disp.replicas[0]).__name__ == ("_NativeContinuousReplica" if native else "_ContinuousReplica")
        futs = [disp.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True, sampling=samp[i]) for i in range(6)]
        res = [f.result(timeout=120) for f in futs]
        disp.close()
        for s in slots:
            s.close()
        for i in range(6):
            assert np.array_equal(res[i][0], ids_b[i]) and same_bits(res[i][1], lp_b[i]), (native, i)


def test_seeds_differ(eng):
    segs, prompts = six()
    runs = [eng.transcribe_batch([segs[0]], [prompts[0]], [16], request_sampling=[(1.0, s)])[0][0].tolist() for s in FIXED_SEEDS]
    again = eng.transcribe_batch([segs[0]], [prompts[0]], [16], request_sampling=[(1.0, FIXED_SEEDS[0])])[0][0].tolist()
    print(f"seeds: {len({tuple(r) for r in runs})} distinct transcripts of {len(runs)}")
    assert again == runs[0] and len({tuple(r) for r in runs}) >= 2


def test_ladder_end_to_end():
    """a threshold the greedy attempt must fail (no log-probability is above 0): every temperature is tried, the last attempt is returned"""
    from sonicscribe_amd.asr import ASRModel, Transcription
    wav = synth.synth_pcm(31, 80000).astype(np.float32) / 32768.0
    temps = (0.0, 0.4, 0.8)
    with pytest.raises(ValueError, match="token_logprobs"):
        ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, sampling=True)
    with pytest.raises(ValueError, match="sampling"):
        ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, token_logprobs=True, temperature=0.5)
    with pytest.raises(ValueError, match="bulk"):
        ASRModel.from_synthetic(spec.TINY, max_batch=32, max_ctx=1024, token_logprobs=True, sampling=True, bulk=True)
    plain = ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, token_logprobs=True)
    try:
        greedy = plain.submit(wav, max_new_tokens=12, detailed=True).result(timeout=60)
        with pytest.raises(ValueError, match="sampling"):
            plain.submit(wav, max_new_tokens=12, temperature=0.5)
        with pytest.raises(ValueError, match="sampling"):
            plain.transcribe_batch([wav], max_new_tokens=12, seed=3)
    finally:
        plain.close()
    # (from_synthetic's own `seed` is the seed of the synthetic WEIGHTS: the sampling seed goes in per call here)
    m = ASRModel.from_synthetic(spec.TINY, max_batch=4, max_ctx=1024, token_logprobs=True, sampling=True, logprob_threshold=0.0)
    try:
        r0 = m.submit(wav, max_new_tokens=12, detailed=True).result(timeout=60)                       # the defaults: one greedy attempt
        assert r0.attempts == 1 and r0.temperature == 0.0 and np.array_equal(r0.token_ids, greedy.token_ids) and same_bits(r0.token_logprobs, greedy.token_logprobs)
        r = m.submit(wav, max_new_tokens=12, detailed=True, temperature=temps, seed=5).result(timeout=120)
        assert isinstance(r, Transcription) and r.attempts == len(temps) and r.temperature == temps[-1]
        one = m.submit(wav, max_new_tokens=12, detailed=True, temperature=temps[-1], seed=5).result(timeout=60)   # the same (audio, t, seed) as the last attempt
        assert one.attempts == 1 and np.array_equal(one.token_ids, r.token_ids) and same_bits(one.token_logprobs, r.token_logprobs) and one.text == r.text
        assert m.submit(wav, max_new_tokens=12, temperature=temps, seed=5).result(timeout=120) == r.text
        assert m.transcribe_batch([wav, wav], max_new_tokens=12, temperature=temps, seed=5) == [r.text, r.text]
        assert m.transcribe_batch([wav], max_new_tokens=12, temperature=temps[-1], seed=5) == [r.text]
        info = m.transcribe(wav, max_new_tokens=12, return_debug_info=True, temperature=temps, seed=5)
        assert info["temperature"] == temps[-1] and info["compression_ratio"] == r.compression_ratio and info["transcript"] == r.text
        # a ladder whose first attempt passes stops there
        m.logprob_threshold = None
        m.compression_ratio_threshold = None
        assert m.submit(wav, max_new_tokens=12, detailed=True, temperature=temps).result(timeout=60).attempts == 1
        st = m.open_stream("s")
        pcm = synth.synth_pcm(31, 80000)
        for i in range(0, len(pcm), 1024):
            st.add_audio_chunk(pcm[i:i + 1024].tobytes())
        a = st.submit_chunks(0, st.next_chunk_id - 1, max_new_tokens=12, detailed=True, temperature=0.8).result(timeout=60)
        assert a.temperature == 0.8 and a.attempts == 1
        with pytest.raises(ValueError, match="ladder"):
            st.submit_chunks(0, st.next_chunk_id - 1, max_new_tokens=12, temperature=temps)
        st.close()
    finally:
        m.close()


def test_refusals_and_memory():
    from sonicscribe_amd.dispatch import Dispatcher
    from sonicscribe_amd.engine import Engine, SonicError
    segs, prompts = six()
    e = Engine(spec.TINY, 0, 0, max_batch=32, max_ctx=1024)
    try:
        with pytest.raises(SonicError, match="token_logprobs"):                # the option without token_logprobs, by name
            e.set_option("sampling", 1)
        e.set_option("token_logprobs", 1)
        e.load_synthetic(SEED)
        a0 = e.memory_info()[0]
        e.transcribe_batch(segs[:2], prompts[:2], [4, 4])
        assert e.memory_info()[0] == a0                                        # off is off: nothing is allocated without the option
        with pytest.raises(SonicError, match="sampling"):
            e.set_request_sampling([(0.5, 1)])
        e.stage_pcm(segs[:1]); e.prefill(prompts[:1], [8])
        with pytest.raises(SonicError, match="running"):                       # refused while work is in hand
            e.set_option("sampling", 1)
        e.decode_step(100)
        e.set_option("sampling", 1)
        a1 = e.memory_info()[0]
        print(f"sampling: sonic_memory_info grows by {a1 - a0} bytes (64 rows x 3 words)")
        assert a1 - a0 == 64 * 3 * 4
        with pytest.raises(SonicError, match="token_logprobs"):
            e.set_option("token_logprobs", 0)
        for bad in (-0.5, 5e-4, 100.5, float("nan"), float("inf")):           # an invalid temperature: Python's check, and the library's own behind it
            with pytest.raises(ValueError, match="temperature"):
                e.set_request_sampling([(bad, 1)])
            t = np.array([bad], np.float32); s = np.array([1], np.uint64)
            assert e.lib.sonic_set_request_sampling(e.h, t.ctypes.data, s.ctypes.data, 1) == 1 and b"temperature" in e.lib.sonic_last_error(e.h)
        e.set_request_sampling([(0.5, 1)])                                     # values for one request, a batch of two: refused by name, and consumed
        with pytest.raises(SonicError, match="sonic_set_request_sampling"):
            e.transcribe_batch(segs[:2], prompts[:2], [4, 4])
        g0, _ = e.transcribe_batch(segs[:2], prompts[:2], [8, 8])
        s1, _ = e.transcribe_batch(segs[:2], prompts[:2], [8, 8], request_sampling=[(1.0, 3), (1.0, 4)])
        g1, _ = e.transcribe_batch(segs[:2], prompts[:2], [8, 8])              # consumed: the next batch is greedy again
        assert all(np.array_equal(g0[r], g1[r]) for r in range(2)) and any(not np.array_equal(g0[r], s1[r]) for r in range(2))
        # a splice between handles whose options differ is refused by name, either way round
        pre = e.slot()
        assert pre.sampling
        pre.set_option("sampling", 0)
        e.service_begin()
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [4])
        with pytest.raises(SonicError, match="sampling"):
            e.splice_rows(pre, [0], [0])
        e.service_end()
        pre.decode_step(100)
        pre.set_option("sampling", 1)
        e.set_option("sampling", 0)
        e.service_begin()
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [4], request_sampling=[(0.5, 1)])
        with pytest.raises(SonicError, match="sampling"):
            e.splice_rows(pre, [0], [0])
        e.service_end()
        pre.decode_step(100)
        # schedulers over handles without the option refuse a temperature by name; the bulk pipeline refuses it whatever the handles have
        slots = [e.slot(), e.slot()]
        disp = Dispatcher([e], slots=[slots], continuous=True, native=True)
        with pytest.raises(ValueError, match="sampling"):
            disp.submit([segs[0]], prompts[0], 4, sampling=(0.5, 1))
        disp.close()
        for s in slots:
            s.close()
        pre.close()
        e.set_option("sampling", 1)
        slots = [e.slot(), e.slot()]
        bulk = Dispatcher([e], slots=[slots], bulk=True, decoders=1)
        with pytest.raises(ValueError, match="bulk"):
            bulk.submit([segs[0]], prompts[0], 4, sampling=(0.5, 1))
        bulk.close()
        for s in slots:
            s.close()
    finally:
        e.close()
