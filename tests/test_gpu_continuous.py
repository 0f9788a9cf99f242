"""Continuous decoding (include/sonic_hip.h sonic_service_* / sonic_splice_rows; dispatch._ContinuousReplica): requests join and leave a running
greedy loop ROW BY ROW.  The reference awaits one transcribe() per connection at a time (backend/connection_manager.py:127-245); a batch
engine pads every batch to its slowest row.  What must hold: whatever rows a request is spliced into, whoever else is decoding, however
often the row was used before - its tokens are those of its solo run (HF generate(do_sample=False) semantics, restated by the engine's own
batch path, which tests/test_gpu_parity.py / test_gpu_benchsize.py pin against the oracle and the reference fixtures)."""
from dataclasses import replace

import numpy as np
import pytest

from gpu_common import make_engine, prompt_for
from sonicscribe_amd import spec, synth

pytestmark = pytest.mark.gpu


def make(d, max_batch, mode=0, max_ctx=512):
    return make_engine(d, mode, max_batch, max_ctx)


def drain(dec, rows, limit=2000):
    """step the decoding handle until every row in `rows` (row -> valid_after) is finished; returns {row: ids}.  Only as many rows as are
    occupied are stepped (rounded up to 16 by the engine): the graphs for 16 / 32 / 48 rows must give the same bits"""
    out = {}
    for _ in range(limit):
        fin, nn, seq, _ = dec.service_step(1, max(rows) + 1)
        for r, va in list(rows.items()):
            if seq > va and fin[r]:
                out[r] = dec.fetch_row(r, int(nn[r]))
                del rows[r]
        if not rows:
            return out
    raise AssertionError("rows did not finish")


FULLW = replace(spec.FULL, enc_layers=2, dec_layers=2, eos_ids=())


@pytest.mark.parametrize("dims,mode", [(replace(spec.TINY, eos_ids=()), 0), (FULLW, 0), (replace(spec.TINY, eos_ids=()), 1)], ids=["tiny", "fullwidth", "tiny-int8"])
def test_spliced_rows_equal_solo_runs(dims, mode):
    dec = make(dims, 48, mode)
    pre = dec.slot()
    segs = [synth.synth_pcm(500 + i, 16000 * (2 + (i * 5) % 9)) for i in range(10)]
    prompts = [prompt_for(dims, len(s)) for s in segs]
    budgets = [9, 40, 15, 3, 27, 1, 15, 33, 8, 21]
    solo = [dec.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]])[0][0] for i in range(10)]      # the batch path, one request at a time
    dec.service_begin()
    with pytest.raises(RuntimeError):
        dec.transcribe_batch([segs[0]], [prompts[0]], [4])               # a continuously decoding handle takes no batch calls
    # wave 1: four requests prefilled together, spliced into scattered rows
    pre.stage_pcm(segs[:4]); pre.prefill(prompts[:4], budgets[:4])
    seq = dec.splice_rows(pre, [0, 1, 2, 3], [5, 0, 37, 9])
    rows = {5: seq, 0: seq, 37: seq, 9: seq}
    who = {5: 0, 0: 1, 37: 2, 9: 3}
    got = {}
    # let them run a little, then wave 2 joins the running loop (the slot prefills while the rows decode)
    for _ in range(2):
        fin, nn, s_, _ = dec.service_step(1, 38)
    pre.stage_pcm(segs[4:7]); pre.prefill(prompts[4:7], budgets[4:7])
    seq2 = dec.splice_rows(pre, [0, 1, 2], [1, 2, 3])
    rows.update({1: seq2, 2: seq2, 3: seq2}); who.update({1: 4, 2: 5, 3: 6})
    for r, ids in drain(dec, rows).items():
        got[who[r]] = ids
    # wave 3 reuses rows that were fetched (5 held request 0 before) while nothing else runs
    pre.stage_pcm(segs[7:]); pre.prefill(prompts[7:], budgets[7:])
    seq3 = dec.splice_rows(pre, [0, 1, 2], [5, 9, 0])
    who3 = {5: 7, 9: 8, 0: 9}
    for r, ids in drain(dec, {5: seq3, 9: seq3, 0: seq3}).items():
        got[who3[r]] = ids
    for i in range(10):
        assert len(got[i]) == budgets[i] and np.array_equal(got[i], solo[i]), i
    dec.service_end()
    again, _ = dec.transcribe_batch([segs[2]], [prompts[2]], [budgets[2]])   # and the handle is a batch engine again
    assert np.array_equal(again[0], solo[2])
    dec.close()


def test_one_prefill_feeds_two_decoders_and_running_rows_cannot_be_fetched():
    """Rows of ONE prefill go to two decoding handles; the slot's next prefill must wait for BOTH copies (each decoder has its own splice event).
    And sonic_fetch_row refuses a row the newest check saw running."""
    dims = replace(spec.TINY, eos_ids=())
    dec = make(dims, 32)
    dec2, pre = dec.slot(), dec.slot()
    segs = [synth.synth_pcm(700 + i, 16000 * (3 + i % 4)) for i in range(8)]
    prompts = [prompt_for(dims, len(s)) for s in segs]
    budgets = [30, 12, 25, 18, 22, 9, 28, 14]
    solo = [dec.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]])[0][0] for i in range(8)]
    dec.service_begin(); dec2.service_begin()
    got = {}
    pre.stage_pcm(segs[:4]); pre.prefill(prompts[:4], budgets[:4], wait=False)
    sa = dec.splice_rows(pre, [0, 1], [3, 4])
    sb = dec2.splice_rows(pre, [2, 3], [0, 20])
    pre.stage_pcm(segs[4:]); pre.prefill(prompts[4:], budgets[4:], wait=False)         # overwrites the slot's rows: only behind both splices
    fin, nn, seq, n_act = dec.service_step(1, 5)
    while seq <= sa:
        fin, nn, seq, n_act = dec.service_step(1, 5)
    if not fin[3]:
        with pytest.raises(RuntimeError):
            dec.fetch_row(3, 1)
    sc = dec.splice_rows(pre, [0, 1], [10, 11])
    sd = dec2.splice_rows(pre, [2, 3], [1, 2])
    for r, ids in drain(dec, {3: sa, 4: sa, 10: sc, 11: sc}).items():
        got[{3: 0, 4: 1, 10: 4, 11: 5}[r]] = ids
    # the second decoder's four rows leave through ONE call (sonic_fetch_rows) once all of them are finished
    want_rows = {0: sb, 20: sb, 1: sd, 2: sd}
    for _ in range(2000):
        fin, nn, seq, _ = dec2.service_step(1, 21)
        if all(seq > va and fin[r] for r, va in want_rows.items()):
            break
    else:
        raise AssertionError("rows did not finish")
    order = [20, 0, 2, 1]
    with pytest.raises(RuntimeError):
        dec2.fetch_rows([0, 0], [1, 1])                                                # a row named twice
    for r, ids in zip(order, dec2.fetch_rows(order, [int(nn[r]) for r in order])):
        got[{0: 2, 20: 3, 1: 6, 2: 7}[r]] = ids
    for i in range(8):
        assert np.array_equal(got[i], solo[i]), i
    dec.service_end(); dec2.service_end()
    dec.close()


def test_rows_that_stop_at_eos_are_refilled():
    """rows that hit EOS early hand their slot to queued requests while the long rows keep decoding; refilled rows are
    bit-identical to solo runs (an engineered EOS set, as tests/test_gpu_benchsize.py::test_eos_stop_vs_oracle does)."""
    base = replace(spec.TINY, eos_ids=())
    probe = make(base, 4)
    segs = [synth.synth_pcm(700 + i, 16000 * (2 + i % 5)) for i in range(12)]
    prompts = [prompt_for(base, len(s)) for s in segs]
    free_run = [probe.transcribe_batch([segs[i]], [prompts[i]], [60])[0][0] for i in range(12)]
    probe.close()
    # an id becomes EOS if that makes the stops ragged: some requests end early at it, others never emit it (random-weight trajectories
    # repeat themselves, so the id is searched for instead of guessed); budgets are ragged on top
    def stops(c):
        return [int(np.argmax(t == c)) + 1 if (t == c).any() else 60 for t in free_run]
    cands = sorted({int(x) for t in free_run for x in t}, key=lambda c: -len(set(stops(c))))
    best = next((c for c in cands if min(stops(c)) < 30 and max(stops(c)) >= 30), cands[0])
    d2 = replace(spec.TINY, eos_ids=(best, 991, 992))
    budgets = [12 + (i * 17) % 47 for i in range(12)]
    dec = make(d2, 4)
    pre = dec.slot()
    solo = [dec.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]])[0][0] for i in range(12)]
    assert len({len(x) for x in solo}) > 3                                               # ragged: rows leave at different steps
    n_eos_stops = sum(1 for x, b in zip(solo, budgets) if len(x) < b)
    dec.service_begin()
    pending = list(range(12))
    occupied, got = {}, {}
    free = [0, 1, 2, 3]
    while pending or occupied:
        if pending and free:                                                              # refill every free row at once
            take = pending[:len(free)]; pending = pending[len(take):]
            pre.stage_pcm([segs[i] for i in take]); pre.prefill([prompts[i] for i in take], [budgets[i] for i in take])
            dst = [free.pop(0) for _ in take]
            seq = dec.splice_rows(pre, list(range(len(take))), dst)
            for i, r in zip(take, dst):
                occupied[r] = (i, seq)
        fin, nn, s_, _ = dec.service_step(1)
        for r, (i, va) in list(occupied.items()):
            if s_ > va and fin[r]:
                got[i] = dec.fetch_row(r, int(nn[r])); del occupied[r]; free.append(r)
    for i in range(12):
        assert np.array_equal(got[i], solo[i]), (i, got[i], solo[i])
    print(f"refill test: {n_eos_stops} of 12 requests stopped at the EOS id {best}, lengths {[len(x) for x in solo]}")
    dec.close()


@pytest.mark.parametrize("native", [True, False], ids=["native-dispatch", "python-dispatch"])
def test_asrmodel_continuous_equals_batch_model(native):
    """the façade with continuous=True: mixed partial / final budgets from many sessions, host tensors and device rings; every transcript
    equals the batch-by-batch model's.  native: the scheduler inside the library (csrc/dispatch.cpp, the default) / the Python class it restates"""
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.dispatch import _ContinuousReplica, _NativeContinuousReplica
    d = replace(spec.TINY, eos_ids=())
    ref = ASRModel.from_synthetic(d, device="cuda:0", max_batch=8, max_ctx=512, slots=1)
    con = ASRModel.from_synthetic(d, device="cuda:0", max_batch=8, max_ctx=512, slots=2, continuous=True, native_dispatch=native)
    assert isinstance(con._dispatcher.replicas[0], _NativeContinuousReplica if native else _ContinuousReplica)
    assert con.get_model_info()["continuous"] is True and con.model.weight_bytes() == ref.model.weight_bytes()
    wavs = [synth.synth_pcm(900 + i, 16000 * (2 + i % 4)).astype(np.float32) / 32768.0 for i in range(30)]
    budgets = [15 if i % 3 else 60 for i in range(30)]
    want = [ref.transcribe(w[None], 16000, max_new_tokens=b) for w, b in zip(wavs, budgets)]
    futs = [con.submit(w[None], 16000, b, session=f"c{i}") for i, (w, b) in enumerate(zip(wavs, budgets))]
    assert [f.result(timeout=120) for f in futs] == want
    assert con.transcribe(wavs[0][None], 16000, max_new_tokens=60) == want[0]
    assert con.transcribe_batch(wavs[:5], max_new_tokens=[20] * 5) == ref.transcribe_batch(wavs[:5], max_new_tokens=[20] * 5)
    long = synth.synth_pcm(77, 16000 * 36).astype(np.float32) / 32768.0                    # two windows behind one prompt
    assert con.transcribe(long[None], 16000, max_new_tokens=12) == ref.transcribe(long[None], 16000, max_new_tokens=12)
    st = con.open_stream("ring-0")
    wire = np.clip(np.rint(wavs[3] * 32768.0), -32768, 32767).astype(np.int16)
    wire = wire[:(len(wire) // 1024) * 1024].tobytes()
    for j in range(0, len(wire), 2048):
        st.add_audio_chunk(wire[j:j + 2048])
    got = st.submit_chunks(0, st.next_chunk_id - 1, 30).result(timeout=60)
    assert got == ref.transcribe((np.frombuffer(wire, np.int16).astype(np.float32) / np.float32(32768.0))[None], 16000, max_new_tokens=30)
    st.close()
    # a request that cannot be decoded (prompt + budget beyond max_ctx) fails alone; one with a bad placeholder count raises ValueError as everywhere
    with pytest.raises(Exception):
        con.submit(wavs[0][None], 16000, 2000).result(timeout=60)
    assert con.submit(wavs[1][None], 16000, budgets[1]).result(timeout=60) == want[1]
    rep = con._dispatcher.replicas[0]
    assert rep.load() == 0 and rep.free_rows == 8 and rep.batches > 0 and rep.steps > 0
    ref.close(); con.close()
    with pytest.raises(RuntimeError):
        con.submit(wavs[1][None], 16000, 4)


@pytest.mark.parametrize("native", [True, False], ids=["native-dispatch", "python-dispatch"])
def test_asrmodel_two_decoders_of_64_rows_bulk_shape(native):
    """the bulk shape of the facade (bench.py's pipeline through dispatch._ContinuousReplica): two decoding handles over 64 rows each + one prefill
    slot on one weight copy; 150 requests of mixed length and budget from the caller's threads, every transcript equal to the one-slot batch model's"""
    from sonicscribe_amd.asr import ASRModel
    d = replace(spec.TINY, eos_ids=())
    ref = ASRModel.from_synthetic(d, device="cuda:0", max_batch=8, max_ctx=512, slots=1, continuous=False)
    bulk = ASRModel.from_synthetic(d, device="cuda:0", max_batch=64, max_ctx=512, slots=3, continuous=True, decoders=2, native_dispatch=native)
    info = bulk.get_model_info()
    assert info["continuous"] is True and info["slots_per_replica"] == 3 and bulk.model.slot_count() == 3
    rep = bulk._dispatcher.replicas[0]
    assert len(rep.decoders) == 2 and len(rep.prefill_engines) == 1
    wavs = [synth.synth_pcm(1200 + i, 16000 * (1 + i % 5)).astype(np.float32) / 32768.0 for i in range(50)]
    budgets = [8 + (i * 11) % 40 for i in range(50)]
    want = [ref.transcribe(w[None], 16000, max_new_tokens=b) for w, b in zip(wavs, budgets)]
    futs = [bulk.submit(wavs[i % 50][None], 16000, budgets[i % 50]) for i in range(150)]
    got = [f.result(timeout=300) for f in futs]
    assert got == [want[i % 50] for i in range(150)]
    assert rep.load() == 0 and rep.free_rows == 128 and (native or all(r is None for rows in rep.rows for r in rows))
    ref.close(); bulk.close()


def test_asrmodel_bulk_mode_runs_on_the_native_pipeline():
    """ASRModel(bulk=True): the facade's file mode behind the LIBRARY's pipeline (dispatch._BulkReplica -> pipeline.NativePipeline -> csrc/pipeline.cpp):
    three decoding handles over 64 rows + one prefill slot on one weight copy; 200 requests of mixed length and budget (two step classes, a
    two-window request, a bad one) from the caller's thread - every transcript equal to the one-slot batch model's, the bad request fails alone."""
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.dispatch import _BulkReplica
    d = replace(spec.TINY, eos_ids=())
    ref = ASRModel.from_synthetic(d, device="cuda:0", max_batch=8, max_ctx=1024, slots=1, continuous=False)
    bulk = ASRModel.from_synthetic(d, device="cuda:0", max_batch=64, max_ctx=1024, slots=4, decoders=3, bulk=True)
    rep = bulk._dispatcher.replicas[0]
    assert isinstance(rep, _BulkReplica) and len(rep.pipe.decoders) == 3 and len(rep.pipe.prefills) == 1 and bulk.get_model_info()["continuous"] is True
    wavs = [synth.synth_pcm(1500 + i, 16000 * (1 + i % 5)).astype(np.float32) / 32768.0 for i in range(50)]
    wavs[7] = synth.synth_pcm(1507, 16000 * 34).astype(np.float32) / 32768.0                  # 34 s: two 30 s windows in one request
    budgets = [(8 + (i * 11) % 8) if i % 3 == 0 else (20 + (i * 7) % 40) for i in range(50)]   # step classes <= 16 and <= 64
    want = [ref.transcribe(w[None], 16000, max_new_tokens=b) for w, b in zip(wavs, budgets)]
    futs = [bulk.submit(wavs[i % 50][None], 16000, budgets[i % 50]) for i in range(200)]
    got = [f.result(timeout=300) for f in futs]
    assert got == [want[i % 50] for i in range(200)]
    st = rep.pipe.stats()
    assert st["batches"] >= 200 // 32 and rep.load() == 0
    with pytest.raises(Exception):
        bulk.submit(wavs[0][None], 16000, 2000).result(timeout=60)                            # prompt + budget beyond max_ctx: fails alone ...
    assert bulk.submit(wavs[1][None], 16000, budgets[1]).result(timeout=60) == want[1]        # ... and the pipeline goes on
    ref.close(); bulk.close()


@pytest.mark.parametrize("dims", [replace(spec.TINY, eos_ids=()), FULLW], ids=["tiny", "fullwidth"])
def test_back_to_back_enqueued_prefills_keep_their_own_plans(dims):
    """sonic_prefill_enqueue returns with the prompt plan's host-to-device copies still queued behind the encoder; a second enqueue on
    the same handle used to overwrite the one pinned staging buffer before the first batch's copies had run - batch N prefilled with batch
    N+1's token sources, positions, lengths and budgets.  Two enqueues on the SAME staged PCM (no stage_pcm in between, which would
    synchronise) with different prompts and budgets must each give their solo tokens; a third reuses the first staging buffer."""
    dec = make(dims, 32)
    pre = dec.slot()
    segs = [synth.synth_pcm(900 + i, 16000 * (4 + 3 * i)) for i in range(4)]
    base = [prompt_for(dims, len(s)) for s in segs]
    variants = [[p + [40 + 7 * v + i, 50 + v] * (v + 1) for i, p in enumerate(base)] for v in range(3)]     # different text tails => other lengths, positions, ids
    budgets = [[5 + 3 * i + 11 * v for i in range(4)] for v in range(3)]
    solo = [[dec.transcribe_batch([segs[i]], [variants[v][i]], [budgets[v][i]])[0][0] for i in range(4)] for v in range(3)]
    dec.service_begin()
    pre.stage_pcm(segs)
    rows, who = {}, {}
    for v in range(3):
        pre.prefill(variants[v], budgets[v], wait=False)                 # queued only: the host is back before the encoder has run
        seq = dec.splice_rows(pre, [0, 1, 2, 3], [8 * v + i for i in range(4)])
        for i in range(4):
            rows[8 * v + i] = seq; who[8 * v + i] = (v, i)
    for r, ids in drain(dec, rows).items():
        v, i = who[r]
        assert len(ids) == budgets[v][i] and np.array_equal(ids, solo[v][i]), (v, i)
    dec.service_end()
    dec.close()


def test_native_dispatcher_failure_cancel_and_close_paths():
    """csrc/dispatch.cpp beyond the happy path: a queued request can be cancelled (its future is cancelled, the library drops it before it reaches a
    handle); close() fails what is still queued and completes what is running; a device error raised inside a decode loop (the error word a fused
    kernel sets when it gives up on an in-kernel wait, injected here) fails every request in flight and queued with the engine's message, and
    later submits are refused - nothing hangs.  Call sites: connection_manager.py:127-245 (a session that goes away), main.py:84-86 (model release)."""
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.dispatch import _NativeContinuousReplica
    d = replace(spec.TINY, eos_ids=())
    m = ASRModel.from_synthetic(d, device="cuda:0", max_batch=4, max_ctx=512, slots=2, continuous=True)
    rep = m._dispatcher.replicas[0]
    assert isinstance(rep, _NativeContinuousReplica)
    wav = synth.synth_pcm(5, 16000 * 3).astype(np.float32) / 32768.0
    want = m.transcribe(wav[None], 16000, max_new_tokens=40)
    # 12 long requests on a 4-row pool: the last ones are still queued when they are cancelled
    futs = [m.submit(wav[None], 16000, 200) for _ in range(12)]
    cancelled = [f for f in futs[6:] if f.cancel()]
    assert len(cancelled) >= 1
    for f in futs:
        if f not in cancelled:
            assert isinstance(f.result(timeout=120), str)
    assert m.transcribe(wav[None], 16000, max_new_tokens=40) == want          # the dispatcher goes on
    # device error inside the loop
    running = [m.submit(wav[None], 16000, 300) for _ in range(6)]
    m.model.set_option("inject_dev_err", 1)
    errs = 0
    for f in running:
        try:
            f.result(timeout=120)
        except Exception as ex:
            errs += 1
            assert "in-kernel wait" in str(ex) or "failed" in str(ex) or "closed" in str(ex), ex
    assert errs >= 1
    with pytest.raises(Exception):
        m.submit(wav[None], 16000, 4).result(timeout=60)
    m.model.set_option("inject_dev_err", 0)
    m.close()
    # close() with work queued: everything resolves
    m2 = ASRModel.from_synthetic(d, device="cuda:0", max_batch=4, max_ctx=512, slots=2, continuous=True)
    futs = [m2.submit(wav[None], 16000, 150) for _ in range(16)]
    m2.close()
    n_ok = 0
    for f in futs:
        assert f.done()
        if f.exception() is None:
            n_ok += 1
        else:
            assert "closed" in str(f.exception())
    assert 1 <= n_ok <= 16


@pytest.mark.parametrize("native", [True, False], ids=["native-dispatch", "python-dispatch"])
def test_mixed_per_request_values_in_one_prefill(native):
    """Six requests that each bring another kind of value of their own - a bias table that binds, a temperature with a seed, a grammar, a draft, a table plus a
    temperature, nothing - prefilled TOGETHER: row i of the prefill must get request i's values and nobody else's.  Each result is its solo run's on the same
    engine, ids and log-probability bits (rows are independent).  The mix is forced, not hoped for: one prefill slot, and a plug request of max_batch
    windows is prefilling while the six are submitted; a run in which every request was prefilled alone fails."""
    from sonicscribe_amd.dispatch import Dispatcher
    from sonicscribe_amd.grammar import CompiledGrammar
    from sonicscribe_amd.reqbias import RequestBias
    from test_gpu_draft import _same, make as make_with_options
    from test_gpu_grammar import grammar_a
    d = spec.TINY
    e = make_with_options(max_batch=8, opts=(("request_bias", 1), ("sampling", 1), ("grammar", 1)))      # + token_logprobs and draft_verify
    try:
        segs = [synth.synth_pcm(700 + i, n) for i, n in enumerate((48000, 80000, 64000, 96000, 56000, 72000))]
        prompts = [prompt_for(d, len(s)) for s in segs]
        budgets = [9, 12, 11, 14, 10, 7]
        plain = [e.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]])[0][0] for i in range(6)]
        gram = CompiledGrammar(grammar_a(), [e])
        table = lambda i: RequestBias([[[int(plain[i][0]), 210], 1000.0], [[210, 211], 1000.0]])      # binds behind the request's first id
        own = [dict(bias=table(0)), dict(sampling=(0.7, 1234)), dict(grammar=gram), dict(draft=[int(t) for t in plain[3][:6]]), dict(bias=table(4), sampling=(0.7, 99)), {}]
        keyword = {"bias": "request_bias", "sampling": "request_sampling", "grammar": "request_grammar", "draft": "request_draft"}
        solo = []
        for i in range(6):
            kw = {keyword[k]: [v.on(e) if k == "grammar" else v] for k, v in own[i].items()}
            ids, _, lps = e.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]], want_logprobs=True, **kw)
            solo.append((ids[0], lps[0]))
        assert not np.array_equal(solo[0][0], plain[0]) and not np.array_equal(solo[2][0], plain[2]), "the table or the grammar binds nowhere: the test shows nothing"
        assert np.array_equal(solo[3][0], plain[3]) and np.array_equal(solo[5][0], plain[5])
        plug = [synth.synth_pcm(690, 128000)] * e.max_batch                                               # max_batch windows of 8 s behind one prompt
        plug_prompt = [1, 17, 23, 5] + [d.audio_token_id] * spec.audio_token_count(e.max_batch * spec.valid_frames(128000)) + [7, 301, 302, 303, 9, 11]
        slots = [e.slot(), e.slot()]
        disp = Dispatcher([e], slots=[slots], continuous=True, native=native, decoders=2)                   # two decoding handles, ONE prefill slot
        rep = disp.replicas[0]
        assert type(rep).__name__ == ("_NativeContinuousReplica" if native else "_ContinuousReplica") and len(rep.prefill_engines) == 1
        first = disp.submit(plug, plug_prompt, 4)
        futs = [disp.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True, **own[i]) for i in range(6)]
        res = [f.result(timeout=120) for f in futs]
        assert len(first.result(timeout=120)) >= 1
        batches = rep.batches
        disp.close()
        for s in slots:
            s.close()
        gram.close()
        print(f"mixed per-request values ({'native' if native else 'python'} dispatcher): {batches} prefill batches for the plug and the six requests")
        for i in range(6):
            assert np.array_equal(res[i][0], solo[i][0]) and _same(res[i][1], solo[i][1]), (native, i, res[i][0], solo[i][0])
        assert batches < 7, f"{batches} prefill batches for 7 requests: every request was prefilled alone, the mix was not reached"
    finally:
        e.close()
