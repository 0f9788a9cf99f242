"""Generation guards on the GPU (sonic_set_generation; greedy_kernel<T, LP, true>): HF's repetition_penalty, no_repeat_ngram_size and
suppress_tokens inside the greedy kernel.  The reference is sonicscribe_amd.genconfig.GenerationGuards.apply, which tests/test_generation_guards_host.py
holds bit for bit against HF's own processors: the emitted token must be np.argmax (first maximum) of apply(raw logits the kernel dumped, history),
exactly.  Log-probabilities are held to DESIGN.md 6.3's derived bound (tests/gpu_common.py lp_bound), evaluated over the processed scores."""
import json
import os

import numpy as np
import pytest

from gpu_common import SEED, check_lp, flags, load_golden, make_engine, prompt_for, same_bits, slabs
from sonicscribe_amd import spec, synth
from sonicscribe_amd.genconfig import GenerationGuards

pytestmark = pytest.mark.gpu
ALL3 = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[304, 10])
PENALTY_THAT_BINDS = 1.5            # on tiny_bf16.npz both rows leave the fixture's ids at the second token (1.2 moves s0 only, 1.1 at step 10)


def make(d=spec.TINY, mode=0, max_batch=4, max_ctx=1024, lp=False, guards=None):
    return make_engine(d, mode, max_batch, max_ctx, flags((lp, "token_logprobs", 1), (guards, "generation", guards)))


@pytest.fixture(scope="module")
def eng():
    e = make(lp=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden(golden_dir):
    g, segs, prompts = load_golden(golden_dir, int_prompts=True)
    return g, segs, prompts, int(g["n_new"])


# ------------------------------------------------------------------------------------------ 1. the kernel hook, exact
def _ids(V):
    """A: in row 1's history (the last id: the last partial vector at V = 16388); C: in no history; Z: continuation of (x, y); S: suppressed; A2 < C: in row 2's history"""
    return dict(A=V - 1, C=V // 2, Z=V - 2, x=1, y=2, S=V - 3, A2=3)


def _histories(V, rng):
    k = _ids(V)
    pool = [0, k["A"], k["x"]] + ([9, 77, V - 4, V - 5] if V > 8 else [])           # duplicates, id 0 and id V - 1; never C or S
    fill = [int(pool[i]) for i in rng.integers(0, len(pool), 1024 - 5)]
    h1 = [k["x"], k["y"], k["Z"]] + fill + [k["x"], k["y"]]                          # 1024 entries: (x, y, Z) early, ends with (x, y)
    h2 = [0, k["A2"], k["x"], k["y"], k["Z"], 0, k["x"], k["y"]]
    hist = np.zeros((3, 1024), np.int32)
    hist[1, :] = h1; hist[2, :len(h2)] = h2
    return hist, np.array([0, 1024, len(h2)], np.int32)                              # row 0: no history


def _check_rows(eng, V, ks, rows, hist, hlen, guards, want_lp=False, force=None, tag=""):
    s = slabs(rows, ks)
    tok, raw, lp = eng.test_greedy_guard(s, 3, hist, hlen, force_ids=force, want_lp=want_lp, **guards)
    tok0, raw0 = eng.test_greedy(s, 3, want_logits=True)
    assert np.array_equal(raw.view(np.uint32), raw0.view(np.uint32)), (tag, "the dump is the raw logits")
    g = GenerationGuards(**guards)
    worst = 0.0
    for b in range(3):
        proc = g.apply(raw[b], hist[b, :hlen[b]])
        want = int(np.argmax(proc)) if force is None else int(force[b])
        assert int(tok[b]) == want, (tag, V, ks, b, int(tok[b]), want)
        if want_lp:
            worst = max(worst, check_lp((tag, V, ks, b), lp[b], proc, tok[b]))
    return tok, tok0, raw, worst


@pytest.mark.parametrize("V", [8, 1024, 16388, 59264])
def test_kernel_hook_exact(eng, V):
    rng = np.random.default_rng(V)
    k = _ids(V)
    hist, hlen = _histories(V, rng)
    worst = 0.0
    for ks in (1, 2, 3):
        def base(lo=-2.0, hi=2.0):
            return [rng.uniform(lo, hi, V).astype(np.float32) for _ in range(3)]
        # the raw argmax is in the history and the penalty demotes it: the pick changes (row 1); rows 0 and 2 keep it
        rows = base()
        for r in rows:
            r[k["A"]] = 5.0; r[k["C"]] = 4.5
        tok, tok0, _, _ = _check_rows(eng, V, ks, rows, hist, hlen, dict(repetition_penalty=1.3), tag="demote")
        assert list(tok0) == [k["A"]] * 3 and list(tok) == [k["A"], k["C"], k["A"]]
        # a tie created by the penalty: 6 / 2 == 3, the lower index wins (row 1: C < A; row 2: A2 < C)
        rows = base()
        rows[1][k["A"]] = 6.0; rows[1][k["C"]] = 3.0; rows[2][k["A2"]] = 6.0; rows[2][k["C"]] = 3.0; rows[0][k["C"]] = 3.0
        tok, tok0, _, _ = _check_rows(eng, V, ks, rows, hist, hlen, dict(repetition_penalty=2.0), tag="tie")
        assert list(tok0) == [k["C"], k["A"], k["A2"]] and list(tok) == [k["C"], k["C"], k["A2"]]
        # the raw argmax continues an earlier occurrence of the last n - 1 ids: banned (n = 1: every id seen; n = 4: whatever the history holds)
        rows = base()
        for r in rows:
            r[k["Z"]] = 5.0; r[k["C"]] = 4.5
        for n in (1, 2, 3):
            tok, tok0, _, _ = _check_rows(eng, V, ks, rows, hist, hlen, dict(no_repeat_ngram_size=n), tag=f"ngram{n}")
            assert list(tok0) == [k["Z"]] * 3 and list(tok) == [k["Z"], k["C"], k["C"]]
        _check_rows(eng, V, ks, rows, hist, hlen, dict(no_repeat_ngram_size=4), tag="ngram4")
        _check_rows(eng, V, ks, rows, hist, np.array([0, 2, 3], np.int32), dict(no_repeat_ngram_size=4), tag="ngram4 short")     # shorter than n, and n - 1 long
        # a suppressed id is the raw argmax (every row, the one without a history too)
        rows = base()
        for r in rows:
            r[k["S"]] = 5.0; r[k["C"]] = 4.5
        tok, tok0, _, _ = _check_rows(eng, V, ks, rows, hist, hlen, dict(suppress_tokens=[k["S"], k["A"]]), tag="suppress")
        assert list(tok0) == [k["S"]] * 3 and list(tok) == [k["C"]] * 3
        # 0.0 and -0.0 at history ids, everything else negative: they tie, the lower index wins, penalty or not
        rows = base(-2.0, -1.0)
        for r in rows:
            r[k["x"]] = -0.0; r[k["y"]] = 0.0
        tok, _, raw, _ = _check_rows(eng, V, ks, rows, hist, hlen, dict(repetition_penalty=1.3), tag="zeros")
        assert list(tok) == [k["x"]] * 3 and np.signbit(raw[1, k["x"]]) and not np.signbit(raw[1, k["y"]])
        # all three, with log-probabilities over the processed scores
        rows = base()
        for r in rows:
            r[k["S"]] = 6.0; r[k["Z"]] = 5.5; r[k["A"]] = 5.0; r[k["C"]] = 4.5; r[k["x"]] = -0.0; r[k["y"]] = 0.0
        g3 = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, suppress_tokens=[k["S"]])
        tok, tok0, _, w = _check_rows(eng, V, ks, rows, hist, hlen, g3, want_lp=True, tag="all3")
        worst = max(worst, w)
        assert list(tok0) == [k["S"]] * 3 and list(tok) == [k["Z"], k["C"], k["A"]]
        # teacher forcing: the forced id is emitted whatever the guards say; a banned forced id has log-probability -inf
        force = np.array([k["C"], k["Z"], k["S"]], np.int32)
        _, _, _, w = _check_rows(eng, V, ks, rows, hist, hlen, g3, want_lp=True, force=force, tag="forced")
        worst = max(worst, w)
        if V == 8:                                                                   # every id banned: token 0 (torch.argmax of equal values)
            tok, _, _, _ = _check_rows(eng, V, ks, rows, hist, hlen, dict(suppress_tokens=list(range(8))), tag="all banned")
            assert list(tok) == [0, 0, 0]
            h8 = np.zeros((3, 1024), np.int32); h8[2, :8] = [3, 1, 4, 0, 5, 7, 2, 6]
            tok, _, _, _ = _check_rows(eng, V, ks, rows, h8, np.array([0, 0, 8], np.int32), dict(no_repeat_ngram_size=1), tag="all seen")
            assert tok[2] == 0
    print(f"guard hook V={V}: worst |lp - ref64| / bound = {worst:.3f}")


# ------------------------------------------------------------------------------------------ 2. end to end at TINY, eager loop
def _identity(ids, logits, prompts, guards, n_new, rows=(0, 1)):
    """every row, every step: argmax(apply(dumped raw logits, prompt + ids so far)) is the emitted id"""
    g = GenerationGuards(**guards)
    for si in rows:
        n = len(ids[si])
        assert 1 <= n <= n_new and (n == n_new or int(ids[si][-1]) in spec.TINY.eos_ids)       # the budget, or an EOS the guards let through
        for s in range(n):
            proc = g.apply(logits[s, si], list(prompts[si]) + [int(t) for t in ids[si][:s]])
            assert int(np.argmax(proc)) == int(ids[si][s]), (guards, si, s)


@pytest.mark.parametrize("name", ["penalty", "ngram", "suppress", "all3"])
def test_end_to_end_eager(golden, name):
    g, segs, prompts, n_new = golden
    guards = {"penalty": dict(repetition_penalty=PENALTY_THAT_BINDS), "ngram": dict(no_repeat_ngram_size=2), "suppress": dict(suppress_tokens=[304, 10]), "all3": ALL3}[name]
    e = make(guards=guards)
    try:
        assert e.get_generation() == GenerationGuards(**guards).as_dict() | {"repetition_penalty": float(np.float32(GenerationGuards(**guards).repetition_penalty))}
        ids, logits = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True)
        _identity(ids, logits, prompts, guards, n_new)
        for si in range(2):
            ref = g[f"s{si}_new_ids"]
            n = min(len(ids[si]), len(ref))
            diff = np.flatnonzero(np.asarray(ids[si][:n]) != ref[:n])
            print(f"tiny s{si} {name}: first step that differs from the unguarded fixture: {diff[0] if diff.size else None}; ids {list(map(int, ids[si]))}")
            if name in ("ngram", "all3", "suppress"):
                assert diff.size                                                    # the guard binds: the fixture rows are 24 equal ids
            if name == "ngram":
                assert int(ids[si][2]) != int(ref[2])                               # (g, g) happened: g is banned at the third token
                for s in range(2, n):
                    assert not (ids[si][s] == ids[si][s - 1] == ids[si][s - 2])
            if name == "suppress":
                assert not np.isin(ids[si], [304, 10]).any()
        if name == "penalty":
            assert all(int(ids[si][0]) == int(g[f"s{si}_new_ids"][0]) and int(ids[si][1]) != int(g[f"s{si}_new_ids"][1]) for si in range(2))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 3. the same bits on every path
def test_invariance_engine_paths():
    d = spec.TINY
    segs = [synth.synth_pcm(700 + i, n) for i, n in enumerate((48000, 200000, 80000))]
    prompts = [prompt_for(d, len(s)) for s in segs]
    budgets = [5, 17, 11]
    e = make(lp=True, guards=ALL3)
    try:
        ids_e, logits_e, lp_e = e.transcribe_batch(segs, prompts, budgets, want_logits=True, want_logprobs=True)       # eager
        g = GenerationGuards(**ALL3)
        for r in range(3):
            for s in range(len(ids_e[r])):
                proc = g.apply(logits_e[s, r], prompts[r] + [int(t) for t in ids_e[r][:s]])
                assert int(np.argmax(proc)) == int(ids_e[r][s])
                check_lp(("paths", r, s), lp_e[r][s], proc, ids_e[r][s])
        ids3, lg, lp3 = e.transcribe_batch(segs, prompts, budgets, want_logprobs=True)                                    # hipGraph loop
        assert lg is None and e.timings()["host_decode_launches"] < max(budgets) - 1
        ids1, _, lp1 = e.transcribe_batch([segs[2]], [prompts[2]], [budgets[2]], want_logprobs=True)                     # alone vs row 2 of 3
        for r in range(3):
            assert np.array_equal(ids3[r], ids_e[r]) and same_bits(lp3[r], lp_e[r]), r
        assert np.array_equal(ids1[0], ids3[2]) and same_bits(lp1[0], lp3[2])
        # spliced into a continuous loop mid-flight: the history travels with the row
        pre = e.slot()
        assert pre.get_generation() == e.get_generation()
        e.service_begin()
        try:
            pre.stage_pcm([segs[1]]); pre.prefill([prompts[1]], [budgets[1]])
            seq1 = e.splice_rows(pre, [0], [2])
            for _ in range(3):
                e.service_step(1, 4)                                                                                     # row 2 is under way ...
            pre.stage_pcm([segs[0], segs[2]]); pre.prefill([prompts[0], prompts[2]], [budgets[0], budgets[2]])
            seq = e.splice_rows(pre, [1, 0], [3, 1])                                                                      # ... when two more join
            got, rows = {}, {3: 2, 1: 0, 2: 1}
            for _ in range(200):
                fin, nn, s_, _ = e.service_step(1, 4)
                done = [r for r in rows if r not in got and s_ > max(seq, seq1) and fin[r]]
                if done:
                    a, b = e.fetch_rows(done, [int(nn[r]) for r in done], want_logprobs=True)
                    for r, x, y in zip(done, a, b):
                        got[r] = (x, y)
                if len(got) == 3:
                    break
            assert len(got) == 3
            for row, req in rows.items():
                assert np.array_equal(got[row][0], ids3[req]) and same_bits(got[row][1], lp3[req]), (row, req)
        finally:
            e.service_end()
            pre.close()
    finally:
        e.close()


def test_invariance_native_dispatcher_and_bulk_pipeline():
    from sonicscribe_amd.dispatch import Dispatcher
    d = spec.TINY
    segs = [synth.synth_pcm(700 + i, n) for i, n in enumerate((48000, 200000, 80000))]
    prompts = [prompt_for(d, len(s)) for s in segs]
    budgets = [5, 17, 11]
    e = make(max_batch=32, lp=True, guards=ALL3)
    plain = make(max_batch=32)
    try:
        solo = [e.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]], want_logprobs=True) for i in range(3)]
        unguarded = [plain.transcribe_batch([segs[i]], [prompts[i]], [budgets[i]])[0][0] for i in range(3)]
        assert any(not np.array_equal(solo[i][0][0], unguarded[i]) for i in range(3))                                   # the guards bind on these requests
        slots = [e.slot(), e.slot()]
        disp = Dispatcher([e], slots=[slots], continuous=True)
        assert type(disp.replicas[0]).__name__ == "_NativeContinuousReplica"
        res = [f.result(timeout=60) for f in [disp.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True) for i in range(3)]]
        disp.close()
        for i in range(3):
            assert np.array_equal(res[i][0], solo[i][0][0]) and same_bits(res[i][1], solo[i][2][0]), i
        bulk = Dispatcher([e], slots=[slots], bulk=True, decoders=1)
        res = [f.result(timeout=60) for f in [bulk.submit([segs[i]], prompts[i], budgets[i], want_logprobs=True) for i in range(3)]]
        bulk.close()
        for i in range(3):
            assert np.array_equal(res[i][0], solo[i][0][0]) and same_bits(res[i][1], solo[i][2][0]), i
    finally:
        e.close(); plain.close()


# ------------------------------------------------------------------------------------------ 4. modes
@pytest.mark.parametrize("mode", [1, 2, 3], ids=["int8", "f16", "f32"])
def test_modes_identity(mode, golden):
    g, segs, prompts, n_new = golden
    e = make(mode=mode, guards=ALL3)
    try:
        ids, logits = e.transcribe_batch(segs, prompts, [n_new, n_new], want_logits=True)
        _identity(ids, logits, prompts, ALL3, n_new)
        assert all(not np.isin(ids[si], [304, 10]).any() for si in range(2))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ 5. live HF
def test_live_hf_generate_with_guards_vs_fp32_engine_through_checkpoint(tmp_path):
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    from tests import hf_helpers as G
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.engine import MODE_F32
    d = spec.TINY
    p, n, sup, n_new = 1.3, 2, [304, 10], 24          # chosen on the CPU: every step's top-1 / top-2 margin of HF's processed scores is > 4e-3 on this input
    model, _ = G.build_tiny(torch.float32)
    model.generation_config.repetition_penalty = p
    model.generation_config.no_repeat_ngram_size = n
    model.generation_config.suppress_tokens = sup
    model.save_pretrained(str(tmp_path), safe_serialization=True)
    cfg = json.load(open(os.path.join(str(tmp_path), "generation_config.json")))
    assert cfg["repetition_penalty"] == p and cfg["no_repeat_ngram_size"] == n and cfg["suppress_tokens"] == sup
    pcm = synth.synth_pcm(10, 80000)
    feats, mask = G.mel_case(G.feature_extractor(), pcm)
    ids = G.PROMPT_PREFIX + [d.audio_token_id] * spec.audio_token_count(int(mask.sum())) + G.PROMPT_SUFFIX
    input_ids = torch.tensor([ids], dtype=torch.long)
    with torch.no_grad():
        gen = model.generate(input_ids=input_ids, input_features=torch.from_numpy(feats)[None], input_features_mask=torch.from_numpy(mask)[None].long(),
                             attention_mask=torch.ones_like(input_ids), max_new_tokens=n_new, do_sample=False, repetition_penalty=p, no_repeat_ngram_size=n,
                             suppress_tokens=sup, return_dict_in_generate=True, output_scores=True, output_logits=True)
    ref_ids = gen.sequences[0, len(ids):].numpy().astype(np.int32)
    scores = torch.stack([s[0] for s in gen.scores]).numpy()
    raw = torch.stack([s[0] for s in gen.logits]).numpy()
    m = ASRModel(str(tmp_path), max_batch=2, max_ctx=1024, slots=1, continuous=False, _allow_synthetic_prompt=True, _engine_mode=MODE_F32)      # no guard arguments: the file is read
    try:
        info = m.get_model_info()
        assert info["repetition_penalty"] == p and info["no_repeat_ngram_size"] == n and info["suppress_tokens"] == sup
        got, _ = m.model.transcribe_batch([pcm], [ids], [n_new])
        srt = np.sort(scores, axis=1)
        margin = srt[:, -1] - srt[:, -2]
        clear = len(margin) if (margin > 1e-3).all() else int(np.argmin(margin > 1e-3))       # compare up to the first step without a clear margin
        changed = np.flatnonzero(raw.argmax(axis=1)[:clear] != ref_ids[:clear])
        print(f"live HF with guards: {len(ref_ids)} steps, {clear} with margin > 1e-3 (min {margin.min():.4f}), the guards changed the pick at steps {changed.tolist()}")
        assert clear >= 16 and changed.size >= 1
        assert np.array_equal(got[0][:clear], ref_ids[:clear]), (got[0].tolist(), ref_ids.tolist())
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 6. off is off; refusals
def test_off_is_off_and_refusals(golden):
    from sonicscribe_amd.engine import SonicError
    g, segs, prompts, n_new = golden
    plain = make(lp=True)
    off = make(lp=True)
    try:
        off.set_generation(1.0, 0, [])
        want = plain.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)
        got = off.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)
        a0 = off.memory_info()[0]
        for si in range(2):
            assert np.array_equal(got[0][si], want[0][si]) and same_bits(got[2][si], want[2][si])
        assert plain.memory_info()[0] == a0                                          # nothing was allocated for the neutral values
        # on, then back to the neutral values: the plain run's bits again
        off.set_generation(1.3, 2, [304])
        assert off.memory_info()[0] >= a0 + 64 * 1024 * 4                            # the history is counted
        on = off.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)
        assert not np.array_equal(on[0][0], want[0][0])
        off.set_generation(1.0, 0, [])
        got = off.transcribe_batch(segs, prompts, [n_new, n_new], want_logprobs=True)
        for si in range(2):
            assert np.array_equal(got[0][si], want[0][si]) and same_bits(got[2][si], want[2][si])
        # refusals: values out of range
        V = spec.TINY.vocab
        for bad in ((0.0, 0, []), (-1.0, 0, []), (float("inf"), 0, []), (float("nan"), 0, []), (1.1, -1, []), (1.1, 65, []), (1.1, 0, [V]), (1.1, 0, [-1]),
                    (1.1, 0, list(range(257)))):
            with pytest.raises(SonicError, match="sonic_set_generation"):
                off.set_generation(*bad)
        off.set_generation(1.1, 64, list(range(256)))
        off.set_generation(1.0, 0, [])
        # refusals: rows are running
        off.stage_pcm(segs[:1]); off.prefill(prompts[:1], [8])
        with pytest.raises(SonicError, match="running"):
            off.set_generation(1.2, 0, [])
        off.decode_step(100)
        off.set_generation(1.2, 0, [])
        off.set_generation(1.0, 0, [])
        off.service_begin()
        with pytest.raises(SonicError, match="continuously"):
            off.set_generation(1.2, 0, [])
        off.service_end()
        # a splice from a source whose guards differ is refused
        off.set_generation(1.2, 0, [])
        pre = off.slot()
        pre.set_generation(1.0, 0, [])
        off.service_begin()
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [4])
        with pytest.raises(SonicError, match="generation guards"):
            off.splice_rows(pre, [0], [0])
        # a prefill slot whose rows were all handed over is free again, although its own decode loop never ran
        pre.decode_step(100)
        pre.set_generation(1.2, 0, [])
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [4])
        with pytest.raises(SonicError, match="running"):
            pre.set_generation(1.0, 0, [])
        off.splice_rows(pre, [0], [0])
        pre.set_generation(1.0, 0, [])
        off.service_end()
        # the other way round is refused too: the destination decodes without guards, the source prefilled with them
        off.set_generation(1.0, 0, [])
        pre.set_generation(1.2, 0, [])
        off.service_begin()
        pre.stage_pcm(segs[:1]); pre.prefill(prompts[:1], [4])
        with pytest.raises(SonicError, match="generation guards"):
            off.splice_rows(pre, [0], [0])
        off.service_end()
        # the integer keys of sonic_set_option go through the same busy check (that batch of pre's has not been decoded)
        with pytest.raises(SonicError, match="running"):
            pre.set_option("gen_no_repeat_ngram_size", 2)
        pre.decode_step(100)
        pre.set_option("gen_no_repeat_ngram_size", 2)
        assert pre.get_generation()["no_repeat_ngram_size"] == 2
        pre.close()
    finally:
        plain.close(); off.close()


# ------------------------------------------------------------------------------------------ 7. ASRModel
def test_asrmodel_surface(tmp_path):
    from sonicscribe_amd import weights
    from sonicscribe_amd.asr import ASRModel
    ck = str(tmp_path)
    weights.save_synthetic_checkpoint(ck, spec.TINY, SEED)
    wav = synth.synth_pcm(31, 80000).astype(np.float32) / 32768.0
    kw = dict(max_batch=4, max_ctx=1024, _allow_synthetic_prompt=True)

    def run(**extra):
        m = ASRModel(ck, **kw, **extra)
        try:
            return m.transcribe(wav, max_new_tokens=12), m.get_model_info(), [e.get_generation() for e in [m.model] + m._slot_engines[0]]
        finally:
            m.close()

    t_plain, info, gens = run()                                                      # no generation_config.json: off
    assert (info["repetition_penalty"], info["no_repeat_ngram_size"], info["suppress_tokens"]) == (1.0, 0, [])
    assert all(g == {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "suppress_tokens": []} for g in gens)
    with open(os.path.join(ck, "generation_config.json"), "w") as f:
        json.dump({"repetition_penalty": 1.3, "no_repeat_ngram_size": 2, "suppress_tokens": [304, 10], "temperature": 0.6, "top_k": 40, "do_sample": True}, f)
    t_file, info, gens = run()                                                       # the file is honoured, on the owner and its slots
    assert (info["repetition_penalty"], info["no_repeat_ngram_size"], info["suppress_tokens"]) == (1.3, 2, [304, 10])
    assert len(gens) >= 2 and all(g["no_repeat_ngram_size"] == 2 and g["suppress_tokens"] == [304, 10] and abs(g["repetition_penalty"] - 1.3) < 1e-6 for g in gens)
    assert t_file != t_plain
    t_kw, info, gens = run(repetition_penalty=1.0, no_repeat_ngram_size=0, suppress_tokens=[])      # the arguments override the file
    assert (info["repetition_penalty"], info["no_repeat_ngram_size"], info["suppress_tokens"]) == (1.0, 0, []) and t_kw == t_plain
    _, info, _ = run(no_repeat_ngram_size=3)                                         # one argument: the others stay the file's
    assert (info["repetition_penalty"], info["no_repeat_ngram_size"], info["suppress_tokens"]) == (1.3, 3, [304, 10])
    with open(os.path.join(ck, "generation_config.json"), "w") as f:
        json.dump({"repetition_penalty": 1.3, "num_beams": 4}, f)
    with pytest.raises(ValueError, match="num_beams"):                               # a field the engine does not implement: refused at construction, by name
        ASRModel(ck, **kw)
