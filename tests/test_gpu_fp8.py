"""Mode fp8 (options fp8_weights / fp8_chain; csrc/gemv_fp8.hip): the decoder's matrices snapped onto per-row power-of-two-scaled e4m3 grids (W'),
and the 1 - 4 row token step streaming the e4m3 copies.  The contract is exactness, so almost everything here is a bit comparison:
  * the quantiser: the library's scales and e4m3 copies equal sonicscribe_amd/fp8.py's (which tests/test_fp8_host.py holds to torch.float8_e4m3fn), the weight
    bytes grow by sum N K + 4 sum N;
  * the kernels: engine A (load_synthetic, then fp8_weights = 1) on the fp8 chain equals engine B (the numpy reference's W' loaded as an ordinary bf16 checkpoint)
    on the bf16 GEMV chain, bit for bit, for every row subset, twice;
  * the rest of the model is W': above 4 rows, in the prefill and with fp8_chain = 0 engine A equals engine B's default chain bit for bit;
  * against the CPU oracle on the snapped state dict: the bound tests/test_gpu_gemv.py holds the bf16 GEMV chain to; free-running ids outside near-ties;
  * through continuous loops (R = 2 / R = 4 chunk graphs), the refusals, the ASRModel(mode="fp8") facade;
  * recorded, not gated: W' against the unsnapped model on the synthetic weights (which say little about a real checkpoint: not measured on speech)."""
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest

from gpu_common import SEED, prompt_for, same_bits
from sonicscribe_amd import fp8, spec, synth

pytestmark = pytest.mark.gpu

FULLW = replace(spec.FULL, enc_layers=1, dec_layers=2, vocab=1024, audio_token_id=1000, eos_ids=())     # full-width layers (K = 2048 and K = 6144), shallow
N_NEW = 10
LM = "model.language_model."


def _engine(d, mode=None, **kw):
    from sonicscribe_amd.engine import Engine, MODE_NATIVE
    return Engine(d, 0, MODE_NATIVE if mode is None else mode, **kw)


@pytest.fixture(scope="module")
def ctx():
    d = FULLW
    sd = synth.synth_state_dict(d, SEED, bf16=True)
    snapped = fp8.snap_state_dict(sd, d)
    a = _engine(d, max_batch=8, max_ctx=512)
    a.load_synthetic(SEED)
    before = (a.weight_bytes(), a.memory_info()[0])
    a.set_option("fp8_weights", 1)
    after = (a.weight_bytes(), a.memory_info()[0])
    b = _engine(d, max_batch=8, max_ctx=512)
    b.load_state_dict(snapped)
    segs = [synth.synth_pcm(30 + i, 16000 * (2 + 3 * (i % 4))) for i in range(5)]
    prompts = [prompt_for(d, len(s), tail=[40 + i] * (i % 4)) for i, s in enumerate(segs)]
    force = np.random.default_rng(8).integers(2, min(d.vocab, 900), size=(5, N_NEW)).astype(np.int32)
    force[force == d.audio_token_id] = 7
    c = SimpleNamespace(d=d, sd=sd, snapped=snapped, a=a, b=b, before=before, after=after, segs=segs, prompts=prompts, force=force, cache={})
    yield c
    a.close()
    b.close()


def run(c, e, rows, opts=()):
    """N_NEW teacher-forced steps of `rows` on engine e with the (key, value, value afterwards) options set around the run -> (step logits [step][row][V], launches per layer)"""
    for k, v, _ in opts:
        e.set_option(k, v)
    e.set_forced_ids(c.force[rows])
    try:
        _, lg = e.transcribe_batch([c.segs[r] for r in rows], [c.prompts[r] for r in rows], [N_NEW] * len(rows), want_logits=True)
        per_layer = e.timings()["decode_launches_per_layer"]
    finally:
        e.set_forced_ids(None)
        for k, _, v in opts:
            e.set_option(k, v)
    return lg, per_layer


def cached(c, key, e, rows, opts=()):
    if key not in c.cache:
        c.cache[key] = run(c, e, rows, opts)
    return c.cache[key]


GEMV = (("decode_gemv", 1, 0),)
CHAIN_OFF = (("fp8_chain", 0, 1),)


def packed(c, m):
    """matrix m of the snapped set as the engine packs its rows (plain tilings only: q|k|v, o_proj, down_proj, the lm_head), from the synthetic state dict"""
    if m == 4 * c.d.dec_layers:
        return c.sd[LM + "embed_tokens.weight"]
    p = f"{LM}layers.{m // 4}."
    if m % 4 == 0:
        return np.concatenate([c.sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"])
    return c.sd[p + {1: "self_attn.o_proj.weight", 3: "mlp.down_proj.weight"}[m % 4]]


def test_quantiser_equals_the_numpy_reference_and_the_bytes_the_formula(ctx):
    c, d = ctx, ctx.d
    last = d.dec_layers - 1
    for m, rows in ((0, None), (1, None), (3, None), (4 * last + 0, 40), (4 * last + 1, 40), (4 * last + 3, 40), (4 * d.dec_layers, None)):
        w = packed(c, m)
        wp, s, _ = fp8.snap(w)
        n = w.shape[0] if rows is None else rows                   # (40 rows: two tiles and a half)
        assert same_bits(c.a.fp8_scales(m, w.shape[0]), s), m
        assert same_bits(c.a.fp8_matrix(m, n, w.shape[1]), wp[:n]), m
    qd, kd, D, ff = d.dec_heads * d.dec_head_dim, d.dec_kv_heads * d.dec_head_dim, d.dec_d, d.dec_ff
    mats = [(qd + 2 * kd, D), (D, qd), (2 * ff, D), (D, ff)] * d.dec_layers + [(d.vocab, D)]
    extra = sum(n * k for n, k in mats) + 4 * sum(n for n, _ in mats)
    assert c.after[0] - c.before[0] == extra == fp8.extra_weight_bytes(d) == c.a.fp8_info()["extra_weight_bytes"]
    assert c.after[1] - c.before[1] == extra                       # the memory info moves by the same bytes
    assert c.a.fp8_info()["matrices"] == 4 * d.dec_layers + 1


def test_fp8_chain_equals_the_bf16_gemv_chain_on_the_snapped_weights(ctx):
    c = ctx
    builds = c.a.fp8_info()["step_builds"]
    lg_a, per_layer = c.cache["a4"] = run(c, c.a, [0, 1, 2, 3])
    assert per_layer == 5 and c.a.fp8_info()["step_builds"] > builds
    lg_b, per_layer_b = cached(c, "b4_gemv", c.b, [0, 1, 2, 3], GEMV)
    assert per_layer_b == 5
    assert lg_a.dtype == np.float32 and np.array_equal(lg_a.view(np.uint32), lg_b.view(np.uint32))
    for rows in ([0], [2], [1, 3], [0, 1, 2]):                      # a row's bits do not depend on its neighbours
        lg_s, _ = run(c, c.a, rows)
        lg_r, _ = run(c, c.b, rows, GEMV)
        for k, r in enumerate(rows):
            assert np.array_equal(lg_s[:, k].view(np.uint32), lg_a[:, r].view(np.uint32)), (rows, r)
            assert np.array_equal(lg_r[:, k].view(np.uint32), lg_a[:, r].view(np.uint32)), (rows, r)
    lg_2, _ = run(c, c.a, [0, 1, 2, 3])                             # deterministic
    assert np.array_equal(lg_2.view(np.uint32), lg_a.view(np.uint32))
    # ... and it is the fp8 form that ran, not the default chain on W': that one adds an output's K products in another order
    lg_d, _ = cached(c, "b4", c.b, [0, 1, 2, 3])
    assert np.array_equal(lg_a[0], lg_d[0]) and not np.array_equal(lg_a, lg_d)


def test_the_rest_of_the_model_is_the_snapped_model(ctx):
    c = ctx
    rows5 = [0, 1, 2, 3, 4]
    builds = c.a.fp8_info()["step_builds"]
    lg_a5, per_layer = run(c, c.a, rows5)                           # five rows: the MFMA chain, and step 0 is the prefill
    lg_b5, per_layer_b = run(c, c.b, rows5)
    assert per_layer == per_layer_b
    assert np.array_equal(lg_a5.view(np.uint32), lg_b5.view(np.uint32))
    lg_off, _ = run(c, c.a, [0, 1, 2, 3], CHAIN_OFF)               # fp8_chain = 0: W' on the default chain
    lg_d, _ = cached(c, "b4", c.b, [0, 1, 2, 3])
    assert np.array_equal(lg_off.view(np.uint32), lg_d.view(np.uint32))
    assert c.a.fp8_info()["step_builds"] == builds                  # neither run built a step in the fp8 form


def test_against_the_oracle_on_the_snapped_state_dict(ctx):
    from oracle import oracle
    c, d = ctx, ctx.d
    lg_a, _ = cached(c, "a4", c.a, [0, 1, 2, 3])
    om = oracle.Model(d, c.snapped, bf16=True)
    tol = 4 * 2.0 ** -6                                             # the bound tests/test_gpu_gemv.py holds the bf16 GEMV chain to
    for r in (0, 3):
        feats, mask = oracle.logmel(c.segs[r])
        o = om.transcribe(feats, int(mask.sum()), c.prompts[r], N_NEW, force_ids=c.force[r])
        err = float(np.abs(lg_a[:, r] - o["step_logits"]).max())
        print(f"fp8 chain, row {r} vs the oracle on W': max |dlogit| {err:.5f} (bound {tol:.5f})")
        assert err <= tol
    # free running: ids equal engine B's default chain wherever that chain's top-two margin is not a near-tie
    ulp = 2.0 ** -6
    ids_a, _ = c.a.transcribe_batch(c.segs[:2], c.prompts[:2], [12, 12], want_logits=True)
    ids_d, lgd = c.b.transcribe_batch(c.segs[:2], c.prompts[:2], [12, 12], want_logits=True)
    for r in range(2):
        srt = np.sort(lgd[:, r], axis=1)
        safe = (srt[:, -1] - srt[:, -2]) > 8 * ulp
        n_safe = len(safe) if safe.all() else int(np.argmin(safe))
        assert np.array_equal(ids_a[r][:n_safe], ids_d[r][:n_safe]), (r, ids_a[r], ids_d[r])


def test_fp8_chain_in_continuous_loops(ctx):
    c, d, e = ctx, ctx.d, ctx.a
    segs = [synth.synth_pcm(60 + i, 16000 * (2 + i)) for i in range(4)]
    prompts = [prompt_for(d, len(s)) for s in segs]
    solo = [e.transcribe_batch([s], [p], [14])[0][0] for s, p in zip(segs, prompts)]
    builds = e.fp8_info()["step_builds"]
    pre = e.slot()
    try:
        e.service_begin()
        assert e.fp8_info()["step_builds"] > builds                 # the R = 2 and R = 4 chunk graphs were captured in the fp8 form
        got, seq = {}, {}
        for step in range(300):
            if step < 4:                                            # rows join one by one: R = 2 graphs, then R = 4
                pre.stage_pcm(segs[step:step + 1]); pre.prefill(prompts[step:step + 1], [14]); seq[step] = e.splice_rows(pre, [0], [step])
            live = [r for r in seq if r not in got]
            if not live and step >= 4:
                break
            fin, nn, s_, _ = e.service_step(1, max(live) + 1 if live else 1)
            for r in live:
                if s_ > seq[r] and fin[r]:
                    got[r] = e.fetch_row(r, int(nn[r]))
        e.service_end()
        for r in range(4):
            assert np.array_equal(got[r], solo[r]), r
    finally:
        pre.close()


def test_refusals_by_name_and_the_ineligible_shapes():
    from sonicscribe_amd.engine import MODE_F16, MODE_INT8, SonicError
    d = spec.TINY
    for mode, kind in ((MODE_INT8, "int8"), (MODE_F16, "fp16")):
        e = _engine(d, mode, max_batch=4, max_ctx=512)
        e.load_synthetic(SEED)
        with pytest.raises(SonicError, match=rf"fp8_weights: only on a bf16 handle.*{kind}"):
            e.set_option("fp8_weights", 1)
        e.close()
    e = _engine(d, max_batch=4, max_ctx=512)
    e.load_synthetic(SEED)
    with pytest.raises(SonicError, match="fp8_chain: option fp8_weights must be on first"):
        e.set_option("fp8_chain", 1)
    with pytest.raises(SonicError, match="fp8_weights is off"):
        e.fp8_info()
    s = e.slot()
    with pytest.raises(SonicError, match="fp8_weights: the owner already has 1 slot"):
        e.set_option("fp8_weights", 1)
    with pytest.raises(SonicError, match="fp8_weights: this handle is a slot"):
        s.set_option("fp8_weights", 1)
    s.close()
    e.set_option("fp8_weights", 1)
    with pytest.raises(SonicError, match="fp8_weights cannot be switched off"):
        e.set_option("fp8_weights", 0)
    with pytest.raises(SonicError, match="fp8_chain: 2 is neither 0 nor 1"):
        e.set_option("fp8_chain", 2)
    e.set_option("fp8_weights", 1)                                   # (again: nothing to do)
    # TINY's K = 256 has an odd number of k-steps per wave: the chain is not eligible, the snapped model runs the default chains - and a slot inherits the option
    s = e.slot()
    assert s.fp8_info()["matrices"] == 4 * d.dec_layers + 1
    b = _engine(d, max_batch=4, max_ctx=512)
    b.load_state_dict(fp8.snap_state_dict(synth.synth_state_dict(d, SEED, bf16=True), d))
    segs = [synth.synth_pcm(30 + i, 16000 * (2 + i)) for i in range(2)]
    prompts = [prompt_for(d, len(x)) for x in segs]
    for h in (e, s):
        ids_a, lg_a = h.transcribe_batch(segs, prompts, [6, 6], want_logits=True)
        ids_b, lg_b = b.transcribe_batch(segs, prompts, [6, 6], want_logits=True)
        assert np.array_equal(lg_a.view(np.uint32), lg_b.view(np.uint32)) and all(np.array_equal(x, y) for x, y in zip(ids_a, ids_b))
        assert h.fp8_info()["step_builds"] == 0
    s.close(); e.close(); b.close()


def test_asrmodel_fp8_mode_and_a_native_model_beside_it(ctx):
    from sonicscribe_amd.asr import ASRModel
    c, d = ctx, ctx.d
    m = ASRModel.from_synthetic(d, SEED, mode="fp8", max_batch=4, max_ctx=512)
    pcm = synth.synth_pcm(70, 80000)
    t = m.transcribe((pcm.astype(np.float32) / 32768.0)[None], 16000, max_new_tokens=6)
    ids, _ = c.a.transcribe_batch([pcm], [prompt_for(d, len(pcm))], [6])      # the engine-level result: engine A is the same model
    assert t == " ".join(str(int(i)) for i in ids[0])
    info = m.get_model_info()
    assert info["mode"] == "fp8" and info["model_dtype"] == "torch.bfloat16"
    assert info["fp8_weights_mb"] == fp8.extra_weight_bytes(d) / 1024 ** 2 and info["fp8_step_builds"] > 0
    assert m.model.weight_bytes() == c.after[0]
    # a native model in the same process is the unsnapped model: its logits are a fresh native engine's
    n = ASRModel.from_synthetic(d, SEED, mode="native", max_batch=4, max_ctx=512, continuous=False)      # (its owner handle stays free for the direct runs below)
    assert n.get_model_info()["mode"] == "native" and n.model.weight_bytes() == c.before[0]
    lg_n, _ = run(c, n.model, [0, 1, 2, 3])
    fresh = _engine(d, max_batch=4, max_ctx=512)
    fresh.load_synthetic(SEED)
    lg_f, _ = run(c, fresh, [0, 1, 2, 3])
    assert np.array_equal(lg_n.view(np.uint32), lg_f.view(np.uint32))
    fresh.close(); n.close(); m.close()
    # recorded, not gated: W' against the unsnapped bf16 model on the synthetic weights (teacher forced; both on their default <= 4-row forms)
    lg_a, _ = cached(c, "a4", c.a, [0, 1, 2, 3])
    dd = np.abs(lg_a - lg_f)
    agree = float((lg_a.argmax(-1) == lg_f.argmax(-1)).mean())
    print(f"W' (fp8 chain) vs the unsnapped bf16 model, {N_NEW} teacher-forced steps x 4 rows, synthetic weights: max |dlogit| {float(dd.max()):.4f}, mean {float(dd.mean()):.5f}, "
          f"argmax agreement {agree:.3f}; logits in [{lg_f.min():.2f}, {lg_f.max():.2f}] (not measured on speech)")
