"""Mode fp8 without a device: sonicscribe_amd/fp8.py - the numpy statement of the snap that tests/test_gpu_fp8.py holds the library to - against
torch.float8_e4m3fn, the tensors snap_state_dict touches, the C surface of the two options, and ASRModel(mode="fp8")'s argument handling."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import abi_pins
from sonicscribe_amd import fp8, spec, synth


def bf16(a):
    """float32 values rounded to bfloat16 (as float32)"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def torch_codes(v):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def torch_values(codes):
    return torch.from_numpy(np.ascontiguousarray(codes, np.uint8)).view(torch.float8_e4m3fn).float().numpy()


def rows_under_test():
    rng = np.random.default_rng(5)
    K = 96
    rows = [np.zeros(K, np.float32)]                                              # an all-zero row: s = 1
    for e in (-14, 0, 3):                                                         # amax exactly 448 * 2^e; every e4m3 subnormal of the row's grid and the ties between them
        r = bf16(rng.standard_normal(K) * 100.0 * 2.0 ** e)
        r[0] = -448.0 * 2.0 ** e
        r[1:18] = np.arange(17) * 2.0 ** (e - 10)                                 # k / 2 subnormal steps: 0, tie, 1, tie, 2, ... 8 (the first normal)
        r[18:35] = -r[1:18]
        rows.append(r)
    for e in (-14, 0):                                                            # amax just above 448 * 2^e: 450 is the next bfloat16, the scale doubles
        r = bf16(rng.standard_normal(K) * 50.0 * 2.0 ** e)
        r[5] = 450.0 * 2.0 ** e
        rows.append(r)
    rows.append(bf16(rng.standard_normal(K) * 1e-6))                              # rows of very different magnitude in one matrix
    rows.append(bf16(rng.standard_normal(K) * 3e4))
    rows.append(bf16(rng.standard_normal(K) * 0.02))
    half = np.zeros(K, np.float32); half[0] = 1.0; half[1:9] = [0.5, 0.51953125, 0.53125, 0.5625, 0.59375, 0.96875, 0.984375, 1.0]      # ties between normal codes
    rows.append(half)
    return np.stack(rows).astype(np.float32)


def test_snap_against_torch_float8_e4m3fn():
    w = rows_under_test()
    assert np.array_equal(bf16(w), w)                                             # bf16-valued rows, as a checkpoint's
    wp, s, codes = fp8.snap(w)
    assert wp.dtype == s.dtype == np.float32 and codes.dtype == np.uint8
    amax = np.abs(w).max(axis=1)
    assert s[0] == 1.0 and np.array_equal(np.exp2(np.round(np.log2(s))), s)       # powers of two
    nz = amax > 0
    assert ((amax[nz] / s[nz] > 224) & (amax[nz] / s[nz] <= 448)).all()
    assert np.array_equal(amax[1:4] / s[1:4], [448.0] * 3) and np.array_equal(amax[4:6] / s[4:6], [225.0] * 2)
    v = w / s[:, None]
    assert np.array_equal(v * s[:, None], w)                                      # W / s is exact
    assert np.array_equal(codes, torch_codes(v))                                  # the codes are torch's round-to-nearest-even
    assert np.array_equal(fp8.decode(codes).view(np.uint32), torch_values(codes).view(np.uint32))
    assert np.array_equal(wp.view(np.uint32), (s[:, None] * torch_values(codes)).view(np.uint32))
    assert np.array_equal(bf16(wp).view(np.uint32), wp.view(np.uint32))           # W' is exact in bfloat16
    assert (codes[1:4, 1:35] & 0x7F).max() == 8 and len(np.unique(codes[1, 1:18])) == 9      # the subnormal codes 0 .. 7 and the first normal were reached
    wp2, s2, codes2 = fp8.snap(wp)                                                # idempotent: W' is a fixed point.  (Its scale may be the next one down: a row whose
    assert np.array_equal(wp2.view(np.uint32), wp.view(np.uint32))                # amax / s = 225 rounds to 224 = 448 / 2; s2 q2 is then the same value written twice as fine)
    assert (s2 <= s).all() and np.array_equal(s2[:4], s[:4]) and np.array_equal(s2[4:6] * 2, s[4:6]) and np.array_equal(fp8.snap(wp2)[1], s2)
    assert np.array_equal(fp8.row_scales(w), s)


def test_every_code_and_every_bfloat16_against_torch():
    codes = np.arange(256, dtype=np.uint8)
    tv = torch_values(codes)
    ok = ~np.isnan(tv)                                                            # 0x7f / 0xff: NaN, never written by the snap
    assert np.array_equal(fp8.decode(codes)[ok].view(np.uint32), tv[ok].view(np.uint32))
    assert np.array_equal(fp8.encode(tv[ok]), codes[ok])
    b = (np.arange(65536, dtype=np.uint32) << 16).view(np.float32)
    b = b[np.isfinite(b) & (np.abs(b) <= 448)]
    assert np.array_equal(fp8.encode(b), torch_codes(b))
    with pytest.raises(ValueError, match="not finite"):
        fp8.row_scales(np.array([[1.0, np.inf]], np.float32))


def test_snap_state_dict_touches_the_decoder_projections_and_the_embedding_only():
    d = replace(spec.TINY, dec_layers=2)
    sd = synth.synth_state_dict(d, 7, bf16=True)
    out = fp8.snap_state_dict(sd, d)
    assert set(out) == set(sd)
    changed = {k for k in sd if not np.array_equal(out[k], sd[k])}
    lm = "model.language_model."
    want = {lm + "embed_tokens.weight"} | {f"{lm}layers.{i}.{n}.weight" for i in range(d.dec_layers)
                                           for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")}
    assert changed == want == set(fp8.snapped_names(d))
    assert not any("audio_tower" in k or "projector" in k or "norm" in k for k in changed)
    for k in want:                                                                # per-row scales: packing q|k|v (or gate/up) first changes nothing
        assert np.array_equal(out[k].view(np.uint32), fp8.snap(sd[k])[0].view(np.uint32))
    p = lm + "layers.0.self_attn."
    qkv = np.concatenate([sd[p + n + "_proj.weight"] for n in "qkv"])
    assert np.array_equal(fp8.snap(qkv)[0], np.concatenate([out[p + n + "_proj.weight"] for n in "qkv"]))
    qd, kd = d.dec_heads * d.dec_head_dim, d.dec_kv_heads * d.dec_head_dim
    mats = [(qd + 2 * kd, d.dec_d), (d.dec_d, qd), (2 * d.dec_ff, d.dec_d), (d.dec_d, d.dec_ff)] * d.dec_layers + [(d.vocab, d.dec_d)]
    assert fp8.extra_weight_bytes(d) == sum(n * k + 4 * n for n, k in mats)
    f = spec.FULL                                                                 # the full-size model: about 1.47 GB beside the bf16 weights
    assert 1.46e9 < fp8.extra_weight_bytes(f) < 1.48e9


def test_the_c_surface_carries_the_two_options():
    abi_pins.check_surface(options=("fp8_weights", "fp8_chain"), header_strings=("fp8_step_builds", "fp8_scales", "fp8_matrix", "e4m3"), engine_methods=("fp8_info", "fp8_scales", "fp8_matrix"))


def test_asrmodel_fp8_argument_handling(tmp_path):
    import json
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.engine import MODE_INT8
    with pytest.raises(ValueError, match="mode must be either"):
        ASRModel("<none>", mode="fp4")
    with pytest.raises(ValueError, match="mode='fp8' is not supported with _engine_mode"):
        ASRModel("<none>", mode="fp8", _engine_mode=MODE_INT8)
    with pytest.raises(ValueError, match="mode='fp8' is not supported with _options fp8_weights=0"):
        ASRModel("<none>", mode="fp8", _options={"fp8_weights": 0})
    # the mode snaps the checkpoint's own bfloat16 values: it asks for the checkpoint ahead of any device
    with pytest.raises(ValueError, match="mode='fp8' needs a bfloat16 checkpoint to snap: .*config.json not found"):
        ASRModel(str(tmp_path / "nowhere"), mode="fp8", device="cpu")
    half = tmp_path / "half"; half.mkdir(); (half / "config.json").write_text(json.dumps({"torch_dtype": "float16"}))
    with pytest.raises(ValueError, match="states torch_dtype float16"):
        ASRModel(str(half), mode="fp8", device="cpu")
    ck = tmp_path / "bf16"; ck.mkdir(); (ck / "config.json").write_text(json.dumps({"torch_dtype": "bfloat16", "text_config": {}}))
    # the rules of "native" hold, those of "int8" do not apply: draft_verify and score_share_prompt pass the argument stage (the device is refused behind it)
    with pytest.raises(ValueError, match="sampling=True needs token_logprobs=True"):
        ASRModel(str(ck), mode="fp8", sampling=True)
    with pytest.raises(ValueError, match="draft_verify is not supported with mode='int8'"):
        ASRModel(str(ck), mode="int8", draft_verify=True, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ASRModel(str(ck), mode="fp8", draft_verify=True, token_logprobs=True, scoring=True, score_share_prompt=True, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the synthetic model brings no checkpoint to ask for
        ASRModel.from_synthetic(spec.TINY, mode="fp8", device="cpu")
