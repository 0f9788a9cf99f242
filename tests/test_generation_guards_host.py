"""Generation guards, host side (sonicscribe_amd/genconfig.py): GenerationGuards.apply against HF's own logits processors on CPU torch, bit for bit,
and what load() makes of a checkpoint's generation_config.json.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

from gpu_common import same_bits
from sonicscribe_amd import genconfig
from sonicscribe_amd.genconfig import GenerationGuards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 97


def hf_apply(scores, history, p, n, sup):
    """HF's LogitsProcessorList in generate()'s order on CPU torch: one row"""
    torch = pytest.importorskip("torch")
    from transformers.generation.logits_process import (LogitsProcessorList, NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    procs = LogitsProcessorList()
    if p is not None:
        procs.append(RepetitionPenaltyLogitsProcessor(penalty=p))
    if n:
        procs.append(NoRepeatNGramLogitsProcessor(n))
    if sup:
        procs.append(SuppressTokensLogitsProcessor(sup, device="cpu"))
    ids = torch.tensor([list(history)], dtype=torch.long)
    out = procs(ids, torch.from_numpy(np.array(scores, np.float32, copy=True))[None])
    return out[0].numpy()


def scores_for(rng, history):
    """random fp32 scores with 0.0, -0.0, negative, and +/- large values, the special ones placed on history ids too"""
    s = rng.normal(0, 4, V).astype(np.float32)
    s[rng.integers(0, V, 6)] = np.float32(0.0)
    s[rng.integers(0, V, 6)] = np.float32(-0.0)
    s[rng.integers(0, V, 4)] = np.float32(3.0e38)
    s[rng.integers(0, V, 4)] = np.float32(-3.0e38)
    s[rng.integers(0, V, 4)] = np.float32(1.0e-42)            # subnormal
    h = list(dict.fromkeys(history))
    for k, v in zip(h, (0.0, -0.0, 3.0e38, -3.0e38, -1.75, 2.5)):
        s[k] = np.float32(v)
    return s


def histories(n):
    """duplicates, id 0 and id V - 1; shorter than n, n - 1 long, longer than n with a repeated (n - 1)-gram"""
    base = [0, V - 1, 5, 7, 5, 7, 0, V - 1, 5, 7, 11, 5, 5, 5, 0, V - 1, 5]
    out = [base, base + [7], [5] * 9, [0, V - 1] * 6]
    out.append(base[:max(n - 2, 0)])
    out.append(base[:max(n - 1, 0)])
    out.append(base[:n])
    out.append(base[:n + 1])
    return [h for h in out if len(h) > 0]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_apply_equals_hf_bit_for_bit(n):
    rng = np.random.default_rng(100 + n)
    sup = [0, V - 1, 13, 13, 40]
    n_ban = n_pen = 0
    for h in histories(n):
        s = scores_for(rng, h)
        for p in (1.05, 1.1, 1.2, 1.3, 2.0, 0.8):
            for cfg in ((p, 0, []), (None, n, []), (None, 0, sup), (p, n, sup), (p, n, [])):
                g = GenerationGuards(*cfg)
                got, want = g.apply(s, h), hf_apply(s, h, *cfg)
                assert same_bits(got, want), (n, h, cfg, np.flatnonzero(got.view(np.int32) != want.view(np.int32))[:5])
                assert np.array_equal(np.isneginf(got), np.isneginf(want))
                n_ban += int(cfg[1] > 0 and np.isneginf(got).any())
                n_pen += int(cfg[0] is not None and not same_bits(got, s))
    assert n_ban > 0 and n_pen > 0                                   # the cases bind


def test_ngram_edges():
    g = GenerationGuards(no_repeat_ngram_size=3)
    assert g.banned_ngram_tokens([]) == [] and g.banned_ngram_tokens([4]) == [] and g.banned_ngram_tokens([4, 5]) == []     # shorter than n, and n - 1 long
    assert g.banned_ngram_tokens([4, 5, 6, 4, 5]) == [6]
    assert sorted(GenerationGuards(no_repeat_ngram_size=1).banned_ngram_tokens([3, 3, 9])) == [3, 3, 9]
    assert GenerationGuards(no_repeat_ngram_size=2).banned_ngram_tokens([7, 7]) == [7]
    s = np.zeros(V, np.float32)
    assert same_bits(GenerationGuards().apply(s, [1, 2, 3]), s) and not GenerationGuards().active
    assert GenerationGuards(1.0, 0, []).active is False and GenerationGuards(1.1).active and GenerationGuards(None, 2).active and GenerationGuards(None, None, [3]).active
    # a penalty is applied once however often the id occurs
    s[5] = 2.0
    assert GenerationGuards(2.0).apply(s, [5, 5, 5])[5] == np.float32(1.0)
    # the float64-then-round form differs from the fp32 operations somewhere: the restatement uses fp32
    x = np.random.default_rng(0).normal(0, 5, 200000).astype(np.float32)
    p = 1.3
    assert not np.array_equal((x.astype(np.float64) / p).astype(np.float32), x / np.float32(p))


def test_constructor_refuses():
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=65), dict(suppress_tokens=list(range(257))), dict(suppress_tokens=[-1])):
        with pytest.raises(ValueError):
            GenerationGuards(**bad)
    assert len(GenerationGuards(suppress_tokens=list(range(256))).suppress_tokens) == 256


def _write(tmp_path, cfg):
    with open(os.path.join(tmp_path, "generation_config.json"), "w") as f:
        json.dump(cfg, f)
    return str(tmp_path)


def test_load(tmp_path):
    assert genconfig.load(str(tmp_path)) == GenerationGuards() and not genconfig.load(str(tmp_path)).active          # no file: off
    d = _write(tmp_path, {"repetition_penalty": 1.2, "no_repeat_ngram_size": 3, "suppress_tokens": [4, 9], "eos_token_id": [1, 2], "pad_token_id": 0,
                          "do_sample": True, "temperature": 0.7, "top_k": 20, "top_p": 0.9, "min_p": 0.1, "typical_p": 0.5, "epsilon_cutoff": 0.1,
                          "num_beams": 1, "num_beam_groups": 1, "min_length": 0, "min_new_tokens": None, "bad_words_ids": None, "penalty_alpha": None,
                          "encoder_repetition_penalty": 1.0, "encoder_no_repeat_ngram_size": 0, "forced_eos_token_id": None, "max_new_tokens": 128,
                          "transformers_version": "5.0.0"})
    g = genconfig.load(d)
    assert g.as_dict() == {"repetition_penalty": 1.2, "no_repeat_ngram_size": 3, "suppress_tokens": [4, 9]} and g.active
    assert g.override(no_repeat_ngram_size=0).as_dict() == {"repetition_penalty": 1.2, "no_repeat_ngram_size": 0, "suppress_tokens": [4, 9]}
    assert g.override(1.0, 0, []).active is False
    assert genconfig.load(_write(tmp_path, {"repetition_penalty": None, "suppress_tokens": None})) == GenerationGuards()
    # fields that touch the scores but leave a greedy run's ids alone pass (genconfig.py says why); the neutral values of the refused ones too
    assert genconfig.load(_write(tmp_path, {"renormalize_logits": True, "remove_invalid_values": True, "stop_strings": None, "watermarking_config": None,
                                            "guidance_scale": 1.0, "exponential_decay_length_penalty": None})) == GenerationGuards()


@pytest.mark.parametrize("field,value", [
    ("num_beams", 4), ("num_beam_groups", 2), ("bad_words_ids", [[5, 6]]), ("min_new_tokens", 3), ("min_length", 2), ("begin_suppress_tokens", [7]),
    ("sequence_bias", [[[5], -2.0]]), ("forced_bos_token_id", 1), ("forced_eos_token_id", 2), ("forced_decoder_ids", [[1, 5]]),
    ("encoder_repetition_penalty", 1.5), ("encoder_no_repeat_ngram_size", 2), ("penalty_alpha", 0.6),
    ("exponential_decay_length_penalty", [10, 1.5]), ("guidance_scale", 1.5), ("stop_strings", ["."]), ("watermarking_config", {"bias": 2.5})])
def test_load_refuses_by_name(tmp_path, field, value):
    with pytest.raises(ValueError, match=re.escape(field)):
        genconfig.load(_write(tmp_path, {"repetition_penalty": 1.1, field: value}))


def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    from sonicscribe_amd import engine
    for name in ("sonic_set_generation", "sonic_get_generation", "sonic_test_greedy_guard"):
        assert name in engine.EXPORTS and re.search(r"SONIC_API int " + name + r"\(", hdr)
    assert all(hasattr(engine.Engine, m) for m in ("set_generation", "get_generation", "test_greedy_guard"))
    if os.path.exists(engine.LIB_PATH):
        import ctypes as C
        lib = C.CDLL(engine.LIB_PATH)
        assert hasattr(lib, "sonic_set_generation") and lib.sonic_set_generation(None, C.c_float(1.0), 0, None, 0) == 1      # SONIC_ERR_INVALID for no handle
