"""The forms of the token step, one eager run each: which chain decode_step() picks for a row count and an option, read back as
sonic_timings.decode_launches_per_layer (include/sonic_hip.h), and the two pairs of forms that must give the same BITS.

  rows  option             launches per layer   chain
  1, 2  -                  5                    PRE form: q|k|v (and the lm_head) consume down_proj's slabs themselves
  2     no_pre_norm        6                    fused o_proj + gate/up, standalone add+RMSNorm behind down_proj
  3     -                  6                    the same
  3     decode_gemv        5                    the opt-in GEMV chain (gemv.hip)
  33    -                  6                    the same fused chain, gate/up normalising in LDS
  33    gu64_split_norm    7                    ... with the RMSNorm as its own launch (the continuous loops' form)
  5     no_fused_gu        8                    unfused: o_proj slabs, add+RMSNorm, gate/up slabs, SwiGLU
  2     int8 engine        8                    the Linear8bitLt step

Bit-exact pairs (the pairs tests/test_gpu_parity.py pins at other shapes, nothing stronger): 2 rows with and without no_pre_norm, 33 rows with and
without gu64_split_norm."""
from dataclasses import replace

import numpy as np
import pytest

from gpu_common import make_engine
from sonicscribe_amd import spec, synth

pytestmark = pytest.mark.gpu

N_NEW = 3


def _requests(d, R):
    lens = [16000 * (1 + (i % 2)) + 37 * i for i in range(R)]                 # 1 .. 2 s segments, ragged
    segs = [synth.synth_pcm(400 + i, n) for i, n in enumerate(lens)]
    prompts = [[1, 17, 23, 5] + [d.audio_token_id] * spec.audio_token_count(spec.valid_frames(n)) + [7, 301, 302, 303, 9, 11][: 3 + i % 4]
               for i, n in enumerate(lens)]
    return segs, prompts


def _run(e, d, R, option=None):
    """One eager batch of R requests with `option` set to 1 for its duration -> (launches per layer, step logits)."""
    segs, prompts = _requests(d, R)
    if option:
        e.set_option(option, 1)
    try:
        _, logits = e.transcribe_batch(segs, prompts, [N_NEW] * R, want_logits=True)
        return e.timings()["decode_launches_per_layer"], logits
    finally:
        if option:
            e.set_option(option, 0)


def test_step_forms_launch_counts_and_bit_exact_pairs():
    from sonicscribe_amd.engine import Engine, MODE_INT8
    d = replace(spec.FULL, enc_layers=1, dec_layers=2, vocab=1024, audio_token_id=1000, eos_ids=())
    e = Engine(d, 0, max_batch=64, max_ctx=384)
    e.load_synthetic(11)
    cases = [(1, None, 5), (2, None, 5), (2, "no_pre_norm", 6), (3, None, 6), (3, "decode_gemv", 5), (33, None, 6), (33, "gu64_split_norm", 7),
             (5, "no_fused_gu", 8)]
    got, logits = {}, {}
    for R, option, _ in cases:
        got[R, option], logits[R, option] = _run(e, d, R, option)
    e.close()
    e8 = make_engine(mode=MODE_INT8, max_batch=8, max_ctx=512)
    got["int8", None], _ = _run(e8, spec.TINY, 2)
    e8.close()
    print("decode_launches_per_layer:", got)
    want = {(R, option): n for R, option, n in cases}
    want["int8", None] = 8
    assert got == want
    for R, option in ((2, "no_pre_norm"), (33, "gu64_split_norm")):
        assert logits[R, None].shape == logits[R, option].shape and logits[R, None].shape[0] == N_NEW
        assert np.array_equal(logits[R, None].view(np.uint32), logits[R, option].view(np.uint32)), (R, option)
