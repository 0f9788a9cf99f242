"""sonic_set_option (csrc/engine_options.cpp): the experiment knobs are one table, and this file pins what that table has to keep - the accepted key set
written out below, the "unknown option" error for anything else, the four clamped knobs taking any integer, and the drop of the captured decode graphs
when a knob that changes the captured kernels moves (a decode after no_fused_gu = 1 then 0 runs the default kernels again, not a stale graph)."""
import numpy as np
import pytest

from gpu_common import make_engine, prompt_for
from sonicscribe_amd import spec, synth

pytestmark = pytest.mark.gpu

KEYS = [
    "skinny_variant", "gemm_force128", "no_fused_gu", "no_fused_gu64", "gu64_two_pass", "gu64_split_norm", "ktrace_wave", "no_skinny768", "no_skinny48",
    "o64_16rows", "i8_no_lnq", "i8_no_qkv_fuse", "i8_dbg", "i8_no_xq", "gemm_small_eff", "gemm128_shallow", "no_skinny_i8_wide", "gemm256_stagger",
    "flash_variant", "flash_enc", "gemm256_persist", "gemm256_persist_cus", "gemm256_gm", "i8_defer_thr", "decode_prefetch", "decode_attn_occ2",
    "decode_attn_v1", "prefill_taps", "no_pre_norm", "decode_gemv", "f32_synth_bf16", "no_graph", "decode_lookahead", "decode_chunk", "prefill_rowmajor",
    "no_rope_tiles", "gemm_trace", "gemm_timing", "no_fused_rope", "ktrace", "inject_dev_err", "no_gelu_lut",
]
CLAMPED = ["gemm256_persist_cus", "gemm256_gm", "decode_lookahead", "decode_chunk"]


def test_option_table():
    from sonicscribe_amd.engine import SonicError
    d = spec.TINY
    pcm = synth.synth_pcm(10, 80000)
    prompt = prompt_for(d, len(pcm))
    n_new = 12
    ref = make_engine(d, max_batch=2, max_ctx=512)             # the untouched engine
    want = ref.transcribe_batch([pcm], [prompt], [n_new])[0][0]
    ref.close()

    e = make_engine(d, max_batch=2, max_ctx=512)
    assert np.array_equal(e.transcribe_batch([pcm], [prompt], [n_new])[0][0], want)      # captures the default decode graphs
    e.set_option("no_fused_gu", 1)
    e.transcribe_batch([pcm], [prompt], [n_new])                                         # captures the unfused form
    e.set_option("no_fused_gu", 0)
    assert np.array_equal(e.transcribe_batch([pcm], [prompt], [n_new])[0][0], want)      # the graph drop is live

    assert len(set(KEYS)) == len(KEYS) == 42
    for k in KEYS:
        e.set_option(k, 0)                                                               # raises SonicError when not accepted
    e.set_option("ktrace", -1)
    for k in CLAMPED:
        e.set_option(k, 0)
        e.set_option(k, 1 << 20)
    for k in ("", "no_such_knob", "no_fused_gu ", "NO_GRAPH", "opt_no_graph"):
        with pytest.raises(SonicError, match="unknown option"):
            e.set_option(k, 1)
    e.close()
