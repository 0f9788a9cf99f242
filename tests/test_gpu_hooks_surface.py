"""The test / bench / debug surface of the library that no other file walks: sonic_debug_read name by name (csrc/engine_options.cpp), the two bench
hooks (csrc/engine_hooks.cpp), sonic_debug_ktrace, and the refusals of sonic_set_option that the option, sampling and request-bias files do not assert.
Everything here is a property of the C ABI: accepted names and capacities, refusal messages, and one value pin (debug_read("pe") against the embeds
sonic_encode returns - both read the same buffer)."""
import numpy as np
import pytest

from gpu_common import make_engine, prompt_for
from sonicscribe_amd import spec, synth

pytestmark = pytest.mark.gpu
D = spec.TINY
BM, CTX = 1, 512
TOK_CAP = BM * min(CTX, D.max_audio_tokens + 256)
QD = D.dec_heads * D.dec_head_dim
# name -> elements the library serves (sonic_debug_read's capacities, from the engine's allocation sizes)
CAP16 = {
    "prefill_tap": TOK_CAP * D.dec_d, "pe": BM * D.max_audio_tokens * D.dec_d, "dx": TOK_CAP * D.dec_d, "dqkv": TOK_CAP * (QD + 2 * D.dec_kv_heads * D.dec_head_dim),
    "dq": TOK_CAP * QD, "datt": TOK_CAP * QD, "dact": TOK_CAP * D.dec_ff, "enc_x": BM * D.enc_T * D.enc_d, "shn": 64 * D.dec_d, "satt": 64 * QD, "sact": 64 * D.dec_ff,
}
CAP32 = {"prefill_tap": TOK_CAP * D.dec_d, "pe": BM * D.max_audio_tokens * D.dec_d, "dx": TOK_CAP * D.dec_d, "enc_x": BM * D.enc_T * D.enc_d,
         "h1": BM * (D.n_frames + 2) * D.enc_d}


def _pcm_prompt():
    pcm = synth.synth_pcm(10, 80000)
    return pcm, prompt_for(D, len(pcm))


def _engine(mode):
    return make_engine(D, mode, BM, CTX)


@pytest.fixture(scope="module")
def e16():
    from sonicscribe_amd.engine import MODE_NATIVE
    e = _engine(MODE_NATIVE)
    yield e
    e.close()


@pytest.fixture(scope="module")
def e32():
    from sonicscribe_amd.engine import MODE_F32
    e = _engine(MODE_F32)
    yield e
    e.close()


def _walk_debug_read(e, caps, other_kind):
    from sonicscribe_amd.engine import SonicError
    pcm, prompt = _pcm_prompt()
    e.transcribe_batch([pcm], [prompt], [4])
    with pytest.raises(SonicError, match="no taps recorded"):
        e.debug_read("prefill_tap", (1,))
    e.set_option("prefill_taps", 1)
    e.transcribe_batch([pcm], [prompt], [4])
    e.set_option("prefill_taps", 0)
    for name, cap in caps.items():
        for index in ((0, D.dec_layers) if name == "prefill_tap" else (0,)):
            assert e.debug_read(name, (cap,), index).shape == (cap,)
        with pytest.raises(SonicError, match=f"exceeds buffer {name}"):
            e.debug_read(name, (cap + 1,))
    for name in (other_kind, "no_such_buffer"):
        with pytest.raises(SonicError, match="unknown buffer"):
            e.debug_read(name, (1,))
    # the value pin: sonic_encode's embeds and debug_read("pe") are two read-backs of one buffer
    feats, mask = e.logmel([pcm])
    emb = e.encode(feats, [int(mask[0].sum())])[0]
    pe = e.debug_read("pe", emb.shape)
    assert np.array_equal(pe.view(np.uint32), emb.view(np.uint32))


def test_debug_read_16bit(e16):
    _walk_debug_read(e16, CAP16, "h1")


def test_debug_read_fp32(e32):
    _walk_debug_read(e32, CAP32, "dqkv")


def test_bench_gemm(e16):
    from sonicscribe_amd.engine import SonicError
    for epi in (0, 1):
        ms = e16.bench_gemm(128, 128, 64, epi, iters=2)
        assert np.isfinite(ms) and ms > 0, (epi, ms)
    with pytest.raises(SonicError, match="bad gemm bench shape"):
        e16.bench_gemm(128, 128, 65, 0, iters=2)
    with pytest.raises(SonicError, match="bad gemm bench shape"):
        e16.bench_gemm(128, 128, 64, 0, iters=0)
    ms = e16.bench_gemm(1500, 192, 64, 4, iters=2)             # the encoder's q|k|v epilogue: V^T per 1500-frame segment
    assert np.isfinite(ms) and ms > 0, ms
    with pytest.raises(SonicError, match="QKV bench needs"):
        e16.bench_gemm(128, 192, 64, 4, iters=2)


def test_bench_skinny(e16):
    from sonicscribe_amd.engine import SonicError
    rng = np.random.default_rng(5)
    X = rng.standard_normal((1, 256)).astype(np.float32); W = (rng.standard_normal((64, 256)) * 0.1).astype(np.float32)
    before = e16.test_skinny(X, W)
    us = e16.bench_skinny(1, 64, 256, 0, iters=2)
    assert np.isfinite(us) and us > 0, us
    with pytest.raises(SonicError, match="bad skinny bench shape"):
        e16.bench_skinny(65, 64, 256, 0, iters=2)
    after = e16.test_skinny(X, W)                               # the bench's variant was for its own call only
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


def test_set_option_refusals():
    from sonicscribe_amd.engine import MODE_NATIVE, SonicError
    e = _engine(MODE_NATIVE)
    try:
        with pytest.raises(SonicError, match="request_bias_fill: -1 is outside"):
            e.set_option("request_bias_fill", -1)
        with pytest.raises(SonicError, match="sampling_fill_milli: 100001 is outside"):
            e.set_option("sampling_fill_milli", 100001)
        with pytest.raises(SonicError, match="unknown option gen_nonsense"):
            e.set_option("gen_nonsense", 1)
        e.set_option("token_logprobs", 1)
        e.set_option("sampling", 1)
        with pytest.raises(SonicError, match="token_logprobs cannot be switched off while option sampling is on"):
            e.set_option("token_logprobs", 0)
        e.set_option("sampling", 0)
        e.set_option("token_logprobs", 0)
    finally:
        e.close()


def test_debug_ktrace():
    from sonicscribe_amd.engine import MODE_NATIVE, SonicError
    e = _engine(MODE_NATIVE)
    try:
        with pytest.raises(SonicError, match="ktrace is off"):
            e.debug_ktrace()
        e.set_option("ktrace", 0)
        pcm, prompt = _pcm_prompt()
        e.transcribe_batch([pcm], [prompt], [4])
        kt = e.debug_ktrace()
        assert kt.shape == (8, 512, 8) and kt.dtype == np.int64
    finally:
        e.close()
