"""ctypes binding of libsonic_hip.so (include/sonic_hip.h).

The product path fails loudly when the HIP library is missing or no GPU is visible; there is no
CPU fallback (the CPU oracle lives under oracle/ and is test infrastructure only).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import reqvalues
from .engine_hooks import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_SWIGLU, EPI_QKV_VT, GemmForm, HooksMixin, _arr, _p  # noqa: F401
from .spec import ModelDims

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libsonic_hip.so")

MODE_NATIVE, MODE_INT8, MODE_F16, MODE_F32 = 0, 1, 2, 3
DTYPE_F32, DTYPE_BF16, DTYPE_I32 = 0, 1, 2
SONIC_ERR_MISMATCH, SONIC_ERR_UNSUPPORTED = 4, 5

ABI_VERSION = 13


class SonicDims(C.Structure):
    _fields_ = [
        ("n_mels", C.c_int32), ("n_frames", C.c_int32), ("enc_T", C.c_int32),
        ("enc_d", C.c_int32), ("enc_ff", C.c_int32), ("enc_layers", C.c_int32), ("enc_heads", C.c_int32), ("enc_rotary_dim", C.c_int32),
        ("enc_theta", C.c_float), ("enc_ln_eps", C.c_float),
        ("merge", C.c_int32),
        ("dec_d", C.c_int32), ("dec_ff", C.c_int32), ("dec_layers", C.c_int32), ("dec_heads", C.c_int32), ("dec_kv_heads", C.c_int32), ("dec_head_dim", C.c_int32),
        ("dec_theta", C.c_float), ("dec_rms_eps", C.c_float),
        ("vocab", C.c_int32), ("audio_token_id", C.c_int32), ("n_eos", C.c_int32),
        ("eos", C.c_int32 * 8),
    ]


class SonicTimings(C.Structure):
    _fields_ = [
        ("mel_ms", C.c_float), ("encoder_ms", C.c_float), ("prefill_ms", C.c_float), ("decode_ms", C.c_float), ("total_ms", C.c_float),
        ("gemm_ms", C.c_float), ("gemm_launches", C.c_int32), ("gemm_flops", C.c_double), ("decode_steps", C.c_int32),
        ("enc_gemm_ms", C.c_float), ("enc_gemm_flops", C.c_double),
        ("host_prefill_enqueue_ms", C.c_float), ("host_decode_launch_ms", C.c_float), ("host_decode_wait_ms", C.c_float), ("host_decode_launches", C.c_int32),
        ("decode_lookahead", C.c_int32), ("decode_launches_per_layer", C.c_int32),
    ]


class DispatchRequest(C.Structure):
    """sonic_dispatch_request: one request as sonic_dispatch_submit takes it.  A fresh record is all-zero - a request that brings no value of its own - with `size` set"""
    _fields_ = [
        ("size", C.c_int64),
        ("host_pcm", C.c_void_p), ("host_off", C.c_void_p), ("rings", C.c_void_p), ("ring_start", C.c_void_p), ("ring_n", C.c_void_p), ("W", C.c_int32),
        ("prompt_ids", C.c_void_p), ("prompt_len", C.c_int32), ("max_new", C.c_int32),
        ("seq_ids", C.c_void_p), ("seq_off", C.c_void_p), ("bias", C.c_void_p), ("n_seq", C.c_int32),
        ("sampled", C.c_int32), ("temperature", C.c_float), ("seed", C.c_uint64),
        ("cut", C.c_int32), ("top_k", C.c_float), ("top_p", C.c_float), ("min_p", C.c_float),
        ("grammar_id", C.c_int32),
        ("draft_ids", C.c_void_p), ("n_draft", C.c_int32),
    ]

    def __init__(self, **kw):
        super().__init__(size=C.sizeof(DispatchRequest), **kw)


# Every export of include/sonic_hip.h: name -> (return type, argument types).  The one place the binding states the C signatures; tests/test_binding_signatures.py
# checks it against the header, declaration by declaration (ctypes would not: a wrong entry is silent stack corruption).
I, F, I64, U64, S, vp = C.c_int, C.c_float, C.c_int64, C.c_uint64, C.c_char_p, C.c_void_p
ip, i64p, fp, vpp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_void_p)
SIGNATURES = {
    "sonic_device_count": (I, []),
    "sonic_create": (I, [C.POINTER(SonicDims)] + [I] * 4 + [vpp]),
    "sonic_destroy": (None, [vp]),
    "sonic_last_error": (S, [vp]),
    "sonic_load_tensor": (I, [vp, S, vp, I, i64p, I]),
    "sonic_load_synthetic": (I, [vp, U64]),
    "sonic_finalize_weights": (I, [vp]),
    "sonic_weight_bytes": (I64, [vp]),
    "sonic_logmel": (I, [vp, vp, vp, I, vp, vp]),
    "sonic_encode": (I, [vp, vp, vp, I] + [vp] * 4),
    "sonic_transcribe_batch": (I, [vp, vp, vp, I, vp, I] + [vp] * 4 + [I, vp, vp]),
    "sonic_stage_pcm": (I, [vp, vp, vp, I]),
    "sonic_run_staged": (I, [vp, vp, I, vp, vp, vp, I]),
    "sonic_fetch_tokens": (I, [vp, vp, I, vp, vp]),
    "sonic_get_timings": (I, [vp, C.POINTER(SonicTimings)]),
    "sonic_synchronize": (I, [vp]),
    "sonic_test_gemm": (I, [vp] * 6 + [I] * 4),
    "sonic_test_skinny": (I, [vp] * 4 + [I, I, I]),
    "sonic_test_attention": (I, [vp] * 5 + [I] * 7),
    "sonic_test_decode_attention": (I, [vp] * 5 + [I] * 4),
    "sonic_test_layernorm": (I, [vp] * 5 + [I, I, F, I]),
    "sonic_bench_gemm": (I, [vp] + [I] * 5 + [fp]),
    "sonic_bench_skinny": (I, [vp] + [I] * 5 + [fp]),
    "sonic_set_option": (I, [vp, S, I]),
    "sonic_debug_read": (I, [vp, S, I, vp, I64]),
    "sonic_debug_ktrace": (I, [vp, vp, I64]),
    "sonic_test_skinny_gu": (I, [vp] * 4 + [I, I, I]),
    "sonic_set_forced_ids": (I, [vp, vp, I, I]),
    "sonic_test_greedy": (I, [vp, vp] + [I] * 4 + [vp, vp]),
    "sonic_test_linear_int8": (I, [vp] * 6 + [I] * 5),
    "sonic_test_decode_attention_cache": (I, [vp, vp, vp, I, I] + [vp] * 7 + [I] * 4),
    "sonic_test_prefill_attention": (I, [vp] * 8 + [I] * 5),
    "sonic_ring_create": (I, [vp, I64, vpp]),
    "sonic_ring_destroy": (None, [vp]),
    "sonic_ring_append": (I, [vp, vp, I64, i64p]),
    "sonic_ring_head": (I64, [vp]),
    "sonic_transcribe_mixed": (I, [vp] * 6 + [I, vp, I] + [vp] * 4 + [I, vp, vp]),
    "sonic_stage_mixed": (I, [vp] * 6 + [I, vp, I]),
    "sonic_ring_create_rate": (I, [vp, I64, I, vpp]),
    "sonic_ring_flush": (I, [vp]),
    "sonic_ring_read": (I, [vp, I64, I64, vp]),
    "sonic_resample": (I, [vp, vp, vp, I64, I, I, vp, I64, i64p]),
    "sonic_prefill": (I, [vp, vp, I, vp, vp, vp, I]),
    "sonic_decode_step": (I, [vp, I, ip, ip]),
    "sonic_device_info": (I, [I, S, I, i64p, i64p, ip]),
    "sonic_memory_info": (I, [vp, i64p, i64p]),
    "sonic_abi_version": (I, []),
    "sonic_slot_create": (I, [vp, vpp]),
    "sonic_slot_count": (I, [vp]),
    "sonic_run_staged_async": (I, [vp, vp, I, vp, vp, vp, I]),
    "sonic_wait": (I, [vp, I, ip]),
    "sonic_service_begin": (I, [vp]),
    "sonic_service_end": (I, [vp]),
    "sonic_splice_rows": (I, [vp, vp, I, vp, vp, i64p]),
    "sonic_service_step": (I, [vp, I, I, vp, vp, i64p, ip]),
    "sonic_fetch_row": (I, [vp, I, I, vp]),
    "sonic_fetch_rows": (I, [vp, I, vp, vp, vp, I]),
    "sonic_prefill_enqueue": (I, [vp, vp, I, vp, vp, vp]),
    "sonic_runtime_info": (I, [I, ip, ip, ip]),
    "sonic_engine_info": (I, [vp] + [ip] * 4 + [vpp]),
    "sonic_dispatch_create": (I, [vp, I, vp, I, I, vpp]),
    "sonic_dispatch_submit": (I, [vp, C.POINTER(DispatchRequest), i64p]),
    "sonic_dispatch_cancel": (I, [vp, I64]),
    "sonic_dispatch_next": (I, [vp, I, i64p, ip, vp, I, ip, S, I]),
    "sonic_dispatch_stats": (I, [vp, i64p, i64p, ip, ip]),
    "sonic_dispatch_close": (I, [vp]),
    "sonic_dispatch_destroy": (I, [vp]),
    "sonic_pipeline_create": (I, [vp, I, vp, I, I, I, vpp]),
    "sonic_pipeline_submit": (I, [vp, vp, vp, I, vp, I] + [vp] * 4 + [I, vp, i64p]),
    "sonic_pipeline_submit_mixed": (I, [vp] * 6 + [I, vp, I] + [vp] * 4 + [I, vp, i64p]),
    "sonic_pipeline_wait": (I, [vp, I64]),
    "sonic_pipeline_stats": (I, [vp, i64p, i64p, ip]),
    "sonic_pipeline_last_error": (S, [vp]),
    "sonic_pipeline_destroy": (I, [vp]),
    "sonic_vad_create": (I, [I, I, vpp]),
    "sonic_vad_destroy": (None, [vp]),
    "sonic_vad_last_error": (S, [vp]),
    "sonic_vad_load_tensor": (I, [vp, S, vp, i64p, I]),
    "sonic_vad_probs": (I, [vp] * 4 + [I, vp]),
    "sonic_vad_probs_rings": (I, [vp] * 6 + [I, vp]),
    "sonic_fetch_logprobs": (I, [vp, vp, I]),
    "sonic_fetch_rows_lp": (I, [vp, I, vp, vp, vp, I, vp]),
    "sonic_dispatch_next_lp": (I, [vp, I, i64p, ip, vp, I, ip, S, I, vp]),
    "sonic_pipeline_submit_lp": (I, [vp] * 6 + [I, vp, I] + [vp] * 4 + [I, vp, vp, i64p]),
    "sonic_test_greedy_lp": (I, [vp, vp] + [I] * 4 + [vp] * 4),
    "sonic_set_generation": (I, [vp, F, I, vp, I]),
    "sonic_get_generation": (I, [vp, fp, ip, vp, I, ip]),
    "sonic_test_greedy_guard": (I, [vp, vp] + [I] * 4 + [vp, I, vp, F, I, vp, I] + [vp] * 4),
    "sonic_test_add_rmsnorm": (I, [vp, vp, vp, I, I, vp, F, vp, I, I, I] + [vp] * 5),
    "sonic_test_quant_rows": (I, [vp, vp, I, I, I] + [vp] * 5),
    "sonic_test_swiglu_slab": (I, [vp, vp] + [I] * 5 + [vp]),
    "sonic_test_decode_o_gu": (I, [vp] * 5 + [F, vp] + [I] * 6 + [vp, vp, vp]),
    "sonic_test_rope_append": (I, [vp] * 7 + [I] * 7 + [vp] * 4),
    "sonic_test_rope_enc": (I, [vp, vp] + [I] * 6 + [vp]),
    "sonic_set_request_bias": (I, [vp] * 5 + [I]),
    "sonic_test_greedy_bias": (I, [vp, vp] + [I] * 4 + [vp, I, vp, F, I, vp, I] + [vp] * 8),
    "sonic_set_request_sampling": (I, [vp, vp, vp, I]),
    "sonic_test_greedy_sample": (I, [vp, vp] + [I] * 4 + [vp, I, vp, F, I, vp, I] + [vp] * 12),
    "sonic_test_decode_i8_norm": (I, [vp] * 5 + [F] + [vp] * 3 + [I] * 6 + [vp] * 7),
    "sonic_test_decode_i8_swiglu": (I, [vp] * 4 + [I] * 5 + [vp] * 7),
    "sonic_test_decode_i8_attn": (I, [vp] * 12 + [I] * 6 + [vp] * 2),
}
del I, F, I64, U64, S, vp, ip, i64p, fp, vpp
EXPORTS = list(SIGNATURES)


def make_dims(d: ModelDims) -> SonicDims:
    x = SonicDims()
    x.n_mels, x.n_frames, x.enc_T = d.n_mels, d.n_frames, d.enc_T
    x.enc_d, x.enc_ff, x.enc_layers, x.enc_heads, x.enc_rotary_dim = d.enc_d, d.enc_ff, d.enc_layers, d.enc_heads, d.enc_rotary_dim
    x.enc_theta, x.enc_ln_eps, x.merge = d.enc_rope_theta, d.enc_ln_eps, d.merge
    x.dec_d, x.dec_ff, x.dec_layers, x.dec_heads, x.dec_kv_heads, x.dec_head_dim = d.dec_d, d.dec_ff, d.dec_layers, d.dec_heads, d.dec_kv_heads, d.dec_head_dim
    x.dec_theta, x.dec_rms_eps = d.dec_rope_theta, d.dec_rms_eps
    x.vocab, x.audio_token_id, x.n_eos = d.vocab, d.audio_token_id, len(d.eos_ids)
    for i, e in enumerate(d.eos_ids):
        x.eos[i] = e
    return x


_lib = None


def load_library():
    """Load libsonic_hip.so; raise RuntimeError (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"sonicscribe_amd: HIP extension not built ({LIB_PATH} missing). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C sonicscribe_amd/csrc`. There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    if lib.sonic_abi_version() != ABI_VERSION:
        raise RuntimeError(f"sonicscribe_amd: {LIB_PATH} has ABI version {lib.sonic_abi_version()}, this binding expects {ABI_VERSION}: rebuild the library")
    _lib = lib
    return lib


class SonicError(RuntimeError):
    pass


class RingSlice:
    """Samples [start, start + n) of a device ring: a decode window that never visits the host."""
    __slots__ = ("ring", "start", "n")

    def __init__(self, ring: "Ring", start: int, n: int):
        self.ring, self.start, self.n = ring, int(start), int(n)

    def __len__(self):
        return self.n


class Ring:
    """PCM (int16, 16 kHz) of one streaming session or one file in HBM (sonic_ring_*).  With `rate` other than 16000 the appends take
    samples at that rate and the device resampler (csrc/resample.hip) writes the ring: content, indices, `head` and every reader stay in
    16 kHz samples (sonic_ring_create_rate)."""

    def __init__(self, engine: "Engine", capacity_samples: int, rate: int = 16000):
        self.engine, self.capacity, self.rate = engine, int(capacity_samples), int(rate)
        h = C.c_void_p()
        if self.rate == 16000:
            engine._check(engine.lib.sonic_ring_create(engine.h, self.capacity, C.byref(h)))
        else:
            from . import frontend
            frontend.resample_geometry(self.rate, 16000)          # ValueError for a rate the library refuses
            engine._check(engine.lib.sonic_ring_create_rate(engine.h, self.capacity, self.rate, C.byref(h)))
        self.h = h
        if not hasattr(engine, "_rings"):
            engine._rings = []
        engine._rings.append(self)

    def _fail(self, what: str, rc: int):
        raise RuntimeError(f"{what} failed with status {rc}: " + (self.engine.lib.sonic_last_error(None) or b"").decode())

    def append(self, pcm) -> int:
        """pcm: bytes (little-endian int16, as on the wire) or an int16 array, at the ring's rate.  Returns the ring's head before the
        call: the absolute index of the first sample this chunk put into the ring (a rate ring: `head` afterwards tells how many)."""
        a = np.frombuffer(pcm, dtype=np.int16) if isinstance(pcm, (bytes, bytearray, memoryview)) else np.ascontiguousarray(pcm, dtype=np.int16)
        first = C.c_int64(0)
        rc = self.engine.lib.sonic_ring_append(self.h, _p(a) if a.size else None, a.size, C.byref(first))
        if rc != 0:
            self._fail("sonic_ring_append", rc)
        return int(first.value)

    def flush(self) -> None:
        """End the stream of a rate ring: the remaining outputs, up to ceil(n * 16000 / rate) in all, with zeros beyond the last sample;
        the next append starts a new stream.  Nothing to do on a 16 kHz ring."""
        rc = self.engine.lib.sonic_ring_flush(self.h)
        if rc != 0:
            self._fail("sonic_ring_flush", rc)

    def read(self, first: int, n: int) -> np.ndarray:
        """int16 ring samples [first, first + n), behind every append so far (sonic_ring_read; the reference's debug WAV dump)."""
        out = np.empty(int(n), np.int16)
        rc = self.engine.lib.sonic_ring_read(self.h, int(first), int(n), _p(out) if out.size else None)
        if rc != 0:
            self._fail("sonic_ring_read", rc)
        return out

    @property
    def head(self) -> int:
        return int(self.engine.lib.sonic_ring_head(self.h))

    def slice(self, start: int, n: int) -> RingSlice:
        return RingSlice(self, start, n)

    def close(self):
        if getattr(self, "h", None):
            self.engine.lib.sonic_ring_destroy(self.h)
            self.h = None
            if self in getattr(self.engine, "_rings", []):
                self.engine._rings.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_GRAMMAR_IDS = threading.Lock()


def grammar_words(grammar) -> np.ndarray:
    """a grammar.Grammar as the int32 words the library takes (include/sonic_hip.h): N | E | node_off | edge_tok | edge_next"""
    return np.ascontiguousarray(np.concatenate([[grammar.n_nodes, grammar.n_edges], grammar.node_off, grammar.edge_tok, grammar.edge_next]), dtype=np.int32)


class DeviceGrammar:
    """A grammar.Grammar on the device (sonic_load_tensor "grammar:<id>"): lives on a weight owner under `id`, serves every handle of it and any number of requests;
    `grammar` is the host automaton it was made from.  close() raises SonicError while a staged or running request refers to it; the owner's close() takes what is left."""

    def __init__(self, engine: "Engine", grammar):
        root = engine.root
        self.engine, self.grammar = root, grammar
        words = grammar_words(grammar)
        with _GRAMMAR_IDS:                                   # (two threads compiling at once must not pick the same id)
            if not hasattr(root, "_grammars"):
                root._grammars = []
            used = {g.id for g in root._grammars}
            self.id = next(i for i in range(1, 65536) if i not in used)
            self._load(words)
            self.h = self.id
            root._grammars.append(self)

    def _load(self, words: np.ndarray):
        shape = (C.c_int64 * 1)(len(words))
        w = words if len(words) else np.zeros(1, np.int32)
        rc = self.engine.lib.sonic_load_tensor(self.engine.h, f"grammar:{self.id}".encode(), _p(w), DTYPE_I32, shape, 1)
        if rc != 0:
            raise SonicError((self.engine.lib.sonic_last_error(None) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            with _GRAMMAR_IDS:
                if getattr(self.engine, "h", None):
                    self._load(np.zeros(0, np.int32))        # shape {0}: destroy
                self.h = None
                if self in getattr(self.engine, "_grammars", []):
                    self.engine._grammars.remove(self)


class DeviceLM:
    """An ngram.NGramLM on the device (sonic_load_tensor "lm:<id>"): lives on a weight owner under `id` and serves every handle of it whose option lm
    names it; `lm` is the host automaton it was made from.  close() raises SonicError while a handle's option refers to it; the owner's close() takes what is left."""

    def __init__(self, engine: "Engine", lm):
        root = engine.root
        self.engine, self.lm = root, lm
        words = np.ascontiguousarray(lm.pack(), dtype=np.int32)
        with _GRAMMAR_IDS:
            if not hasattr(root, "_lms"):
                root._lms = []
            used = {m.id for m in root._lms}
            self.id = next(i for i in range(1, 65536) if i not in used)
            self._load(words)
            self.h = self.id
            root._lms.append(self)

    def _load(self, words: np.ndarray):
        shape = (C.c_int64 * 1)(len(words))
        w = words if len(words) else np.zeros(1, np.int32)
        rc = self.engine.lib.sonic_load_tensor(self.engine.h, f"lm:{self.id}".encode(), _p(w), DTYPE_I32, shape, 1)
        if rc != 0:
            raise SonicError((self.engine.lib.sonic_last_error(None) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            with _GRAMMAR_IDS:
                if getattr(self.engine, "h", None):
                    self._load(np.zeros(0, np.int32))        # shape {0}: destroy
                self.h = None
                if self in getattr(self.engine, "_lms", []):
                    self.engine._lms.remove(self)


def weight_bits(weight: float) -> int:
    """an fp32 weight as the int32 option lm_weight carries"""
    return int(np.array([weight], np.float32).view(np.int32)[0])


class TokenScores(NamedTuple):
    """A request's log-probabilities on a handle with option top_logprobs = K > 0: `lp` [n] float32 (the emitted tokens'), `top_logprobs` [n, K] float32 and
    `top_ids` [n, K] int32 - at every step the K best ids by (score descending, id ascending) among the ids with a finite score, with their log-probabilities;
    places beyond the finite scores hold (-inf, -1)."""
    lp: np.ndarray
    top_logprobs: np.ndarray
    top_ids: np.ndarray


class AlignedScores(NamedTuple):
    """TokenScores of an align run (option forced_align): the same three members (`top_logprobs` / `top_ids` are [n, 0] on a handle without
    top_logprobs) and `times` [n] int32 - t_n, the index into the request's audio-token run at which token n starts (one audio token = 80 ms)."""
    lp: np.ndarray
    top_logprobs: np.ndarray
    top_ids: np.ndarray
    times: np.ndarray


def unpack_logprobs(rec, n: int, K: int, align: bool = False):
    """The first n records of a wide log-probability array (include/sonic_hip.h, option top_logprobs: 1 + 2K floats per token - the emitted token's
    log-probability, the K alternatives', their ids as fp32) -> (lp [n], top_lp [n, K] float32, top_ids [n, K] int32).  K = 0: the records are the
    log-probabilities themselves, and the result is that float32 array alone - what the wrappers returned before the option existed.  align: the records are an
    align run's, one float wider (t_n last), and the result is an AlignedScores."""
    W = 1 + 2 * int(K) + (1 if align else 0)
    r = np.asarray(rec, np.float32).reshape(-1)[: int(n) * W].reshape(int(n), W)
    if align:        # an align run's records: W = 1 + 2K + 1, the last float is t_n (an index below 2^24: exact in fp32)
        return AlignedScores(r[:, 0].copy(), r[:, 1:1 + K].copy(), r[:, 1 + K:1 + 2 * K].astype(np.int32), r[:, W - 1].astype(np.int32))
    if K == 0:
        return r[:, 0].copy()
    return TokenScores(r[:, 0].copy(), r[:, 1:1 + K].copy(), r[:, 1 + K:].astype(np.int32))


# The options a handle mirrors as attributes of the same name, with their type: set_option keeps them current, a slot created from now on copies them (in the
# library and here).  top_logprobs is the width of every log-probability record the handle returns; forced_parallel and forced_align may also be set on a slot alone;
# the last four admit the per-request values of reqvalues.VALUES.
MIRRORED_OPTIONS = {"token_logprobs": bool, "top_logprobs": int, "forced_parallel": bool, "forced_align": bool, **{v.option: bool for v in reqvalues.VALUES}}


def copy_mirrored_options(src, dst) -> None:
    """the mirrored options of `src` onto the slot `dst`, as sonic_slot_create copies them: top_logprobs is 0 on a slot whose token_logprobs is off"""
    for name, kind in MIRRORED_OPTIONS.items():
        setattr(dst, name, kind(getattr(src, name, 0)))
    if not dst.token_logprobs:
        dst.top_logprobs = 0


class Engine(HooksMixin):
    """One model replica on one MI355X."""

    def __init__(self, dims: ModelDims, device_id: int = 0, mode: int = MODE_NATIVE, max_batch: int = 32, max_ctx: int = 1024, _slot_of: Optional["Engine"] = None):
        self.lib = load_library()
        self.dims = dims
        self.max_batch, self.max_ctx = max_batch, max_ctx
        self.mode = _slot_of.mode if _slot_of is not None else mode
        self._cd = make_dims(dims)
        self.owner: Optional["Engine"] = _slot_of       # a slot keeps its weight owner alive
        self._slots: List["Engine"] = []
        h = C.c_void_p()
        if _slot_of is not None:
            rc = self.lib.sonic_slot_create(_slot_of.h, C.byref(h))
        else:
            rc = self.lib.sonic_create(C.byref(self._cd), device_id, mode, max_batch, max_ctx, C.byref(h))
        if rc != 0:
            msg = (self.lib.sonic_last_error(None) or b"").decode()
            if rc == SONIC_ERR_UNSUPPORTED:
                raise ImportError(msg)
            raise (ValueError if "mode must be" in msg else SonicError)(msg)
        self.h = h

    @property
    def root(self) -> "Engine":
        return self.owner if self.owner is not None else self

    def slot(self) -> "Engine":
        """Another batch in flight on this engine's weights (sonic_slot_create): an Engine of its own in every respect - stream, buffers,
        KV cache, graphs, lock - that shares the owner's weight allocations.  Closed with its owner at the latest."""
        root = self.root
        s = Engine(self.dims, 0, 0, self.max_batch, self.max_ctx, _slot_of=root)
        copy_mirrored_options(root, s)
        root._slots.append(s)
        return s

    @property
    def tok_cap(self) -> int:
        """tokens one prefill of this handle holds (the library's tok_cap: max_batch x min(max_ctx, audio rows of a window + 256))"""
        return self.max_batch * min(self.max_ctx, self.dims.max_audio_tokens + 256)

    def slot_count(self) -> int:
        return int(self.lib.sonic_slot_count(self.h))

    def info(self) -> dict:
        """sonic_engine_info: what the library says about this handle (row / context capacity, mode, device, identity of its weight copy)."""
        v = [C.c_int32() for _ in range(4)]
        w = C.c_void_p()
        self._check(self.lib.sonic_engine_info(self.h, *[C.byref(x) for x in v], C.byref(w)))
        return {"max_batch": v[0].value, "max_ctx": v[1].value, "mode": v[2].value, "device": v[3].value, "weights_id": w.value}

    # -- plumbing
    def _check(self, rc: int):
        if rc != 0:
            msg = (self.lib.sonic_last_error(self.h) or b"").decode()
            if rc == SONIC_ERR_MISMATCH:
                raise ValueError(msg)
            raise SonicError(msg)

    def close(self):
        if getattr(self, "h", None):
            for s in list(self._slots):                      # slots read this engine's weights: they go first
                s.close()
            for r in list(getattr(self, "_rings", ())):      # rings belong to their engine and go first
                r.close()
            for g in list(getattr(self, "_grammars", ())):   # the library frees the grammars with their owner: the handles die here
                g.h = None
            self._grammars = []
            for m in list(getattr(self, "_lms", ())):        # ... and the language models likewise
                m.h = None
            self._lms = []
            self.lib.sonic_destroy(self.h)
            self.h = None
            if self.owner is not None and self in self.owner._slots:
                self.owner._slots.remove(self)

    def ring_create(self, capacity_samples: int, rate: int = 16000) -> "Ring":
        """Device-resident PCM ring of one streaming session (include/sonic_hip.h sonic_ring_*).  capacity_samples counts
        16 kHz samples; `rate` is the rate of the samples the appends bring (resampled on the device when it is not 16000)."""
        return Ring(self, capacity_samples, rate)

    def grammar_create(self, grammar) -> "DeviceGrammar":
        """a grammar.Grammar onto this engine's weight owner (sonic_load_tensor "grammar:<id>"): one handle for every slot and every request"""
        return DeviceGrammar(self, grammar)

    def lm_create(self, lm) -> "DeviceLM":
        """an ngram.NGramLM onto this engine's weight owner (sonic_load_tensor "lm:<id>"): one handle for every slot"""
        return DeviceLM(self, lm)

    def set_lm(self, lm: Optional["DeviceLM"], weight: float = 0.0):
        """Shallow fusion on this handle (options lm_weight / lm): every decode of it adds weight x the model's log-probabilities to its scores.  None: off.
        On the owner before its slots are created (they copy both).  Needs option token_logprobs (SonicError naming it otherwise)."""
        if lm is None:
            self.set_option("lm", 0)
            return
        if lm.h is None:
            raise SonicError("lm: the language model has been closed")
        self.set_option("lm_weight", weight_bits(weight))
        self.set_option("lm", lm.id)

    def set_request_grammar(self, grammars):
        """The grammars of the requests of the NEXT prefill / run on this handle (options request_grammar_begin / request_grammar), one DeviceGrammar or None (a free
        request) per request; that call consumes them.  Needs option grammar (SonicError naming it otherwise)."""
        gs = list(grammars)
        self._check(self.lib.sonic_set_option(self.h, b"request_grammar_begin", len(gs)))
        for r, g in enumerate(gs):
            if g is not None:
                if g.h is None:
                    raise SonicError("request_grammar: the grammar has been closed")
                if g.engine is not self.root:         # (ids are per weight owner: another owner's id would name one of this owner's grammars)
                    raise SonicError("request_grammar: the grammar lives on another weight owner (a grammar serves the engine it was created on and its slots)")
                self._check(self.lib.sonic_set_option(self.h, b"request_grammar", (r << 16) | int(g.id)))

    def resample(self, x, in_rate: int, out_rate: int = 16000) -> np.ndarray:
        """torchaudio.transforms.Resample(in_rate, out_rate)(x) on the device (sonic_resample; asr.py:255-261): x is int16 PCM (taken as
        s / 32768) or float samples, mono; returns fp32 [ceil(n * out_rate / in_rate)].  Does not wait for a decoding batch."""
        from . import frontend
        a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        if a.ndim == 2 and a.shape[0] == 1:
            a = a[0]
        if a.ndim != 1:
            raise ValueError(f"resample takes mono audio ([N] or [1, N]), got shape {tuple(a.shape)}")
        frontend.resample_geometry(in_rate, out_rate)
        a = np.ascontiguousarray(a) if a.dtype == np.int16 else np.ascontiguousarray(a, dtype=np.float32)
        i16, f32 = (_p(a), None) if a.dtype == np.int16 else (None, _p(a))
        n_out = C.c_int64(0)
        rc = self.lib.sonic_resample(self.h, i16, f32, a.size, int(in_rate), int(out_rate), None, 0, C.byref(n_out))
        out = np.empty(int(n_out.value), np.float32)
        if rc == 0 and out.size:
            rc = self.lib.sonic_resample(self.h, i16, f32, a.size, int(in_rate), int(out_rate), _p(out), out.size, C.byref(n_out))
        if rc != 0:
            raise SonicError((self.lib.sonic_last_error(None) or b"").decode())
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights
    def load_tensor(self, name: str, arr: np.ndarray, bf16_bits: bool = False):
        arr = np.ascontiguousarray(arr)
        shape = (C.c_int64 * arr.ndim)(*arr.shape)
        if bf16_bits:
            assert arr.dtype == np.uint16
            dt = DTYPE_BF16
        else:
            arr = arr.astype(np.float32, copy=False)
            dt = DTYPE_F32
        self._check(self.lib.sonic_load_tensor(self.h, name.encode(), _p(arr), dt, shape, arr.ndim))

    def load_state_dict(self, state: Dict[str, np.ndarray]):
        for k, v in state.items():
            self.load_tensor(k, v)
        self.finalize()

    def load_synthetic(self, seed: int):
        self._check(self.lib.sonic_load_synthetic(self.h, seed))
        self.finalize()

    def finalize(self):
        self._check(self.lib.sonic_finalize_weights(self.h))

    def weight_bytes(self) -> int:
        return int(self.lib.sonic_weight_bytes(self.h))

    def fp8_info(self) -> Dict[str, int]:
        """mode fp8 (option fp8_weights), over sonic_debug_read: the token steps this handle built in the fp8 form since the option was set, the
        number of snapped matrices (index m of fp8_scales / fp8_matrix: layer * 4 + {0 q|k|v, 1 o_proj, 2 gate/up, 3 down_proj}, the last one the lm_head) and what
        their e4m3 copies and scales add to the owner's weight bytes.  SonicError on a handle without the option."""
        from . import fp8
        self.debug_read("fp8_scales", (1,), 0)      # (the library refuses this read by the option's name where it is off)
        return {"step_builds": int(self.debug_read("fp8_step_builds", (1,))[0]),
                "matrices": 4 * self.dims.dec_layers + 1, "extra_weight_bytes": fp8.extra_weight_bytes(self.dims)}

    def fp8_scales(self, m: int, n: int) -> np.ndarray:
        """the first n row scales of snapped matrix m, in the row order of its tiled copy"""
        return self.debug_read("fp8_scales", (n,), m)

    def fp8_matrix(self, m: int, rows: int, K: int) -> np.ndarray:
        """the first `rows` rows [rows][K] of snapped matrix m's e4m3 copy as fp32 scale * code, in the row order of its tiled copy"""
        return self.debug_read("fp8_matrix", (rows, K), m)

    # -- stages
    @staticmethod
    def _pack_pcm(segments: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        offs = np.zeros(len(segments) + 1, np.int64)
        for i, s in enumerate(segments):
            offs[i + 1] = offs[i] + len(s)
        pcm = np.concatenate([np.ascontiguousarray(s, dtype=np.int16) for s in segments]) if segments else np.zeros(0, np.int16)
        if pcm.size == 0:
            pcm = np.zeros(1, np.int16)
        return np.ascontiguousarray(pcm), offs

    def logmel(self, segments: Sequence[np.ndarray]):
        d = self.dims
        pcm, offs = self._pack_pcm(segments)
        B = len(segments)
        feats = np.empty((B, d.n_mels, d.n_frames), np.float32)
        mask = np.empty((B, d.n_frames), np.int32)
        self._check(self.lib.sonic_logmel(self.h, _p(pcm), _p(offs), B, _p(feats), _p(mask)))
        return feats, mask

    def encode(self, feats: np.ndarray, n_valid_frames: Sequence[int], want_layers: bool = False, want_enc_out: bool = False):
        d = self.dims
        feats = np.ascontiguousarray(feats, dtype=np.float32)
        B = feats.shape[0]
        nv = np.ascontiguousarray(n_valid_frames, dtype=np.int32)
        emb = np.empty((B, d.max_audio_tokens, d.dec_d), np.float32)
        n_audio = np.empty(B, np.int32)
        layers = np.empty((B, d.enc_layers, d.enc_T, d.enc_d), np.float32) if want_layers else None
        enc_out = np.empty((B, d.enc_T, d.enc_d), np.float32) if want_enc_out else None
        self._check(self.lib.sonic_encode(self.h, _p(feats), _p(nv), B, _p(emb), _p(n_audio), _p(layers), _p(enc_out)))
        return emb, n_audio, layers, enc_out

    # -- the hot call
    @staticmethod
    def _pack_prompts(prompts: Sequence[Sequence[int]]):
        offs = np.zeros(len(prompts) + 1, np.int64)
        for i, p in enumerate(prompts):
            offs[i + 1] = offs[i] + len(p)
        ids = np.concatenate([np.asarray(p, np.int32) for p in prompts]).astype(np.int32)
        return np.ascontiguousarray(ids), offs

    def _pack_mixed(self, segments):
        """Windows that are RingSlice objects stay on the device; the rest is packed like _pack_pcm (ring windows: empty host ranges)."""
        W = len(segments)
        host = [np.zeros(0, np.int16) if isinstance(s, RingSlice) else s for s in segments]
        pcm, offs = self._pack_pcm(host)
        rings = (C.c_void_p * W)(*[s.ring.h if isinstance(s, RingSlice) else None for s in segments])
        start = np.array([s.start if isinstance(s, RingSlice) else 0 for s in segments], np.int64)
        n = np.array([s.n if isinstance(s, RingSlice) else 0 for s in segments], np.int32)
        for s in segments:
            if isinstance(s, RingSlice) and s.ring.engine.root is not self.root:
                raise ValueError("a ring slice can only be decoded by the engine that owns the ring (or by a slot of it)")
        return pcm, offs, rings, start, n

    def transcribe_batch(self, segments: Sequence[Any], prompts: Sequence[Sequence[int]], max_new: Sequence[int],
                         req_win: Optional[Sequence[int]] = None, want_logits: bool = False, want_logprobs: bool = False, request_bias=None, request_sampling=None,
                         request_grammar=None, request_draft=None, forks=None):
        """segments: int16 PCM windows (<= 30 s each, already peak-normalised) or RingSlice objects (raw wire PCM resident in a device
        ring; normalised on the device over the windows of their request); one prompt per request. Returns (ids list, logits or None);
        with want_logprobs (option token_logprobs on this handle) one more element: the float32 log-probability of every returned token, per request.
        request_bias: one reqbias.RequestBias or None per request (option request_bias on this handle; set_request_bias).
        request_sampling: one (temperature, seed) or None (greedy) per request (option sampling on this handle; set_request_sampling).
        request_grammar: one DeviceGrammar or None (free) per request (option grammar on this handle; set_request_grammar).
        request_draft: one id sequence or None (no draft) per request (option draft_verify on this handle; set_request_draft).
        forks: one count n_a >= 1 per request (row forks): request a becomes n_a rows that share its encoder pass and prefill and decode on their
        own.  The four keywords above then take one value per ROW and the results have one entry per row, in the order of fork_rows(forks)."""
        samp = None if request_sampling is None else pack_request_sampling(request_sampling)      # (validated before anything is armed)
        draft = None if request_draft is None else pack_request_draft(request_draft)
        counts = None if forks is None else self._check_forks(forks, len(prompts), request_bias, samp, request_grammar, request_draft)
        if any(isinstance(s, RingSlice) for s in segments):      # the two forms differ in how the audio is packed and in the entry point that takes it
            pcm, offs, rings, start, n = self._pack_mixed(segments)
            entry, audio = self.lib.sonic_transcribe_mixed, (_p(pcm), _p(offs), rings, _p(start), _p(n))
        else:
            pcm, offs = self._pack_pcm(segments)
            entry, audio = self.lib.sonic_transcribe_batch, (_p(pcm), _p(offs))
        ids, poffs = self._pack_prompts(prompts)
        A = len(prompts)
        R = A if counts is None else int(counts.sum())      # the rows of the run: what the library writes results for
        mn = np.ascontiguousarray(max_new, dtype=np.int32)
        out_ld = int(mn.max())
        out = np.zeros((R, out_ld), np.int32)
        out_len = np.zeros(R, np.int32)
        rw = _arr(req_win, np.int32)
        logits = np.zeros((out_ld, R, self.dims.vocab), np.float32) if want_logits else None
        self._arm_requests(request_bias, samp, request_grammar, draft, counts)
        self._check(entry(self.h, *audio, len(segments), _p(rw), A, _p(ids), _p(poffs), _p(mn), _p(out), out_ld, _p(out_len), _p(logits)))
        res = [out[r, : out_len[r]].copy() for r in range(R)]
        return (res, logits, self._fetch_logprobs(out_len, out_ld)) if want_logprobs else (res, logits)

    @staticmethod
    def fork_rows(forks) -> List[List[int]]:
        """The row order of a forked run, stated once: per request the rows of its forks.  Fork 0 of request a is row a; the further forks follow
        behind the A requests, request by request: fork_rows([3, 1, 2]) == [[0, 3, 4], [1], [2, 5]]."""
        counts = [int(n) for n in forks]
        rows, nxt = [], len(counts)
        for a, n in enumerate(counts):
            rows.append([a] + list(range(nxt, nxt + n - 1)))
            nxt += max(n, 1) - 1
        return rows

    def _check_forks(self, forks, A: int, bias, samp_packed, grammar, draft):
        """the fork counts of a call as the int32 array the library takes, validated against the call's requests and per-row lists (ValueError naming `forks`)"""
        counts = [int(n) for n in forks]
        if len(counts) != A:
            raise ValueError(f"forks: {len(counts)} counts for {A} requests")
        if any(n < 1 for n in counts):
            raise ValueError("forks: every count is at least 1 (the request itself)")
        rows = sum(counts)
        if rows > int(getattr(self, "max_batch", 64)):
            raise ValueError(f"forks: the counts add up to {rows} rows, the handle has {getattr(self, 'max_batch', 64)} (max_batch)")
        if draft is not None:
            raise ValueError("forks: a forked run takes no drafts (request_draft)")
        lists = (("request_bias", bias), ("request_sampling", None if samp_packed is None else samp_packed[0]), ("request_grammar", grammar))
        for name, values in lists:
            if values is not None and len(values) != rows:
                raise ValueError(f"forks: {name} states {len(values)} values, the forked run has {rows} rows (one value per row, in the order of fork_rows)")
        return np.ascontiguousarray(counts, dtype=np.int32)

    def _arm_forks(self, counts):
        self._check(self.lib.sonic_load_tensor(self.h, b"request_forks", _p(counts), DTYPE_I32, (C.c_int64 * 1)(len(counts)), 1))

    def _arm_requests(self, bias, samp_packed, grammar, draft_packed, fork_counts=None):
        """The per-request values of the next prefill / run on this handle, None for a value the caller does not state: the call right ahead of the library call
        that consumes them, on success or failure - nothing in between can raise.  In the order of reqvalues.VALUES; the sampling values and the drafts come packed
        (pack_request_sampling, pack_request_draft: validated before anything is armed)."""
        if bias is not None:
            self.set_request_bias(bias)
        if samp_packed is not None:
            self._arm_sampling(samp_packed)
        if grammar is not None:
            self.set_request_grammar(grammar)
        if draft_packed is not None:
            self._arm_draft(draft_packed)
        if fork_counts is not None:      # row forks (_check_forks): right ahead of the consuming call
            self._arm_forks(fork_counts)
        if samp_packed is not None and len(samp_packed) == 3:      # top_k / top_p / min_p of rows stated as 5-tuples (option truncation): likewise
            self._arm_truncation(samp_packed[2])

    def score_batch(self, segments: Sequence[Any], prompts: Sequence[Sequence[int]], targets, req_win: Optional[Sequence[int]] = None, fanout: int = 1,
                    want_logits: bool = False, align: bool = False, share_prompt: bool = False):
        """Score given continuations in ONE prefill pass (the parallel forced run; needs option forced_parallel on this handle).  targets: one id
        sequence per prompt, or an int array [R][ld] padded with any valid id beyond a sequence's own length when all share a length - sequence r is scored up to
        and including its first EOS id (HF's rule).  fanout = N: the R sequences are R / N audio requests with N candidates each; `segments` / `req_win` then
        describe the R / N audio requests, which go through log-mel, encoder and projector once.  No logits processor is applied: the log-probabilities are those
        of the raw model distribution at temperature 1.  Returns what transcribe_batch(..., want_logprobs=True) returns: (ids list, logits [ld][R][V] or None,
        per sequence its float32 log-probabilities - with option top_logprobs a TokenScores); the log-probabilities need option token_logprobs (None without).
        align (needs options forced_align and token_logprobs on this handle): per sequence an AlignedScores, whose `times` are t_n per token.
        share_prompt (option forced_share_prompt for this call): the N sequences of a group bring the same prompt, and it is prefilled once per group -
        the run then holds A * P + sum(L - 1) tokens where it held sum(P + L - 1).  Not on an int8 or fp32 handle, not beside forced_align (SonicError by name)."""
        if not getattr(self, "forced_parallel", False):
            raise SonicError("score_batch needs option forced_parallel on this handle (set_option('forced_parallel', 1))")
        if align and not (getattr(self, "forced_align", False) and getattr(self, "token_logprobs", False)):
            raise SonicError("score_batch(align=True) needs options forced_align and token_logprobs on this handle (set_option('forced_align', 1))")
        from .scoring import pack_targets
        forced, lens = pack_targets(targets, self.dims.eos_ids, pad_id=0)
        if len(forced) != len(prompts):
            raise ValueError(f"{len(prompts)} prompts but {len(forced)} target sequences")
        self.set_option("forced_fanout", int(fanout))
        self.set_forced_ids(forced)
        try:
            if share_prompt:
                self.set_option("forced_share_prompt", 1)
            want_lp = bool(getattr(self, "token_logprobs", False))
            self._lp_align = bool(getattr(self, "forced_align", False))      # (an align handle's parallel run returns the wide records, asked for or not)
            out = self.transcribe_batch(segments, prompts, [int(n) for n in lens], req_win=req_win, want_logits=want_logits, want_logprobs=want_lp)
        finally:
            self._lp_align = False
            self.set_forced_ids(None)
            if share_prompt:
                self.set_option("forced_share_prompt", 0)
        if want_lp and getattr(self, "forced_align", False) and not align:      # the caller asked for scores alone: what a handle without the option returns
            K = int(getattr(self, "top_logprobs", 0))
            out = (out[0], out[1], [a.lp if K == 0 else TokenScores(a.lp, a.top_logprobs, a.top_ids) for a in out[2]])
        return out if want_lp else (out[0], out[1], None)

    def _fetch_logprobs(self, out_len, out_ld: int) -> list:
        """sonic_fetch_logprobs for the batch whose token counts are out_len: one float32 array per request (entries beyond a row's count are never written);
        with option top_logprobs one TokenScores per request (unpack_logprobs)"""
        K = int(getattr(self, "top_logprobs", 0))
        al = bool(getattr(self, "_lp_align", False))
        lp = np.full((len(out_len), max(1, int(out_ld)) * (1 + 2 * K + (1 if al else 0))), np.nan, np.float32)
        self._check(self.lib.sonic_fetch_logprobs(self.h, _p(lp), lp.shape[1]))
        return [unpack_logprobs(lp[r], int(out_len[r]), K, al) for r in range(len(out_len))]

    def stage_pcm(self, segments: Sequence[Any], req_win: Optional[Sequence[int]] = None):
        if any(isinstance(s, RingSlice) for s in segments):
            pcm, offs, rings, start, n = self._pack_mixed(segments)
            rw = _arr(req_win, np.int32)
            R = len(rw) - 1 if rw is not None else len(segments)
            self._check(self.lib.sonic_stage_mixed(self.h, _p(pcm), _p(offs), rings, _p(start), _p(n), len(segments), _p(rw), R))
            return
        pcm, offs = self._pack_pcm(segments)
        self._check(self.lib.sonic_stage_pcm(self.h, _p(pcm), _p(offs), len(segments)))

    def run_staged(self, prompts: Sequence[Sequence[int]], max_new: Sequence[int], req_win: Optional[Sequence[int]] = None,
                   want_logits: bool = False):
        ids, poffs = self._pack_prompts(prompts)
        mn = np.ascontiguousarray(max_new, dtype=np.int32)
        rw = _arr(req_win, np.int32)
        self._run_cache = (ids, poffs, mn, rw)
        self._check(self.lib.sonic_run_staged(self.h, _p(rw), len(prompts), _p(ids), _p(poffs), _p(mn), int(want_logits)))

    def prefill(self, prompts: Sequence[Sequence[int]], max_new: Sequence[int], req_win: Optional[Sequence[int]] = None, want_logits: bool = False, wait: bool = True,
                request_bias=None, request_sampling=None, request_grammar=None, request_draft=None, forks=None):
        """Stage entry point: everything up to and including the first greedy token of the staged batch (sonic_prefill).  wait=False: the
        work is only queued when the call returns (sonic_prefill_enqueue; a following splice_rows orders itself behind it on the device).
        forks: as transcribe_batch's - the handle then holds sum(forks) rows, in the order of fork_rows(forks), for decode_step, fetch_tokens and splice_rows."""
        ids, poffs = self._pack_prompts(prompts)
        mn = np.ascontiguousarray(max_new, dtype=np.int32)
        rw = _arr(req_win, np.int32)
        samp = None if request_sampling is None else pack_request_sampling(request_sampling)
        draft = None if request_draft is None else pack_request_draft(request_draft)
        counts = None if forks is None else self._check_forks(forks, len(prompts), request_bias, samp, request_grammar, request_draft)
        self._arm_requests(request_bias, samp, request_grammar, draft, counts)      # (as transcribe_batch's keywords: this prefill consumes them, on success or failure)
        if not wait:
            self._check(self.lib.sonic_prefill_enqueue(self.h, _p(rw), len(prompts), _p(ids), _p(poffs), _p(mn)))
            return
        self._check(self.lib.sonic_prefill(self.h, _p(rw), len(prompts), _p(ids), _p(poffs), _p(mn), int(want_logits)))

    def decode_step(self, n_steps: int = 1):
        """Stage entry point: up to n_steps further greedy steps; returns (rows still active, steps actually run)."""
        na, done = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.sonic_decode_step(self.h, int(n_steps), C.byref(na), C.byref(done)))
        return int(na.value), int(done.value)

    def memory_info(self):
        """(allocated, reserved) bytes of this handle's live device allocations (equal: there is no caching layer under the engine)."""
        a, r = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.sonic_memory_info(self.h, C.byref(a), C.byref(r)))
        return int(a.value), int(r.value)

    def rerun_staged(self):
        """Repeat the last run_staged call without re-packing (benchmark inner loop)."""
        ids, poffs, mn, rw = self._run_cache
        self._check(self.lib.sonic_run_staged(self.h, _p(rw), len(mn), _p(ids), _p(poffs), _p(mn), 0))

    def run_staged_async(self, prompts: Optional[Sequence[Sequence[int]]] = None, max_new: Optional[Sequence[int]] = None,
                         req_win: Optional[Sequence[int]] = None):
        """sonic_run_staged_async: returns at once, a worker thread of the handle runs the batch; wait() collects its status.
        Without arguments: the arguments of the last run_staged call."""
        if prompts is not None:
            ids, poffs = self._pack_prompts(prompts)
            mn = np.ascontiguousarray(max_new, dtype=np.int32)
            rw = _arr(req_win, np.int32)
            self._run_cache = (ids, poffs, mn, rw)
        ids, poffs, mn, rw = self._run_cache
        rc = self.lib.sonic_run_staged_async(self.h, _p(rw), len(mn), _p(ids), _p(poffs), _p(mn), 0)
        if rc != 0:
            raise SonicError((self.lib.sonic_last_error(None) or b"").decode() or f"sonic_run_staged_async failed with status {rc}")

    # -- continuous decoding (sonic_service_*): this engine's rows are a pool, requests prefilled on a slot are spliced in row by row
    def service_begin(self):
        self._check(self.lib.sonic_service_begin(self.h))

    def service_end(self):
        self._check(self.lib.sonic_service_end(self.h))

    def splice_rows(self, src: "Engine", src_rows: Sequence[int], dst_rows: Sequence[int]) -> int:
        """rows src_rows of `src` (requests of its last prefill()) -> free rows dst_rows of this engine; returns the chunk sequence number
        after which service_step()'s flags describe the new occupants"""
        a = np.ascontiguousarray(src_rows, dtype=np.int32); b = np.ascontiguousarray(dst_rows, dtype=np.int32)
        seq = C.c_int64(0)
        self._check(self.lib.sonic_splice_rows(self.h, src.h, len(a), _p(a), _p(b), C.byref(seq)))
        return int(seq.value)

    def service_step(self, n_chunks: int = 1, rows: int = 0):
        """queue n_chunks more chunks over rows 0 .. rows-1 (rounded up to 16; 0 = all); returns (finished[64], n_new[64], seq, n_active) of
        the newest completed check"""
        fin = np.zeros(64, np.int32); nn = np.zeros(64, np.int32)
        seq, na = C.c_int64(0), C.c_int32(0)
        self._check(self.lib.sonic_service_step(self.h, int(n_chunks), int(rows), _p(fin), _p(nn), C.byref(seq), C.byref(na)))
        return fin, nn, int(seq.value), int(na.value)

    def fetch_row(self, row: int, n: int) -> np.ndarray:
        out = np.zeros(max(1, int(n)), np.int32)
        self._check(self.lib.sonic_fetch_row(self.h, int(row), int(n), _p(out)))
        return out[:n].copy()

    def fetch_rows(self, rows: Sequence[int], counts: Sequence[int], want_logprobs: bool = False):
        """fetch_row for several finished rows in one call (one wait, one release launch); want_logprobs: (ids list, log-probability list) from
        sonic_fetch_rows_lp (both in one call: the fetch releases the rows)"""
        r, c = np.asarray(rows, np.int32), np.asarray(counts, np.int32)
        ld = max(1, int(c.max()) if len(c) else 1)
        out = np.zeros((len(r), ld), np.int32)
        if want_logprobs:
            K = int(getattr(self, "top_logprobs", 0))
            lp = np.full((len(r), ld * (1 + 2 * K)), np.nan, np.float32)
            self._check(self.lib.sonic_fetch_rows_lp(self.h, len(r), _p(r), _p(c), _p(out), ld, _p(lp)))
            return [out[i, :int(c[i])].copy() for i in range(len(r))], [unpack_logprobs(lp[i], int(c[i]), K) for i in range(len(r))]
        self._check(self.lib.sonic_fetch_rows(self.h, len(r), _p(r), _p(c), _p(out), ld))
        return [out[i, :int(c[i])].copy() for i in range(len(r))]

    def synchronize(self):
        """block until everything queued on this handle's stream has completed (sonic_synchronize)"""
        self._check(self.lib.sonic_synchronize(self.h))

    def wait(self, block: bool = True) -> bool:
        """Collect the asynchronous run (raises its error).  block=False: returns False while it is still running."""
        busy = C.c_int32(0)
        self._check(self.lib.sonic_wait(self.h, int(block), C.byref(busy)))
        return not busy.value

    def fetch_tokens(self, R: int, out_ld: int, want_logprobs: bool = False):
        out = np.zeros((R, out_ld), np.int32)
        out_len = np.zeros(R, np.int32)
        self._check(self.lib.sonic_fetch_tokens(self.h, _p(out), out_ld, _p(out_len), None))
        res = [out[r, : out_len[r]].copy() for r in range(R)]
        return (res, self._fetch_logprobs(out_len, out_ld)) if want_logprobs else res

    def timings(self) -> Dict[str, float]:
        t = SonicTimings()
        self._check(self.lib.sonic_get_timings(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in SonicTimings._fields_}

    # -- product setters
    def set_option(self, key: str, value: int):
        self._check(self.lib.sonic_set_option(self.h, key.encode(), value))
        if key in MIRRORED_OPTIONS:
            setattr(self, key, MIRRORED_OPTIONS[key](value))

    def set_forced_ids(self, ids):
        """ids: [R][ld] int array (token n of request r) or None to clear; see sonic_set_forced_ids."""
        if ids is None:
            self._check(self.lib.sonic_set_forced_ids(self.h, None, 0, 0))
            return
        a = np.ascontiguousarray(ids, dtype=np.int32)
        assert a.ndim == 2
        self._check(self.lib.sonic_set_forced_ids(self.h, _p(a), a.shape[0], a.shape[1]))

    def set_generation(self, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, suppress_tokens: Sequence[int] = ()):
        """HF generate()'s logits processors inside the greedy kernel (sonic_set_generation): the neutral values (1.0, 0, no ids) switch them off.  On the
        owner before its slots are created (they copy it); refused (SonicError) for values out of range and while the handle has rows running."""
        sup = np.ascontiguousarray(list(suppress_tokens), dtype=np.int32)
        self._check(self.lib.sonic_set_generation(self.h, float(repetition_penalty), int(no_repeat_ngram_size), _p(sup) if sup.size else None, int(sup.size)))

    def get_generation(self) -> dict:
        """the values in force on this handle (sonic_get_generation)"""
        p, n, ns = C.c_float(0), C.c_int32(0), C.c_int32(0)
        sup = np.zeros(256, np.int32)
        self._check(self.lib.sonic_get_generation(self.h, C.byref(p), C.byref(n), _p(sup), 256, C.byref(ns)))
        return {"repetition_penalty": float(p.value), "no_repeat_ngram_size": int(n.value), "suppress_tokens": [int(x) for x in sup[:ns.value]]}

    def set_request_bias(self, tables):
        """The sequence-bias tables of the requests of the NEXT prefill / run on this handle (sonic_set_request_bias), one reqbias.RequestBias or None per request;
        that call consumes them.  Needs option request_bias (SonicError naming it otherwise); the caps were checked when the tables were built, the vocabulary is
        checked here."""
        tables = list(tables)
        seq_ids, seq_off, bias, req_off = pack_request_bias(tables)
        self._check(self.lib.sonic_set_request_bias(self.h, _p(seq_ids) if seq_ids.size else None, _p(seq_off), _p(bias) if bias.size else None, _p(req_off), len(tables)))

    def _arm_draft(self, words):
        self._check(self.lib.sonic_load_tensor(self.h, b"request_draft", _p(words), DTYPE_I32, (C.c_int64 * 1)(len(words)), 1))

    def set_request_draft(self, drafts):
        """The drafts of the requests of the NEXT prefill / run on this handle (sonic_load_tensor "request_draft"), one id sequence or None (no draft)
        per request; that call consumes them.  The engine accepts the longest prefix of a draft that the model itself would have emitted, takes the model's own token
        at the first disagreement and decodes on from there.  Needs option draft_verify (SonicError naming it otherwise); the library refuses - it never cuts - a
        draft that holds an EOS id or the audio placeholder, or more than max_new - 1 ids."""
        self._arm_draft(pack_request_draft(list(drafts)))

    def draft_accepted(self, R: int) -> np.ndarray:
        """a_r of this handle's last prefill (sonic_debug_read "draft_accepted"): how many ids of its draft each of the R requests took; tests and diagnostics"""
        out = np.zeros(max(1, int(R)), np.float32)
        self._check(self.lib.sonic_debug_read(self.h, b"draft_accepted", 0, _p(out), int(R)))
        return out[:R].astype(np.int32)

    def _arm_sampling(self, packed):
        t, s = packed[0], packed[1]
        self._check(self.lib.sonic_set_request_sampling(self.h, _p(t), _p(s), len(t)))

    def _arm_truncation(self, rows):
        self._check(self.lib.sonic_load_tensor(self.h, b"request_truncation", _p(rows), DTYPE_F32, (C.c_int64 * 2)(len(rows), 3), 2))

    def set_request_sampling(self, values):
        """The (temperature, seed) of the requests of the NEXT prefill / run on this handle (sonic_set_request_sampling), one pair or None (greedy) per request; that
        call consumes them.  Needs option sampling (SonicError naming it otherwise).  ValueError for a temperature that is neither 0 nor in [1e-3, 100].
        A request may instead state (temperature, seed, top_k, top_p, min_p) (sampling.check_truncation names a value out of range): the batch's
        rows of (top_k, top_p, min_p) then follow as sonic_load_tensor "request_truncation", which needs option truncation.  Pairs alone make today's calls."""
        packed = pack_request_sampling(list(values))
        self._arm_sampling(packed)
        if len(packed) == 3:
            self._arm_truncation(packed[2])


def pack_request_bias(tables):
    """one table per request (reqbias.RequestBias, or None for a request without one) -> sonic_set_request_bias's arrays (seq_ids, seq_off, bias, req_off)"""
    ids, lens, vals, req_off = [], [], [], [0]
    for t in tables:
        if t is not None:
            i, o, b = t.table()
            ids.append(i); lens.append(np.diff(o)); vals.append(b)
        req_off.append(req_off[-1] + (len(t) if t is not None else 0))
    seq_ids = np.ascontiguousarray(np.concatenate(ids) if ids else np.zeros(0), dtype=np.int32)
    ln = np.concatenate(lens) if lens else np.zeros(0, np.int64)
    seq_off = np.zeros(len(ln) + 1, np.int32)
    seq_off[1:] = np.cumsum(ln)
    bias = np.ascontiguousarray(np.concatenate(vals) if vals else np.zeros(0), dtype=np.float32)
    return seq_ids, seq_off, bias, np.asarray(req_off, dtype=np.int32)


def pack_request_draft(drafts):
    """one draft per request (a sequence of token ids, or None / empty for a request without one) -> the int32 words sonic_load_tensor "request_draft" takes:
    R | off[0 .. R] | ids"""
    ds = [np.zeros(0, np.int64) if d is None else np.asarray(list(d), dtype=np.int64).reshape(-1) for d in drafts]
    if not ds:
        raise ValueError("request_draft: no request")
    off = np.concatenate([[0], np.cumsum([len(d) for d in ds])])
    ids = np.concatenate(ds) if ds else np.zeros(0, np.int64)
    if ids.size and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):      # (what the ids may be is the library's to say: vocabulary, EOS ids, the audio placeholder)
        raise ValueError("request_draft: token ids must be int32 values")
    return np.ascontiguousarray(np.concatenate([[len(ds)], off, ids]), dtype=np.int32)


def pack_request_sampling(values):
    """one (temperature, seed) per request, or None for a greedy one -> sonic_set_request_sampling's arrays, validated (sampling.check_temperature / check_seed).
    When a request states (temperature, seed, top_k, top_p, min_p) a third element follows: float32 [R][3], the rows of sonic_load_tensor "request_truncation"
    (sampling.pack_truncation; a request without the three values has them off)"""
    from . import sampling
    vals = [(0.0, 0) if v is None else tuple(v) for v in values]
    for v in vals:
        if len(v) not in (2, 5):
            raise ValueError(f"request_sampling: {v!r} is neither (temperature, seed) nor (temperature, seed, top_k, top_p, min_p)")
    t, s = sampling.pack_sampling([v[0] for v in vals], [v[1] for v in vals])
    if all(len(v) == 2 for v in vals):
        return t, s
    return t, s, sampling.pack_truncation([v[2:] if len(v) == 5 else (0, 1.0, 0.0) for v in vals])


def device_info(device_id: int = 0) -> dict:
    """name / total and free memory / HIP runtime version of a device (what asr.py:501-506 reads from torch.cuda)."""
    lib = load_library()
    name = C.create_string_buffer(256)
    tot, fr, ver = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    if lib.sonic_device_info(int(device_id), name, 256, C.byref(tot), C.byref(fr), C.byref(ver)) != 0:
        raise RuntimeError((lib.sonic_last_error(None) or b"").decode())
    return {"name": name.value.decode(), "total_bytes": int(tot.value), "free_bytes": int(fr.value), "hip_runtime_version": int(ver.value)}


def runtime_info(device_id: int = 0) -> dict:
    """Hardware queues the HIP runtime of this process really has on the device (measured), GPU_MAX_HW_QUEUES as it reads now, and what an
    engine with slots wants (sonic_runtime_info)."""
    lib = load_library()
    q, env, want = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    if lib.sonic_runtime_info(int(device_id), C.byref(q), C.byref(env), C.byref(want)) != 0:
        raise RuntimeError((lib.sonic_last_error(None) or b"").decode())
    return {"hw_queues": int(q.value), "hw_queues_env": int(env.value), "hw_queues_wanted": int(want.value)}


def device_count() -> int:
    return int(load_library().sonic_device_count())
