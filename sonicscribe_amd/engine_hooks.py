"""The test, bench and debug wrappers of the binding (sonic_test_*, sonic_bench_*, sonic_debug_*): a mixin of engine.Engine, which supplies `lib`, `h` and
`_check`.  Nothing here is on the product path.  This module does not import engine (engine imports it); the two helpers both use live here."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_SWIGLU, EPI_QKV_VT = 0, 1, 2, 3, 4


class GemmForm(C.Structure):
    """sonic_gemm_form: one GEMM launch form, the words of sonic_load_tensor "gemm.form.run".  A fresh record is all-zero - the dense form of sonic_test_gemm - with `size` set"""
    _fields_ = [(n, C.c_int32) for n in (
        "size", "M", "N", "K", "epi", "lda", "ldc", "ldr", "batch", "strideA", "strideC", "c_row_offset", "w_tiled", "gu8", "resid_in_place",
        "n_split", "seg_T", "vt_ld", "rope_ncols", "group_rows", "gelu_arith")]

    def __init__(self, **kw):
        super().__init__(size=C.sizeof(GemmForm), **kw)


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _arr(x, dtype):
    """contiguous array of dtype, or None"""
    return None if x is None else np.ascontiguousarray(x, dtype)


def _quant_bufs(rows: int, K: int):
    return (np.zeros((rows, K), np.int8), np.zeros(rows, np.float32), np.zeros(rows, np.int32), np.zeros((rows, K), np.int32), np.zeros((rows, K), np.float32))


class HooksMixin:
    def test_gemm(self, A, W, bias=None, resid=None, epi=EPI_BIAS):
        A = np.ascontiguousarray(A, np.float32); W = np.ascontiguousarray(W, np.float32)
        M, K = A.shape; N = W.shape[0]
        n_out = N // 2 if epi == EPI_SWIGLU else N
        out = np.empty((M, n_out), np.float32)
        b = _arr(bias, np.float32)
        r = _arr(resid, np.float32)
        self._check(self.lib.sonic_test_gemm(self.h, _p(A), _p(W), _p(b), _p(r), _p(out), M, N, K, epi))
        return out

    def debug_gemm_route(self) -> dict:
        """sonic_debug_read "gemm_route": the route of this thread's last launch_gemm -> {"rows256", "rows128", "shape128", "cus"} and "deferred": whether its last
        int8 linear armed the deferral of long outlier lists; host only"""
        out = np.zeros(5, np.float32)
        self._check(self.lib.sonic_debug_read(self.h, b"gemm_route", 0, _p(out), 5))
        return dict(zip(("rows256", "rows128", "shape128", "cus", "deferred"), (int(v) for v in out)))

    def _form_tensor(self, name: bytes, a, dtype: int):
        a = np.zeros(0, np.float32) if a is None else np.ascontiguousarray(a).reshape(-1)
        self._check(self.lib.sonic_load_tensor(self.h, name, _p(a if a.size else np.zeros(1, a.dtype)), dtype, (C.c_int64 * 1)(a.size), 1))

    def test_gemm_form(self, A, W, bias=None, resid=None, rope=None, C_fill=None, Vt_fill=None, **form):
        """The GEMM form hook (sonic_load_tensor "gemm.form:<buffer>" / "gemm.form.run", sonic_debug_read "gemm_form_c" / "gemm_form_vt"): one GEMM in a production launch
        form on the handle's own type.  A: flat; W [N][K]; form: the fields of GemmForm beside M / N / K
        (N, K from W; M is required).  C_fill / Vt_fill: what the pitched buffers hold before the launch (an array of the buffer's size, or a scalar; default 0).
        Returns the whole pitched C as [rows][ldc] - row c_row_offset of batch 0 is its first GEMM row, at least 8 rows follow the last - and, for EPI_QKV_VT,
        (C, Vt [segments][N - n_split][vt_ld]); on an int8 handle the q|k|v buffer is [rows][N].  Nothing stays staged on the handle."""
        W = np.ascontiguousarray(W, np.float32)
        N, K = W.shape
        f = GemmForm(N=N, K=K, **form)
        M, epi, batch = f.M, f.epi, max(f.batch, 1)
        n_out = N // 2 if epi == EPI_SWIGLU else f.n_split if epi == EPI_QKV_VT else N
        lda, ldc = f.lda or K, N if (self.mode == 1 and epi == EPI_QKV_VT) else (f.ldc or n_out)
        A = np.ascontiguousarray(A, np.float32).reshape(-1)
        assert M >= 1 and A.size >= (batch - 1) * f.strideA + (M - 1) * lda + K, "A is shorter than the form reads"
        c_elems = f.c_row_offset * ldc + (batch - 1) * f.strideC + (M + 8) * ldc
        Cb = np.empty(c_elems, np.float32)
        Cb[:] = 0.0 if C_fill is None else np.asarray(C_fill, np.float32).reshape(-1)
        r = _arr(resid, np.float32)
        assert r is None or r.size == M * (f.ldr or n_out)
        cs = _arr(rope, np.float32)
        Vt = None
        if epi == EPI_QKV_VT:
            assert f.seg_T > 0 and (cs is None or cs.shape == (f.seg_T, 32))
            Vt = np.empty((-(-M // f.seg_T), N - f.n_split, f.vt_ld), np.float32)
            Vt[:] = 0.0 if Vt_fill is None else np.asarray(Vt_fill, np.float32).reshape(Vt.shape if np.ndim(Vt_fill) else ())
        from .engine import DTYPE_F32, DTYPE_I32
        for name, a in ((b"A", A), (b"W", W), (b"bias", _arr(bias, np.float32)), (b"resid", r), (b"rope", cs), (b"C", Cb), (b"Vt", Vt)):
            self._form_tensor(b"gemm.form:" + name, a, DTYPE_F32)
        self._form_tensor(b"gemm.form.run", np.frombuffer(bytes(f), np.int32), DTYPE_I32)
        self._check(self.lib.sonic_debug_read(self.h, b"gemm_form_c", 0, _p(Cb), Cb.size))
        if Vt is not None:
            self._check(self.lib.sonic_debug_read(self.h, b"gemm_form_vt", 0, _p(Vt), Vt.size))
        for name in (b"C", b"Vt"):
            self._form_tensor(b"gemm.form:" + name, None, DTYPE_F32)
        Cb = Cb.reshape(-1, ldc) if c_elems % ldc == 0 else Cb
        return (Cb, Vt) if epi == EPI_QKV_VT else Cb

    def test_skinny(self, X, W):
        X = np.ascontiguousarray(X, np.float32); W = np.ascontiguousarray(W, np.float32)
        M, K = X.shape; N = W.shape[0]
        out = np.empty((M, N), np.float32)
        self._check(self.lib.sonic_test_skinny(self.h, _p(X), _p(W), _p(out), M, N, K))
        return out

    def test_attention(self, q, k, v, causal: bool):
        """q [B][Tq][Hq][hd], k/v [B][Tk][Hkv][hd] -> [B][Tq][Hq][hd]"""
        q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); v = np.ascontiguousarray(v, np.float32)
        B, Tq, Hq, hd = q.shape; Tk, Hkv = k.shape[1], k.shape[2]
        out = np.empty_like(q)
        self._check(self.lib.sonic_test_attention(self.h, _p(q), _p(k), _p(v), _p(out), B, Tq, Tk, Hq, Hkv, hd, int(causal)))
        return out

    def test_align(self, q, k):
        """sonic_test_attention on an align handle (option forced_align): q [B][Tq][Hq][128], k [B][Tk][Hkv][128] -> (M [B][Tq][Tk] float32,
        t [B][Tq] int32) - the three word-timestamp kernels over all Hq heads, every sequence's audio run being its Tk keys"""
        q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32)
        B, Tq, Hq, hd = q.shape; Tk, Hkv = k.shape[1], k.shape[2]
        out = np.empty((B, Tq, Tk + 1), np.float32)
        self._check(self.lib.sonic_test_attention(self.h, _p(q), _p(k), None, _p(out), B, Tq, Tk, Hq, Hkv, hd, 0))
        return out[:, :, :Tk].copy(), out[:, :, Tk].astype(np.int32)

    def test_decode_attention(self, q, k, v):
        """q [B][Hq][128], k/v [B][Tk][Hkv][128] -> [B][Hq][128]"""
        q = np.ascontiguousarray(q, np.float32); k = np.ascontiguousarray(k, np.float32); v = np.ascontiguousarray(v, np.float32)
        B, Hq, _ = q.shape; Tk, Hkv = k.shape[1], k.shape[2]
        out = np.empty_like(q)
        self._check(self.lib.sonic_test_decode_attention(self.h, _p(q), _p(k), _p(v), _p(out), B, Tk, Hq, Hkv))
        return out

    def test_layernorm(self, x, w, b=None, eps=1e-5, rms=False):
        x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
        bb = _arr(b, np.float32)
        out = np.empty_like(x)
        self._check(self.lib.sonic_test_layernorm(self.h, _p(x), _p(w), _p(bb), _p(out), x.shape[0], x.shape[1], eps, int(rms)))
        return out

    def bench_gemm(self, M: int, N: int, K: int, epi: int = EPI_BIAS_GELU, iters: int = 20) -> float:
        ms = C.c_float(0)
        self._check(self.lib.sonic_bench_gemm(self.h, M, N, K, epi, iters, C.byref(ms)))
        return float(ms.value)

    def bench_skinny(self, M: int, N: int, K: int, variant: int, iters: int = 50) -> float:
        us = C.c_float(0)
        self._check(self.lib.sonic_bench_skinny(self.h, M, N, K, variant, iters, C.byref(us)))
        return float(us.value)

    def debug_ktrace(self) -> np.ndarray:
        """[slot 8][block 512][point 8] device wall-clock ticks (10 ns) of the decode kernels of the layer set by option "ktrace"."""
        out = np.zeros((8, 512, 8), np.int64)
        self._check(self.lib.sonic_debug_ktrace(self.h, _p(out), out.size))
        return out

    def debug_read(self, name: str, shape, index: int = 0) -> np.ndarray:
        out = np.empty(shape, np.float32)
        self._check(self.lib.sonic_debug_read(self.h, name.encode(), index, _p(out), out.size))
        return out

    def test_skinny_gu(self, X, Wi):
        X = np.ascontiguousarray(X, np.float32); Wi = np.ascontiguousarray(Wi, np.float32)
        M, K = X.shape; N = Wi.shape[0]
        out = np.empty((M, N // 2), np.float32)
        self._check(self.lib.sonic_test_skinny_gu(self.h, _p(X), _p(Wi), _p(out), M, N, K))
        return out

    def _greedy(self, entry: str, slabs, B: int, want_logits: bool = True, want_lp: bool = True, force_ids=None, guard=None, tables=None, samp=None, want_noise: bool = False):
        """What the five greedy wrappers share: slabs, history, suppress list, tables, forced ids and outputs prepared once, then sonic_test_<entry> - the C entry
        point of the wrapper that calls, never another family's.  guard = (hist, hist_len, repetition_penalty, no_repeat_ngram_size, suppress_tokens) for the
        entries that take histories; samp = (temperature, seed, step).  -> (tok, logits or None, lp or None, noise or None).  On a handle with option
        top_logprobs = K > 0 the hooks return row b's whole record, and lp is an engine.TokenScores: lp [B], top_logprobs [B, K], top_ids [B, K]"""
        s = np.ascontiguousarray(slabs, np.float32)
        ks, mpad, V = s.shape
        args = [_p(s), ks, mpad, V, B]
        if guard is not None:
            hist, hist_len, penalty, ngram, suppress_tokens = guard
            h = hl = None
            if hist_len is not None:
                h = np.ascontiguousarray(hist, np.int32).reshape(B, -1)
                hl = np.ascontiguousarray(hist_len, np.int32)
            sup = np.ascontiguousarray(list(suppress_tokens), dtype=np.int32)
            args += [_p(h) if h is not None and h.size else None, 0 if h is None else h.shape[1], _p(hl), float(penalty), int(ngram), _p(sup) if sup.size else None, int(sup.size)]
        if entry != "greedy":
            f = _arr(force_ids, np.int32)
            args.append(_p(f))
        if entry in ("greedy_bias", "greedy_sample"):
            seq_ids = seq_off = bias = req_off = None
            if tables is not None:
                from .engine import pack_request_bias
                seq_ids, seq_off, bias, req_off = pack_request_bias(list(tables))
            args += [_p(seq_ids) if seq_ids is not None and seq_ids.size else None, _p(seq_off), _p(bias) if bias is not None and bias.size else None, _p(req_off)]
        if samp is not None:
            t = np.ascontiguousarray(samp[0], np.float32)
            sd = np.ascontiguousarray([int(x) for x in samp[1]], np.uint64)
            stp = np.ascontiguousarray(samp[2], np.int32)
            assert t.shape == sd.shape == stp.shape == (B,)
            args += [_p(t), _p(sd), _p(stp)]
        tok = np.zeros(B, np.int32)
        lg = np.zeros((B, V), np.float32) if want_logits else None
        K = int(getattr(self, "top_logprobs", 0))
        lp = np.full(B * (1 + 2 * K), np.nan, np.float32) if want_lp else None
        noise = np.zeros((B, V), np.float32) if want_noise else None
        out = [tok, lg] + ([lp] if entry != "greedy" else []) + ([noise] if samp is not None else [])
        self._check(getattr(self.lib, "sonic_test_" + entry)(self.h, *args, *[_p(o) for o in out]))
        if K and lp is not None:
            from .engine import unpack_logprobs
            lp = unpack_logprobs(lp, B, K)
        return tok, lg, lp, noise

    def test_greedy(self, slabs, B: int, want_logits: bool = False):
        """slabs: [ksplit][mpad][V] fp32 -> (token per row [B], bf16 logits [B][V] or None)"""
        return self._greedy("greedy", slabs, B, want_logits, want_lp=False)[:2]

    def test_greedy_lp(self, slabs, B: int, force_ids=None):
        """sonic_test_greedy through greedy_kernel<T, true>: slabs [ksplit][mpad][V] fp32 -> (token per row [B], logits [B][V], log-probability of the
        emitted token [B]); force_ids [B]: the token every row emits instead of its argmax"""
        return self._greedy("greedy_lp", slabs, B, force_ids=force_ids)[:3]

    def test_greedy_guard(self, slabs, B: int, hist, hist_len, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, suppress_tokens=(), force_ids=None,
                          want_lp: bool = False):
        """sonic_test_greedy through greedy_kernel<T, LP, true>: slabs [ksplit][mpad][V] fp32, hist [B][ld] int (row b's first hist_len[b] entries are its
        history) -> (token per row [B], RAW logits [B][V], log-probability of the emitted token over the processed scores [B] or None)"""
        return self._greedy("greedy_guard", slabs, B, True, want_lp, force_ids, (hist, hist_len, repetition_penalty, no_repeat_ngram_size, suppress_tokens))[:3]

    def test_greedy_bias(self, slabs, B: int, hist, hist_len, tables, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, suppress_tokens=(), force_ids=None,
                         want_lp: bool = False):
        """sonic_test_greedy_guard through greedy_kernel<T, LP, true, true>: `tables` holds one reqbias.RequestBias or None per row -> (token per row [B], RAW
        logits [B][V], log-probability of the emitted token over the processed scores [B] or None)"""
        return self._greedy("greedy_bias", slabs, B, True, want_lp, force_ids, (hist, hist_len, repetition_penalty, no_repeat_ngram_size, suppress_tokens), list(tables))[:3]

    def test_greedy_sample(self, slabs, B: int, temperature, seed, step, hist=None, hist_len=None, tables=None, repetition_penalty: float = 1.0,
                           no_repeat_ngram_size: int = 0, suppress_tokens=(), force_ids=None, want_noise: bool = True):
        """sonic_test_greedy_sample: the sampling instantiations of the greedy kernel in this handle's type.  hist_len None: the plain family; tables None: the guard
        family; else the bias family -> (token [B], RAW logits [B][V], log-probability over the processed scores at temperature 1 [B], Gumbel noise used [B][V] or None)"""
        return self._greedy("greedy_sample", slabs, B, True, True, force_ids, (hist, hist_len, repetition_penalty, no_repeat_ngram_size, suppress_tokens), tables,
                            (temperature, seed, step), want_noise)

    def arm_truncation_hook(self, rows):
        """sonic_load_tensor "truncation.hook": float32 [B][3] rows of (top_k, top_p, min_p) for the next test_greedy_sample launch on this handle (also the one inside
        test_greedy_grammar); the library validates them (SonicError naming the parameter)"""
        from .engine import DTYPE_F32, SonicError
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 3)
        if self.lib.sonic_load_tensor(self.h, b"truncation.hook", _p(rows), DTYPE_F32, (C.c_int64 * 2)(len(rows), 3), 2) != 0:
            raise SonicError((self.lib.sonic_last_error(None) or b"").decode())

    def read_truncation_hook(self, B: int):
        """sonic_debug_read "hook_truncation": the records of the last launch that took a truncation -> (the bits of the y of the last kept id [B] (uint32), that
        id [B], the kept count n [B]); a row that took the branch around the select (t = 0, the three filters off, or scores of -inf only) reports (0, -1, V)"""
        rec = np.zeros(64 * 3, np.float32)
        self._check(self.lib.sonic_debug_read(self.h, b"hook_truncation", 0, _p(rec), 3 * B))
        rec = rec[: 3 * B].reshape(B, 3)
        return np.ascontiguousarray(rec[:, 0]).view(np.uint32), rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)

    def test_greedy_truncation(self, slabs, B: int, temperature, seed, step, truncation, **kw):
        """The TRUNC instantiations of the greedy kernel: `truncation`, one (top_k, top_p, min_p) per row (sampling.pack_truncation validates them),
        is armed on the handle and the test_greedy_sample launch that follows (its keywords: **kw) takes it -> test_greedy_sample's four results and the rows' records"""
        from . import sampling
        rows = sampling.pack_truncation(list(truncation))
        assert rows.shape == (B, 3)
        self.arm_truncation_hook(rows)
        return self.test_greedy_sample(slabs, B, temperature, seed, step, **kw) + (self.read_truncation_hook(B),)

    def test_greedy_grammar(self, slabs, B: int, grammar, state_in, eos_ids=(), hist=None, hist_len=None, tables=None, samp=None, repetition_penalty: float = 1.0,
                            no_repeat_ngram_size: int = 0, suppress_tokens=(), force_ids=None, want_noise: bool = True):
        """The grammar instantiations of the greedy kernel in this handle's type (include/sonic_hip.h beside sonic_test_greedy_sample): the automaton is armed on the
        handle (sonic_load_tensor "grammar.hook:<V>", options hook_grammar_state / hook_grammar_eos) and the next guard / bias / sample hook launch takes it.
        grammar: a grammar.Grammar (one automaton for the launch); state_in [B]: -1 a free row, n a node, -2 left; eos_ids: what a row at -2 may emit.  tables (one
        reqbias.RequestBias or None per row): the bias families; samp = (temperature, seed, step): the sampling families -> (token [B], RAW logits [B][V],
        log-probability over the masked scores [B] - a TokenScores with option top_logprobs -, Gumbel noise [B][V] or None, state out [B])"""
        from .engine import DTYPE_I32, SonicError, grammar_words
        V = np.asarray(slabs).shape[2]
        w = grammar_words(grammar)
        if self.lib.sonic_load_tensor(self.h, f"grammar.hook:{V}".encode(), _p(w), DTYPE_I32, (C.c_int64 * 1)(len(w)), 1) != 0:
            raise SonicError((self.lib.sonic_last_error(None) or b"").decode())
        si = np.ascontiguousarray(state_in, np.int32)
        assert si.shape == (B,)
        for b in range(B):
            self._check(self.lib.sonic_set_option(self.h, b"hook_grammar_state", (b << 20) | (int(si[b]) + 2)))
        for t in eos_ids:
            self._check(self.lib.sonic_set_option(self.h, b"hook_grammar_eos", int(t)))
        h = np.zeros((B, 1), np.int32) if hist is None else np.ascontiguousarray(hist, np.int32).reshape(B, -1)
        hl = np.zeros(B, np.int32) if hist_len is None else np.ascontiguousarray(hist_len, np.int32)
        guard = (h, hl, repetition_penalty, no_repeat_ngram_size, suppress_tokens)
        if samp is not None:
            tok, lg, lp, noise = self._greedy("greedy_sample", slabs, B, True, True, force_ids, guard, tables, samp, want_noise)
        elif tables is not None:
            tok, lg, lp, noise = self._greedy("greedy_bias", slabs, B, True, True, force_ids, guard, list(tables))
        else:
            tok, lg, lp, noise = self._greedy("greedy_guard", slabs, B, True, True, force_ids, guard)
        so = np.zeros(64, np.float32)
        self._check(self.lib.sonic_debug_read(self.h, b"hook_grammar_state", 0, _p(so), B))
        return tok, lg, lp, noise, so[:B].astype(np.int32)

    def arm_lm_hook(self, lm, V: Optional[int] = None):
        """sonic_load_tensor "lm.hook:<V>": an ngram.NGramLM (or its packed words) for the language-model hooks of this handle, validated against V (SonicError in the
        library's words); every row at the start node, no token pending, weight 0.  None disarms"""
        from .engine import DTYPE_I32, SonicError
        w = np.zeros(0, np.int32) if lm is None else np.ascontiguousarray(lm.pack() if hasattr(lm, "pack") else lm, dtype=np.int32)
        V = int(V if V is not None else (w[0] if len(w) else 0))
        self._lm_hook_V = V
        if self.lib.sonic_load_tensor(self.h, f"lm.hook:{V}".encode(), _p(w if len(w) else np.zeros(1, np.int32)), DTYPE_I32, (C.c_int64 * 1)(len(w)), 1) != 0:
            raise SonicError((self.lib.sonic_last_error(None) or b"").decode())

    def test_lm_step(self, B: int, state_in, tok_in, weight: float, finished=None, want_add: bool = True):
        """lm_step_kernel alone over B rows of the armed hook model: row b enters at state_in[b] with the pending token tok_in[b] (-1: none) ->
        (state out [B], pending token out [B], the vectors [B][V] float32 - zeros for a finished row - or None)"""
        from .engine import DTYPE_I32, SonicError, weight_bits
        self._check(self.lib.sonic_set_option(self.h, b"hook_lm_weight", weight_bits(weight)))
        for b in range(B):
            self._check(self.lib.sonic_set_option(self.h, b"hook_lm_state", (b << 24) | int(state_in[b])))
            self._check(self.lib.sonic_set_option(self.h, b"hook_lm_tok", (b << 24) | (int(tok_in[b]) + 1)))
        fin = np.zeros(B, np.int32) if finished is None else np.ascontiguousarray(finished, np.int32)
        assert fin.shape == (B,)
        if self.lib.sonic_load_tensor(self.h, b"lm.hook.step", _p(fin), DTYPE_I32, (C.c_int64 * 1)(B), 1) != 0:
            raise SonicError((self.lib.sonic_last_error(self.h) or self.lib.sonic_last_error(None) or b"").decode())
        st, tk = self.read_lm_hook(B)
        add = None
        if want_add:
            V = int(self._lm_hook_V)
            add = self.debug_read("hook_lm_add", (B, V))
        return st, tk, add

    def read_lm_hook(self, B: int):
        """sonic_debug_read "hook_lm_state" / "hook_lm_tok": the rows' words as the last language-model hook launch left them"""
        return self.debug_read("hook_lm_state", (B,)).astype(np.int32), self.debug_read("hook_lm_tok", (B,)).astype(np.int32)

    def test_greedy_lm(self, slabs, B: int, lm, state_in, weight: float, tok_in=None, hist=None, hist_len=None, tables=None, samp=None, repetition_penalty: float = 1.0,
                       no_repeat_ngram_size: int = 0, suppress_tokens=(), force_ids=None, want_noise: bool = True):
        """The LM instantiations of the greedy kernel in this handle's type: `lm` (an ngram.NGramLM) is armed, lm_step_kernel builds the rows' vectors at state_in
        and `weight`, and the guard / bias / sample hook launch that follows takes them.  tables: the bias families; samp = (temperature, seed, step): the sampling
        families -> (token [B], RAW logits [B][V], log-probability over the fused scores [B] - a TokenScores with option top_logprobs -, Gumbel noise [B][V] or None,
        the vectors [B][V], the rows' pending tokens behind the launch [B])"""
        V = np.asarray(slabs).shape[2]
        self.arm_lm_hook(lm, V)
        _, _, add = self.test_lm_step(B, state_in, [-1] * B if tok_in is None else tok_in, weight)
        h = np.zeros((B, 1), np.int32) if hist is None else np.ascontiguousarray(hist, np.int32).reshape(B, -1)
        hl = np.zeros(B, np.int32) if hist_len is None else np.ascontiguousarray(hist_len, np.int32)
        guard = (h, hl, repetition_penalty, no_repeat_ngram_size, suppress_tokens)
        if samp is not None:
            tok, lg, lp, noise = self._greedy("greedy_sample", slabs, B, True, True, force_ids, guard, tables, samp, want_noise)
        elif tables is not None:
            tok, lg, lp, noise = self._greedy("greedy_bias", slabs, B, True, True, force_ids, guard, list(tables))
        else:
            tok, lg, lp, noise = self._greedy("greedy_guard", slabs, B, True, True, force_ids, guard)
        return tok, lg, lp, noise, add, self.read_lm_hook(B)[1]

    def test_linear_int8(self, X, W, bias=None, resid=None, group_rows=None, epi=EPI_BIAS):
        """One Linear8bitLt call; X [M][K], W [N][K] fp16-valued. group_rows: rows per reference call (default: all rows one call)."""
        X = np.ascontiguousarray(X, np.float32); W = np.ascontiguousarray(W, np.float32)
        M, K = X.shape; N = W.shape[0]
        out = np.empty((M, N // 2 if epi == EPI_SWIGLU else N), np.float32)
        b = _arr(bias, np.float32)
        r = _arr(resid, np.float32)
        self._check(self.lib.sonic_test_linear_int8(self.h, _p(X), _p(W), _p(b), _p(r), _p(out), M, N, K, int(group_rows or M), epi))
        return out

    def test_decode_attention_cache(self, kcache, vcache, kv_len, Hq: int, q=None, slabs=None, rope_cs=None, want_caches: bool = True):
        """The decode attention as decode_step launches it.  kcache / vcache [B][Hkv][ctx_max][128] (whole, the caller fills what lies behind kv_len),
        kv_len [B] (new token included).  Either q [B][Hq][128] (nothing appended) or slabs [ksplit][mpad][(Hq + 2 Hkv) * 128] with rope_cs [ctx_max][128]
        (fused slab sum + RoPE + append).  Returns (out [B][Hq][128], kcache after, vcache after); the caches are None unless want_caches."""
        kc = np.ascontiguousarray(kcache, np.float32); vc = np.ascontiguousarray(vcache, np.float32)
        B, Hkv, ctx, hd = kc.shape
        assert hd == 128 and vc.shape == kc.shape and (q is None) != (slabs is None)
        kl = np.ascontiguousarray(kv_len, np.int32)
        assert kl.shape == (B,)
        ks = mpad = 0
        if q is not None:
            q = np.ascontiguousarray(q, np.float32)
            assert q.shape == (B, Hq, 128)
        else:
            slabs = np.ascontiguousarray(slabs, np.float32); rope_cs = np.ascontiguousarray(rope_cs, np.float32)
            ks, mpad = slabs.shape[:2]
            assert slabs.shape == (ks, mpad, (Hq + 2 * Hkv) * 128) and rope_cs.shape == (ctx, 128)
        out = np.empty((B, Hq, 128), np.float32)
        ko = np.empty_like(kc) if want_caches else None
        vo = np.empty_like(vc) if want_caches else None
        self._check(self.lib.sonic_test_decode_attention_cache(self.h, _p(q), _p(slabs), ks, mpad, _p(rope_cs), _p(kc), _p(vc), _p(kl), _p(out), _p(ko), _p(vo),
                                                               B, Hq, Hkv, ctx))
        return out, ko, vo

    def arm_share_prompt_hook(self, pre_row, pre_len):
        """sonic_load_tensor "share_prompt.hook": int32 [2][B] = pre_row | pre_len for the next test_prefill_attention launch on this handle, which then runs the
        shared-prefix kernel and validates them against its shapes"""
        from .engine import DTYPE_I32, SonicError
        w = np.ascontiguousarray(np.stack([np.asarray(pre_row, np.int32), np.asarray(pre_len, np.int32)]), np.int32)
        if self.lib.sonic_load_tensor(self.h, b"share_prompt.hook", _p(w), DTYPE_I32, (C.c_int64 * 2)(2, w.shape[1]), 2) != 0:
            raise SonicError((self.lib.sonic_last_error(None) or b"").decode())

    def test_prefill_attention(self, q, kcache, vt, q_off, q_len, kv_len, out_init=None, pre_row=None, pre_len=None):
        """The prefill's causal attention with run_prefill's strides.  q [n_tok][Hq][128] packed, kcache [B][Hkv][ctx_max][128], vt [B][Hkv][128][ctx_max],
        q_off / q_len / kv_len [B].  out_init [n_tok][Hq][128] is what the output buffer holds before the launch (default zeros).  pre_row / pre_len [B]: armed as
        the share-prompt hook first - sequence b's keys [0, pre_len[b]) are those of cache row pre_row[b].  -> [n_tok][Hq][128]"""
        q = np.ascontiguousarray(q, np.float32); kc = np.ascontiguousarray(kcache, np.float32); vt = np.ascontiguousarray(vt, np.float32)
        n_tok, Hq, hd = q.shape
        B, Hkv, ctx, _ = kc.shape
        assert hd == 128 and kc.shape[3] == 128 and vt.shape == (B, Hkv, 128, ctx)
        qo, ql, kl = (np.ascontiguousarray(x, np.int32) for x in (q_off, q_len, kv_len))
        assert qo.shape == ql.shape == kl.shape == (B,)
        if pre_row is not None:
            self.arm_share_prompt_hook(pre_row, pre_len)
        out = np.zeros_like(q) if out_init is None else np.array(out_init, np.float32, order="C")
        assert out.shape == q.shape
        self._check(self.lib.sonic_test_prefill_attention(self.h, _p(q), _p(kc), _p(vt), _p(qo), _p(ql), _p(kl), _p(out), n_tok, B, Hq, Hkv, ctx))
        return out

    def test_add_rmsnorm(self, x, slabs, w, eps: float, rows: int, y_init=None, quant: bool = False):
        """add_rmsnorm_kernel as the decode step launches it.  x [rows_alloc][d], slabs [ksplit][mpad][d] fp32, w [d]; y_init [rows_alloc][d] is what the output
        buffer holds before the launch (default zeros).  -> (x after, y after[, (q int8 [rows][d], sca [rows], oc_cnt [rows], oc_list [rows][d], oc_val [rows][d])]);
        list entries the kernel did not write are -1 / 0.  quant needs an fp16 engine."""
        x = np.array(x, np.float32, order="C"); s = np.ascontiguousarray(slabs, np.float32); w = np.ascontiguousarray(w, np.float32)
        rows_alloc, d = x.shape
        ks, mpad = s.shape[:2]
        assert s.shape == (ks, mpad, d) and w.shape == (d,)
        y = np.zeros_like(x) if y_init is None else np.array(y_init, np.float32, order="C")
        assert y.shape == x.shape
        qb = _quant_bufs(rows, d) if quant else (None,) * 5
        self._check(self.lib.sonic_test_add_rmsnorm(self.h, _p(x), _p(s), ks, mpad, _p(w), float(eps), _p(y), int(rows), rows_alloc, d, *[_p(b) for b in qb]))
        return (x, y, qb) if quant else (x, y)

    def test_quant_rows(self, X, K: Optional[int] = None):
        """quant_rows_kernel on X [M][ld] (fp16 values; the first K columns of every row, default all) -> (q, sca, oc_cnt, oc_list, oc_val) as test_add_rmsnorm"""
        X = np.ascontiguousarray(X, np.float32)
        M, ld = X.shape
        K = ld if K is None else int(K)
        qb = _quant_bufs(M, K)
        self._check(self.lib.sonic_test_quant_rows(self.h, _p(X), M, K, ld, *[_p(b) for b in qb]))
        return qb

    def test_swiglu_slab(self, slabs, rows: int, gu8: int):
        """swiglu_slab_kernel: slabs [ksplit][mpad][2 ff] fp32 -> act [rows][ff]"""
        s = np.ascontiguousarray(slabs, np.float32)
        ks, mpad, n2 = s.shape
        act = np.empty((rows, n2 // 2), np.float32)
        self._check(self.lib.sonic_test_swiglu_slab(self.h, _p(s), ks, mpad, n2 // 2, int(rows), int(gu8), _p(act)))
        return act

    def test_decode_o_gu(self, att, Wo, resid, ln_w, eps: float, Wgu, form: int, want_ss: bool = False):
        """One layer's o_proj -> RMSNorm -> gate/up chain (sonic_test_decode_o_gu).  att [M][K], Wo [D][K], resid [rows_alloc][D], ln_w [D], Wgu [2 ff][D] (gate / up rows
        interleaved in groups of 16).  -> dict: resid [rows_alloc][D], act [M][ff], hn [M][D] (forms 1, 2), ss [2][D / 64][32][4] (want_ss, forms 0, 1)"""
        att = np.ascontiguousarray(att, np.float32); Wo = np.ascontiguousarray(Wo, np.float32); Wgu = np.ascontiguousarray(Wgu, np.float32)
        r = np.array(resid, np.float32, order="C"); w = np.ascontiguousarray(ln_w, np.float32)
        M, K = att.shape; D = Wo.shape[0]; ff = Wgu.shape[0] // 2
        assert Wo.shape == (D, K) and r.shape[1] == D and w.shape == (D,) and Wgu.shape == (2 * ff, D)
        hn = np.empty((M, D), np.float32) if form != 0 else None
        act = np.empty((M, ff), np.float32)
        ss = np.empty((2, D // 64, 32, 4), np.float32) if want_ss else None
        self._check(self.lib.sonic_test_decode_o_gu(self.h, _p(att), _p(Wo), _p(r), _p(w), float(eps), _p(Wgu), int(form), M, K, D, ff, r.shape[0], _p(hn), _p(act), _p(ss)))
        return {"resid": r, "act": act, "hn": hn, "ss": ss}

    def test_rope_append(self, qkv, cs, tok_seq, tok_pos, q_off, q_len, Hq: int, kcache, vcache, vt, tiled: bool):
        """The prefill's RoPE + KV append.  qkv [n_tok][(Hq + 2 Hkv) * 128], cs [ctx_max][128], kcache / vcache [B][Hkv][ctx_max][128], vt [B][Hkv][128][vt_ld] as the
        buffers are before the launch.  -> (q [n_tok][Hq][128], kcache, vcache, vt after)"""
        qkv = np.ascontiguousarray(qkv, np.float32); cs = np.ascontiguousarray(cs, np.float32)
        kc = np.array(kcache, np.float32, order="C"); vc = np.array(vcache, np.float32, order="C"); vt = np.array(vt, np.float32, order="C")
        B, Hkv, ctx, hd = kc.shape
        n_tok = qkv.shape[0]
        assert hd == 128 and vc.shape == kc.shape and vt.shape[:3] == (B, Hkv, 128) and cs.shape == (ctx, 128) and qkv.shape[1] == (Hq + 2 * Hkv) * 128
        ts, tp, qo, ql = (np.ascontiguousarray(a, np.int32) for a in (tok_seq, tok_pos, q_off, q_len))
        assert ts.shape == tp.shape == (n_tok,) and qo.shape == ql.shape == (B,)
        q = np.empty((n_tok, Hq, 128), np.float32)
        self._check(self.lib.sonic_test_rope_append(self.h, _p(qkv), _p(cs), _p(ts), _p(tp), _p(qo), _p(ql), n_tok, B, Hq, Hkv, ctx, vt.shape[3], int(tiled),
                                                    _p(q), _p(kc), _p(vc), _p(vt)))
        return q, kc, vc, vt

    def test_rope_enc(self, qk, T: int, heads2: int, rd: int, cs, hd: int = 64):
        """rope_enc_kernel on a copy of qk [M][ld]; cs [T][rd]"""
        qk = np.array(qk, np.float32, order="C"); cs = np.ascontiguousarray(cs, np.float32)
        assert cs.shape == (T, rd)
        self._check(self.lib.sonic_test_rope_enc(self.h, _p(qk), qk.shape[0], qk.shape[1], int(T), int(heads2), int(hd), int(rd), _p(cs)))
        return qk

    # ---- the int8 token step: one decode-flavour Linear8bitLt plus its consumer (int8 engines; X [M][K], W [N][K] fp16-valued).  layout 0: W tiled; 1: also the
    # k-major copy.  Every result dict carries "ksplit" and "cfg" (the int8 skinny GEMM's tiling as launched) and, with want_slab, "slab" int32 [M][N]
    @staticmethod
    def _i8_info(r, info, slab):
        r["ksplit"], r["cfg"] = int(info[0]), int(info[1])
        if slab is not None:
            r["slab"] = slab
        return r

    def test_decode_i8_norm(self, X, W, x, norm_w, eps: float, form: int, layout: int, amax=None, big=None, y_init=None, want_slab: bool = False):
        """o_proj / down_proj -> add_rmsnorm with a DeqInfo and a QuantOut.  x [rows_alloc][N] residual rows, norm_w [N]; y_init [rows_alloc][N] is what the output
        buffer holds before the launch (default zeros).  form 1: amax [M][4] fp32 partial maxima, big [M][4] int32 counts.  -> dict: x, y [rows_alloc][N] after,
        quant = (q int8 [M][N], sca [M], oc_cnt [M], oc_list [M][N], oc_val [M][N])"""
        X = np.ascontiguousarray(X, np.float32); W = np.ascontiguousarray(W, np.float32)
        M, K = X.shape; N = W.shape[0]
        x = np.array(x, np.float32, order="C"); w = np.ascontiguousarray(norm_w, np.float32)
        assert W.shape == (N, K) and x.shape[1] == N and w.shape == (N,)
        y = np.zeros_like(x) if y_init is None else np.array(y_init, np.float32, order="C")
        assert y.shape == x.shape
        am = _arr(amax, np.float32); bg = _arr(big, np.int32)
        assert (am is None or am.shape == (M, 4)) and (bg is None or bg.shape == (M, 4))
        qb = _quant_bufs(M, N)
        info = np.zeros(2, np.int32); slab = np.zeros((M, N), np.int32) if want_slab else None
        self._check(self.lib.sonic_test_decode_i8_norm(self.h, _p(X), _p(W), _p(x), _p(w), float(eps), _p(y), _p(am), _p(bg), M, N, K, x.shape[0], int(form), int(layout),
                                                       *[_p(b) for b in qb], _p(info), _p(slab)))
        return self._i8_info({"x": x, "y": y, "quant": qb}, info, slab)

    def test_decode_i8_swiglu(self, X, Wgu, layout: int, act_init=None, want_slab: bool = False):
        """gate/up -> swiglu_quant.  Wgu [2 ff][K], gate / up rows interleaved in groups of 16; act_init [rows_alloc][ff] (default: M rows of zeros).
        -> dict: act [rows_alloc][ff] after, quant = the five quantiser outputs of act's first M rows"""
        X = np.ascontiguousarray(X, np.float32); W = np.ascontiguousarray(Wgu, np.float32)
        M, K = X.shape; ff = W.shape[0] // 2
        assert W.shape == (2 * ff, K)
        act = np.zeros((M, ff), np.float32) if act_init is None else np.array(act_init, np.float32, order="C")
        assert act.shape[1] == ff
        qb = _quant_bufs(M, ff)
        info = np.zeros(2, np.int32); slab = np.zeros((M, 2 * ff), np.int32) if want_slab else None
        self._check(self.lib.sonic_test_decode_i8_swiglu(self.h, _p(X), _p(W), _p(act), M, ff, K, act.shape[0], int(layout), *[_p(b) for b in qb], _p(info), _p(slab)))
        return self._i8_info({"act": act, "quant": qb}, info, slab)

    def test_decode_i8_attn(self, X, Wqkv, rope_cs, kcache, vcache, kv_len, Hq: int, amax, big, layout: int, want_slab: bool = False):
        """q|k|v -> the fused decode attention with the int8 prologue.  X [B][D] hidden rows, Wqkv [(Hq + 2 Hkv) * 128][D]; rope_cs, kcache, vcache, kv_len as
        test_decode_attention_cache; amax [B][4] fp32 and big [B][4] int32 as the buffers are before the launch.  -> dict: out [B][Hq][128], kcache, vcache, amax, big after"""
        X = np.ascontiguousarray(X, np.float32); W = np.ascontiguousarray(Wqkv, np.float32); cs = np.ascontiguousarray(rope_cs, np.float32)
        kc = np.ascontiguousarray(kcache, np.float32); vc = np.ascontiguousarray(vcache, np.float32)
        B, D = X.shape
        _, Hkv, ctx, hd = kc.shape
        N = (Hq + 2 * Hkv) * 128
        assert hd == 128 and kc.shape == vc.shape == (B, Hkv, ctx, 128) and W.shape == (N, D) and cs.shape == (ctx, 128)
        kl = np.ascontiguousarray(kv_len, np.int32)
        am = np.array(amax, np.float32, order="C"); bg = np.array(big, np.int32, order="C")
        assert kl.shape == (B,) and am.shape == bg.shape == (B, 4)
        out = np.empty((B, Hq, 128), np.float32); ko = np.empty_like(kc); vo = np.empty_like(vc)
        info = np.zeros(2, np.int32); slab = np.zeros((B, N), np.int32) if want_slab else None
        self._check(self.lib.sonic_test_decode_i8_attn(self.h, _p(X), _p(W), _p(cs), _p(kc), _p(vc), _p(kl), _p(am), _p(bg), _p(out), _p(ko), _p(vo),
                                                       B, D, Hq, Hkv, ctx, int(layout), _p(info), _p(slab)))
        return self._i8_info({"out": out, "kcache": ko, "vcache": vo, "amax": am, "big": bg}, info, slab)
