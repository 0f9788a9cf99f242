"""What the GPU test files share (imported like glue_ref.py; not a conftest, not collected): the synthetic seed, prompts, engines with their options in a given
order, the GEMM routing options with the assertions on the route witness, bit comparisons, the float64 log-softmax reference, the derived log-probability bounds, the kernel hooks' slabs, the six invariance segments and the loaders
behind the `orc` / `golden` fixtures.  tests/test_common_host.py pins every one of them on the CPU.

The log-probability bound (DESIGN.md 6.3 goes through the kernel line by line).  With u = 2^-24, V the vocabulary, n_t = ceil(V / 4096) * 4 the elements one
thread adds and ref64 the float64 log-softmax of the very fp32 scores the kernel compared,

    |lp - ref64| <= (n_t + 3 * (ceil(n_t / 16) - 1) + 2 + 16 + 1 + 2.25 * ln V) * u + u * |ref64|

  n_t                     the adds a thread's first term goes through, one rounding each
  3 * (trips - 1)         one rescale of the running sum per later trip of the unrolled loop: v_exp_f32 (1 ulp <= 2 u) and a multiply
  2                       v_exp_f32 of the term itself
  16                      the merges: lane -> wave maximum (3), six butterfly adds, wave -> block maximum (3), four levels of the tree over 16 waves
  1                       second-order terms and the fp64 tail (log, subtractions)
  2.25 ln V               the arguments of exp: r - max rounds (u |x|; exact for bf16 / fp16 logits), x * log2(e) rounds (u |x|) with a constant that is
                          0.22 u off; along a term's path the shifts add up to x_i = l_i - max(l), and sum_i p_i |x_i| = H(p) - log(sum) <= ln V
  u |ref64|               the one rounding of the fp64 result to fp32
Guards, bias, sampling, truncation and grammar add no rounding to the sum, they change the scores it is taken over: their tests evaluate the same bound over the
processed scores.  The row kernel of scoring and draft verify walks a row in strides of 16384 with 16 elements per thread and trip; the
derivation is the same with n_t = ceil(V / 16384) * 16 (score_bound)."""
import contextlib
import math
import os

import numpy as np

from sonicscribe_amd import spec, synth

SEED = 20260128
U = 2.0 ** -24
PREFIX = (1, 17, 23, 5)
SUFFIX = (7, 301, 302, 303, 9, 11)


# ------------------------------------------------------------------------------------------ prompts, engines, segments
def prompt_for(d, n_samples, tail=(), suffix=SUFFIX, prefix=PREFIX):
    """prefix + one audio token per encoder output of n_samples (one length, or a sequence of window lengths whose audio tokens are summed) + suffix + tail"""
    windows = [n_samples] if np.ndim(n_samples) == 0 else n_samples
    n_audio = sum(spec.audio_token_count(spec.valid_frames(int(n))) for n in windows)
    return list(prefix) + [d.audio_token_id] * n_audio + list(suffix) + list(tail)


def make_engine(dims=spec.TINY, mode=0, max_batch=4, max_ctx=1024, options=(), seed=SEED, device=0):
    """an Engine with `options` applied in the order given (several are refused out of order), then the synthetic weights.  A key of "generation" takes the
    keyword dict of Engine.set_generation at that point of the order; every other (key, value) is a set_option"""
    from sonicscribe_amd.engine import Engine
    e = Engine(dims, device, mode, max_batch=max_batch, max_ctx=max_ctx)
    for key, value in options:
        if key == "generation":
            e.set_generation(**value)
        else:
            e.set_option(key, value)
    e.load_synthetic(seed)
    return e


def flags(*pairs):
    """the (key, value) options whose flag is truthy, in the order written: flags((lp, "token_logprobs", 1), (k, "top_logprobs", k))"""
    return [tuple(p[1:]) for p in pairs if p[0]]


def six(d=spec.TINY):
    """the six synthetic segments of the invariance tests with their prompts"""
    segs = [synth.synth_pcm(700 + i, n) for i, n in enumerate((48000, 200000, 80000, 64000, 120000, 96000))]
    return segs, [prompt_for(d, len(s)) for s in segs]


# ------------------------------------------------------------------------------------------ GEMM routes (csrc/gemm.hip gemm_plan; Engine.debug_gemm_route is the witness)
ROUTE_DEFAULTS = {"gemm_small_eff": 75, "gemm_force128": 0, "gemm128_shallow": 0, "no_fused_rope": 0, "i8_no_qkv_fuse": 0}
BIG_TILE = {"gemm_small_eff": 0}            # every eligible GEMM on the 256x256 tile
FORCE128 = {"gemm_force128": 1}             # ... on the 128x128 kernel, at the launch shape its grid selects
SHALLOW128 = {"gemm_force128": 1, "gemm128_shallow": 1}     # ... at its 128x128 two-stage shape


@contextlib.contextmanager
def route_options(eng, opts):
    """the routing options `opts` (keys of ROUTE_DEFAULTS) set on eng for the block, their defaults restored behind it whatever happens inside"""
    assert set(opts) <= set(ROUTE_DEFAULTS), sorted(set(opts) - set(ROUTE_DEFAULTS))
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        yield
    finally:
        for k in opts:
            eng.set_option(k, ROUTE_DEFAULTS[k])


def assert_big_tile(eng, M, split=None):
    """the calling thread's last GEMM ran on the 256x256 tile: all M rows, or - split = (rows256, rows128) - exactly that ragged-tail split; split = "any": all rows
    but a tail of at most 128 that the 128x128 kernel took (the shapes whose split depends on the chip's CU count)"""
    r = eng.debug_gemm_route()
    if split == "any":
        assert r["rows256"] >= 512 and r["rows256"] + r["rows128"] == M and r["rows128"] <= 128 and r["rows256"] % 256 == (0 if r["rows128"] else M % 256), (M, r)
    else:
        assert (r["rows256"], r["rows128"]) == ((M, 0) if split is None else tuple(split)), (M, split, r)
    return r


def assert_128(eng, M, shape=None):
    """the calling thread's last GEMM ran on the 128x128 kernel alone, at launch shape `shape` (0 / 1 / 2) when one is given"""
    r = eng.debug_gemm_route()
    assert r["rows256"] == 0 and r["rows128"] == M and (shape is None or r["shape128"] == shape), (M, shape, r)
    return r


# ------------------------------------------------------------------------------------------ bits
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    """both float32 as they stand (nothing is converted), the same shape, the same bit patterns"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)))


# ------------------------------------------------------------------------------------------ the log-probability reference and its bounds
def ref_log_softmax(logits):
    """float64 log-softmax of fp32 logits [.., V]"""
    l = np.asarray(logits, np.float64)
    m = l.max(axis=-1, keepdims=True)
    return l - (m + np.log(np.exp(l - m).sum(axis=-1, keepdims=True)))


def ref_logprob(logits, tok):
    """float64 log-softmax of fp32 logits [.., V] at tok [..]: l[tok] - (max + log(sum(exp(l - max)))), the value of the scalar expression bit for bit"""
    return np.take_along_axis(ref_log_softmax(logits), np.asarray(tok)[..., None].astype(np.int64), axis=-1)[..., 0]


def _bound(V, ref64, stride, per_trip):
    n_t = math.ceil(V / stride) * per_trip
    c = 3 * (math.ceil(n_t / 16) - 1) + 2 + 16 + 1
    return (n_t + c + 2.25 * math.log(V)) * U + U * np.abs(ref64)


def lp_bound(V, ref64):
    """the greedy kernel's bound (module docstring): 1024 threads, four elements per thread and trip"""
    return _bound(V, ref64, 4096, 4)


def score_bound(V, ref64):
    """the row kernel's bound: 1024 threads, sixteen elements per thread and trip"""
    return _bound(V, ref64, 16384, 16)


def check_lp(tag, lp, processed, tok):
    """lp against the float64 log-softmax of the processed scores at tok, held to lp_bound; a banned token: exactly -inf (HF's value).  Returns error / bound"""
    if np.isneginf(processed[int(tok)]):
        assert np.isneginf(lp), (tag, lp)
        return 0.0
    ref = ref_logprob(processed, tok)
    ratio = abs(float(lp) - ref) / lp_bound(len(processed), ref)
    assert np.isfinite(lp) and ratio <= 1.0, (tag, float(lp), ref, ratio)
    return ratio


# ------------------------------------------------------------------------------------------ inputs of the kernel hooks
def slabs(rows, ks, mpad=16):
    """k-split slabs [ks][mpad][V] whose fp32 sum over k, in index order, is `rows` bit for bit: exact splits of a value with a few spare mantissa bits"""
    V = rows[0].shape[0]
    w = {1: [1.0], 2: [0.5, 0.5], 3: [0.5, 0.25, 0.25]}[ks]
    s = np.zeros((ks, mpad, V), np.float32)
    for b, r in enumerate(rows):
        for k in range(ks):
            s[k, b] = r * np.float32(w[k])
    return s


# ------------------------------------------------------------------------------------------ behind the orc / golden fixtures
def load_oracle():
    from oracle import oracle
    return oracle


def load_golden(golden_dir, name="tiny_bf16.npz", int_prompts=False):
    """(npz, the two segments, their prompts) of a reference fixture; int_prompts: lists of Python ints, not the stored arrays"""
    g = np.load(os.path.join(golden_dir, name))
    segs = [synth.synth_pcm(int(g[f"s{i}_seg_index"]), int(g[f"s{i}_n_samples"])) for i in range(2)]
    prompts = [[int(t) for t in g[f"s{i}_prompt_ids"]] if int_prompts else g[f"s{i}_prompt_ids"] for i in range(2)]
    return g, segs, prompts


def forced_ids(g):
    return np.stack([g[f"s{i}_force_ids"] for i in range(2)]).astype(np.int32)
