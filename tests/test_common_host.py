"""The shared test helpers (tests/gpu_common.py, tests/abi_pins.py) pinned on the CPU: they carry every GPU file's tolerances and references, so each is held
here to an independent statement of what it must be.  No GPU."""
import math

import numpy as np
import pytest

import abi_pins
import gpu_common as C
from sonicscribe_amd import spec


@pytest.mark.parametrize("V,n_t,trips", [(1024, 4, 1), (4096, 4, 1), (4100, 8, 1), (59264, 60, 4), (70000, 72, 5)])
def test_lp_bound_is_design_6_3(V, n_t, trips):
    """DESIGN.md 6.3 written out: each of 1024 threads adds four elements per 4096-wide stride (n_t adds), the loop is unrolled four strides to a trip and every
    trip after the first rescales the running sum (3 roundings), then 2 + 16 + 1 and the exp arguments' 2.25 ln V, all in units of u = 2^-24, plus u |ref64|"""
    u = 1.0 / (1 << 24)
    strides = -(-V // 4096)
    assert 4 * strides == n_t and -(-strides // 4) == trips
    for ref64 in (0.0, -0.5, -30.0):
        want = (n_t + 3 * (trips - 1) + 2 + 16 + 1 + 2.25 * math.log(V)) * u + u * abs(ref64)
        assert C.lp_bound(V, ref64) == want
    assert C.lp_bound(V, np.array([-0.5, -30.0])).tolist() == [C.lp_bound(V, -0.5), C.lp_bound(V, -30.0)]
    assert C.U == u and C.SEED == 20260128


def test_same_bits_and_bits():
    f = np.float32
    nan_a, nan_b = np.array([0x7FC00000, 0x7FC00001], np.uint32).view(f)
    assert not C.same_bits(np.array([0.0], f), np.array([-0.0], f))
    assert not C.same_bits(np.array([nan_a], f), np.array([nan_b], f))
    assert C.same_bits(np.array([nan_a, 1.5], f), np.array([nan_a, 1.5], f))
    assert not C.same_bits(np.array([1.0], f), np.array([1.0], np.float64)) and not C.same_bits(np.array([1.0], np.float64), np.array([1.0], np.float64))
    assert not C.same_bits(np.zeros(3, f), np.zeros((3, 1), f))
    assert C.same_bits(f(2.5), f(2.5)) and not C.same_bits([1.0], [1.0])               # scalars of the type pass; a list of Python floats is float64
    assert C.bits(np.array([1.0, -0.0], f)).tolist() == [0x3F800000, 0x80000000] and C.bits(np.zeros((4, 2), f)[:, 0]).dtype == np.uint32


@pytest.mark.parametrize("V", [8, 1000, 59264])
def test_ref_logprob_is_the_scalar_expression(V):
    rng = np.random.default_rng(V)
    rows = rng.uniform(-8, 8, (3, V)).astype(np.float32)
    rows[1, : V // 2] = -np.inf                                                       # banned ids: exp gives 0, the sum skips them
    tok = np.array([0, V - 1, V // 3])

    def scalar(row, t):
        l = np.asarray(row, np.float64)
        m = l.max()
        return l[int(t)] - (m + np.log(np.exp(l - m).sum()))

    want = np.array([scalar(rows[b], tok[b]) for b in range(3)])
    got = C.ref_logprob(rows, tok)
    assert got.dtype == np.float64 and got.shape == (3,) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    for b in range(3):
        one = C.ref_logprob(rows[b], tok[b])
        assert np.ndim(one) == 0 and np.float64(one).view(np.uint64) == want[b].view(np.uint64)
        assert np.array_equal(C.ref_log_softmax(rows[b])[tok[b]:tok[b] + 1].view(np.uint64), want[b:b + 1].view(np.uint64))
    assert np.array_equal(C.ref_logprob(rows[None], tok[None]).view(np.uint64), want[None].view(np.uint64))      # [1, 3, V]: any leading shape


@pytest.mark.parametrize("ks", [1, 2, 3])
def test_slabs_sum_back_to_the_rows(ks):
    rng = np.random.default_rng(ks)
    rows = [rng.uniform(-300, 300, 1000).astype(np.float32), np.full(1000, np.float32(1.5)), (-3.0e4 + rng.uniform(-300, 300, 1000)).astype(np.float32)]
    for mpad in (16, 32):
        s = C.slabs(rows, ks, mpad) if mpad != 16 else C.slabs(rows, ks)
        assert s.shape == (ks, mpad, 1000) and s.dtype == np.float32 and not s[:, 3:].any()
        acc = np.zeros((mpad, 1000), np.float32)
        for k in range(ks):
            acc = acc + s[k]
        assert acc.dtype == np.float32 and all(C.same_bits(acc[b], rows[b]) for b in range(3))


def test_prompt_for():
    d = spec.TINY
    a = d.audio_token_id
    assert spec.audio_token_count(spec.valid_frames(48000)) == 37 and spec.audio_token_count(spec.valid_frames(200000)) == 156
    assert C.prompt_for(d, 48000) == [1, 17, 23, 5] + [a] * 37 + [7, 301, 302, 303, 9, 11]
    assert C.prompt_for(d, 200000) == [1, 17, 23, 5] + [a] * 156 + [7, 301, 302, 303, 9, 11]
    count = lambda n: spec.audio_token_count(spec.valid_frames(n))
    # the local functions this one replaced, as they were written
    assert C.prompt_for(d, 80000, tail=(9, 8)) == [1, 17, 23, 5] + [a] * count(80000) + [7, 301, 302, 303, 9, 11] + list((9, 8))          # test_gpu_pipeline_native.py
    assert C.prompt_for(d, 64000, suffix=(7, 301, 9)) == [1, 17, 23, 5] + [a] * count(64000) + list((7, 301, 9))                          # test_gpu_slots.py
    assert C.prompt_for(d, [80000, 64000]) == [1, 17, 23, 5] + [a] * sum(count(s) for s in [80000, 64000]) + [7, 301, 302, 303, 9, 11]    # test_gpu_forks.py
    assert C.prompt_for(d, [48000]) == C.prompt_for(d, 48000) == C.prompt_for(d, np.int64(48000))
    assert C.prompt_for(d, 48000, prefix=[3], suffix=[4]) == [3] + [a] * 37 + [4]
    segs, prompts = C.six()
    assert [len(s) for s in segs] == [48000, 200000, 80000, 64000, 120000, 96000] and prompts == [C.prompt_for(d, len(s)) for s in segs]


def test_flags_keep_their_order():
    assert C.flags((1, "a", 1), (0, "b", 2), ({"x": 1}, "generation", {"x": 1}), (None, "c", 3), (8, "d", 8)) == [("a", 1), ("generation", {"x": 1}), ("d", 8)]


class _RouteEngine:
    """what route_options and the route assertions use of an Engine: set_option and debug_gemm_route"""
    def __init__(self, route):
        self.route, self.calls = dict(zip(("rows256", "rows128", "shape128", "cus"), route)), []

    def set_option(self, key, value):
        self.calls.append((key, value))

    def debug_gemm_route(self):
        return dict(self.route)


def test_route_options_restore_and_route_assertions_refuse():
    """the options of the GEMM tests go back to the library's defaults (csrc/common.h LaunchOpts, engine_options.cpp) even when the block raises, and each route
    assertion refuses every route but the one it names - a test whose shape stopped reaching its kernel fails instead of passing on the other one"""
    assert C.ROUTE_DEFAULTS == {"gemm_small_eff": 75, "gemm_force128": 0, "gemm128_shallow": 0, "no_fused_rope": 0, "i8_no_qkv_fuse": 0}
    src = open(abi_pins.CSRC + "/common.h").read()
    assert "int gemm_small_eff = 75;" in src and "int gemm_force128 = 0;" in src and "int gemm128_shallow = 0;" in src
    e = _RouteEngine((0, 0, 0, 256))
    with pytest.raises(RuntimeError):
        with C.route_options(e, C.SHALLOW128):
            raise RuntimeError("inside")
    assert e.calls == [("gemm_force128", 1), ("gemm128_shallow", 1), ("gemm_force128", 0), ("gemm128_shallow", 0)]
    with pytest.raises(AssertionError):
        with C.route_options(e, {"no_such_route_option": 1}):
            pass
    assert (C.BIG_TILE, C.FORCE128) == ({"gemm_small_eff": 0}, {"gemm_force128": 1})
    big, small, split = _RouteEngine((520, 0, 0, 256)), _RouteEngine((0, 520, 2, 256)), _RouteEngine((8192, 128, 0, 256))
    assert C.assert_big_tile(big, 520)["rows256"] == 520 and C.assert_128(small, 520, 2)["shape128"] == 2 and C.assert_128(small, 520)
    C.assert_big_tile(split, 8320, split=(8192, 128)); C.assert_big_tile(split, 8320, split="any"); C.assert_big_tile(big, 520, split="any")
    for fn in (lambda: C.assert_big_tile(small, 520), lambda: C.assert_big_tile(small, 520, split="any"), lambda: C.assert_big_tile(split, 8320),
               lambda: C.assert_big_tile(big, 520, split=(512, 8)), lambda: C.assert_big_tile(big, 521, split="any"), lambda: C.assert_128(big, 520),
               lambda: C.assert_128(small, 520, 1), lambda: C.assert_128(split, 8320), lambda: C.assert_128(small, 519)):
        with pytest.raises(AssertionError):
            fn()


def test_check_surface_and_that_it_checks(monkeypatch):
    abi_pins.check_surface()
    abi_pins.check_surface(names=("sonic_set_option",), options=("token_logprobs",), header_strings=("SONIC_API",), engine_methods=("set_option",))
    for bad in (dict(names=("sonic_no_such_entry",)), dict(options=("no_such_option",)), dict(header_strings=("no such words in the header",)),
                dict(engine_methods=("no_such_method",))):
        with pytest.raises(AssertionError):
            abi_pins.check_surface(**bad)
    monkeypatch.setattr(abi_pins, "N_EXPORTS", abi_pins.N_EXPORTS + 1)
    with pytest.raises(AssertionError):
        abi_pins.check_surface()
    monkeypatch.undo()
    monkeypatch.setattr(abi_pins, "ABI_VERSION", abi_pins.ABI_VERSION + 1)
    with pytest.raises(AssertionError):
        abi_pins.check_surface()
