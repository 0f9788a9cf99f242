"""The launch table of the greedy controller (csrc/greedy.hip launch_greedy), walked in one place: the nine families {plain, LP}, GUARD x {-, LP},
BIAS x {-, LP}, SAMPLE x {plain, GUARD, BIAS} through the hooks Engine already has.  Each family's arithmetic is tested in depth elsewhere
(test_gpu_logprobs.py, test_gpu_generation_guards.py, test_gpu_request_bias.py, test_gpu_sampling_kernel.py); what this file holds is that every line of
the table launches the kernel it names: with neutral values every family is the plain family bit for bit, and every flag a family has changes the
result the way that flag must.  A wrong flag or a wrong LDS size in one line fails one of the two.

Shapes: 4 rows, 1 and 2 slabs, V = 8 (two f32x4 groups), 16388 (one group into the second trip of the 4 x 4096 loop), 59264 (the production vocabulary:
the largest three-bitmap LDS request).  Rows are uniform(-4, 4) from a fixed seed, cut to bf16 precision (test_gpu_sampling_kernel.bf16_exact): the
three SAMPLE families run in the handle's type (bf16, fp16, the fp32 kind), the other six hooks launch the bf16 kernels whatever the handle, and values
that are exact in all three types make every launch see the same scores.

Log-probabilities: DESIGN.md 6.3's derived bound (lp_bound of gpu_common.py), against float64 log_softmax of the processed scores."""
import numpy as np
import pytest

from gpu_common import SEED, check_lp, make_engine, same_bits, slabs
from sonicscribe_amd.reqbias import RequestBias
from test_gpu_request_bias import _histories  # noqa: E402
from test_gpu_sampling_kernel import bf16_exact, select  # noqa: E402

pytestmark = pytest.mark.gpu
B = 4
NEG = np.float32("-inf")
SHAPES = pytest.mark.parametrize("V,ks", [(V, ks) for V in (8, 16388, 59264) for ks in (1, 2)])
# name -> (LP, GUARD, BIAS, SAMPLE); the six bf16 hooks run on the bf16 handle, the SAMPLE families on all three
FAMILIES = {"plain": (0, 0, 0, 0), "lp": (1, 0, 0, 0), "guard": (0, 1, 0, 0), "guard_lp": (1, 1, 0, 0), "bias": (0, 1, 1, 0), "bias_lp": (1, 1, 1, 0),
            "sample": (1, 0, 0, 1), "sample_guard": (1, 1, 0, 1), "sample_bias": (1, 1, 1, 1)}
MODES = {"bf16": 0, "f16": 2, "f32": 3}


def launches(flag=None):
    """(family, handle) of every launch of the table whose family has `flag` (index into FAMILIES' tuples; None: all)"""
    out = []
    for name, f in FAMILIES.items():
        if flag is None or f[flag]:
            out += [(name, m) for m in (MODES if f[3] else ["bf16"])]
    return out


@pytest.fixture(scope="module")
def engines():
    es = {}

    def get(mode):
        if mode not in es:
            es[mode] = make_engine(mode=MODES[mode], max_batch=B)                  # the hooks take everything as arguments: no option plays a part
        return es[mode]
    yield get
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def cases():
    """(rows, slabs, hist, hlen) per shape, computed once and left unchanged"""
    memo = {}

    def get(V, ks):
        if (V, ks) not in memo:
            rng = np.random.default_rng(SEED + V)
            rows = [bf16_exact(rng.uniform(-4.0, 4.0, V)) for _ in range(B)]
            hist, hlen = _histories(V, rng)
            memo[V, ks] = (rows, slabs(rows, ks), hist, hlen)
        return memo[V, ks]
    return get


def run(engines, family, mode, s, hist, hlen, tables=None, suppress=(), temperature=None):
    """one launch of `family` -> (tokens, raw logits, log-probabilities or None, noise or None); neutral unless tables / suppress / temperature say otherwise"""
    eng = engines(mode)
    lp, guard, bias, sample = FAMILIES[family]
    if bias and tables is None:
        tables = [None, RequestBias(), None, None]                                # no table and an empty one
    if sample:
        t = [0.0] * B if temperature is None else temperature
        kw = dict(hist=hist, hist_len=hlen, tables=tables if bias else None, suppress_tokens=suppress) if guard else {}
        return eng.test_greedy_sample(s, B, t, list(range(B)), [0] * B, **kw)     # seed = row, step 0
    if bias:
        return eng.test_greedy_bias(s, B, hist, hlen, tables, suppress_tokens=suppress, want_lp=bool(lp)) + (None,)
    if guard:
        return eng.test_greedy_guard(s, B, hist, hlen, suppress_tokens=suppress, want_lp=bool(lp)) + (None,)
    if lp:
        return eng.test_greedy_lp(s, B) + (None,)
    return eng.test_greedy(s, B, want_logits=True) + (None, None)


@SHAPES
def test_neutral_identity(engines, cases, V, ks):
    """penalty 1.0, n-gram 0, no suppress list, empty tables, temperature 0: all nine families emit the plain family's tokens and dump its raw-logit bits; the
    seven with LP return the bits of test_greedy_lp (what test_neutral_guard_identity and test_rows_with_t_zero state pair by pair)"""
    rows, s, hist, hlen = cases(V, ks)
    tok0, raw0, _, _ = run(engines, "plain", "bf16", s, hist, hlen)
    _, _, lp0, _ = run(engines, "lp", "bf16", s, hist, hlen)
    assert all(same_bits(raw0[b], rows[b]) for b in range(B)), "the dump is the raw logits"
    assert tok0.tolist() == [int(np.argmax(r)) for r in rows]
    for b in range(B):
        check_lp(("lp", V, ks, b), lp0[b], raw0[b], tok0[b])
    for family, mode in launches():
        tok, raw, lp, noise = run(engines, family, mode, s, hist, hlen)
        assert np.array_equal(tok, tok0) and same_bits(raw, raw0), (family, mode, V, ks, tok.tolist(), tok0.tolist())
        if FAMILIES[family][0]:
            assert same_bits(lp, lp0), (family, mode, V, ks, lp.tolist(), lp0.tolist())
        if noise is not None:
            assert not noise.any(), (family, mode, "temperature 0 draws no noise")


@SHAPES
def test_guard_probe(engines, cases, V, ks):
    """GUARD (6 families): every row's argmax on the suppress list (one list per launch) - the token is the argmax of what is left"""
    rows, s, hist, hlen = cases(V, ks)
    sup = sorted({int(np.argmax(r)) for r in rows})
    for family, mode in launches(1):
        tok, raw, lp, _ = run(engines, family, mode, s, hist, hlen, suppress=sup)
        for b in range(B):
            proc = np.array(raw[b], np.float32)
            proc[sup] = NEG
            want = int(np.argmax(proc))
            assert int(tok[b]) == want and want not in sup, (family, mode, V, ks, b, int(tok[b]), want)
            if FAMILIES[family][0]:
                check_lp((family, mode, V, ks, b), lp[b], proc, tok[b])


@SHAPES
def test_bias_probe(engines, cases, V, ks):
    """BIAS (3 families): a length-1 entry of +100.0 on every row's lowest id - that id wins"""
    rows, s, hist, hlen = cases(V, ks)
    low = [int(np.argmin(r)) for r in rows]
    tables = [RequestBias([[[i], 100.0]]) for i in low]
    for family, mode in launches(2):
        tok, raw, lp, _ = run(engines, family, mode, s, hist, hlen, tables=tables)
        for b in range(B):
            assert int(np.argmin(raw[b])) == low[b] and int(tok[b]) == low[b], (family, mode, V, ks, b, int(tok[b]), low[b])
            if FAMILIES[family][0]:
                check_lp((family, mode, V, ks, b), lp[b], tables[b].apply(raw[b], hist[b, :hlen[b]]), tok[b])


@SHAPES
def test_sample_probe(engines, cases, V, ks):
    """SAMPLE (3 families): temperature 1.0, seed = row - noise was drawn, and the token is the first maximum of float32(raw / 1) + noise, the rule of
    test_selection_bit_for_bit; its log-probability is over the scores at temperature 1"""
    rows, s, hist, hlen = cases(V, ks)
    for family, mode in launches(3):
        tok, raw, lp, noise = run(engines, family, mode, s, hist, hlen, temperature=[1.0] * B)
        for b in range(B):
            assert noise[b].any(), (family, mode, V, ks, b)
            want, _ = select(raw[b], 1.0, noise[b])
            assert int(tok[b]) == want, (family, mode, V, ks, b, int(tok[b]), want)
            check_lp((family, mode, V, ks, b), lp[b], raw[b], tok[b])
