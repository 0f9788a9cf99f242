"""The MFMA GEMM family (csrc/gemm.hip, csrc/gemm256.hip) in the launch forms production uses, kernel by kernel, against the float64 references of
tests/gemm_ref.py: the 256x256 tile and the three launch shapes of the 128x128 kernel, row-major and fragment-tiled weights (gu8 included), pitched rows and
R == C, the ragged-tail split, the batched conv-stem forms, the q|k|v epilogue with V^T and the fused partial RoPE, and the int8 kinds with their tiled copy.

Every case asserts the kernel it means to test from the route witness (Engine.debug_gemm_route: the plan launch_gemm launched from), selected with the existing
options (gpu_common.route_options); a shape that stops reaching its kernel fails there.  (Checked once by turning the gemm_small_eff = 0 option of these tests and
of the repaired ones in test_gpu_parity.py / test_gpu_int8.py into a no-op: all 48 cases that need the option failed, each on its route assertion; the 13 that
passed reach their kernel without it - the 8320 / 8300 x 2048 grids fill the chip, q|k|v is never sent to the 128x128 kernel, four int8 shapes are small on purpose.)  The shapes are the smallest at which the code can still go wrong:
  S1 = (520, 272, 256)   big tile: four k tiles (the fewest gemm256_eligible admits), a last row tile of 8 rows, a second column tile of 16 columns;
                         128x128 kernel: launch shape 2 (32 x 32 tiles), shape 0 under gemm128_shallow
  S2 = (1040, 528, 320)  five k tiles (an odd count); 128x128 kernel: launch shape 1 (32 x 64 tiles, four-stage ring)
  SwiGLU runs them at N = 288 and 544 (shape 1 where the others take 2), int8 at K = 512 and 640 (its k tile is 128).
Bounds (gemm_ref: none is new): bias 2 ulp, GELU 3, residual 3 on |lin| + |R|, SwiGLU 4 ulp + 1e-3, the fused rotation 4 ulp of |x1 c| + |x2 s| + 1e-3; fp16 with
its own ulp.  Across routes and weight layouts one case's results are the same bits (same k order in 32-wide MFMA steps, shared epilogue arithmetic; tiling only
changes where a fragment is read from).

Two kinds of operands (operands()).  "exact": small dyadic values whose products and partial sums are exact in fp32 in any order, so the pre-activation rT(acc + bias)
is the reference's bit for bit and the epilogue alone is held to its bound.  "random": full-mantissa N(0, s) values, where fp32 accumulation order is visible - for the
claims that results are the SAME BITS across kernels and layouts (vacuous on exact data), for the plain product, whose 2-ulp bound a moved pre-activation
cannot leave (one element-type step is at most 2 ulp), and for the epilogues against the float64 reference evaluated on the kernel's OWN pre-activation (the
plain EPI_BIAS product of the same operands in the same launch form, itself held to 2 ulp of the float64 linear) at the epilogue's bound: what one moved
pre-activation step does is then on the linear's account, and the epilogue has its 3 resp. 4 ulp to itself.
Why not random data against the float64 reference everywhere: a correct kernel whose fp32 sum lands on the other side of a rounding boundary hands its epilogue a
pre-activation one element-type step away from the reference's, and the epilogues' bounds do not hold that step: near x = -2, gelu'(x) * step(x) is 2.5 x the 3-ulp
bound of gelu(x); the residual's step plus the two half-steps of the closing rounding reach 4 ulp of |lin| + |R| against a bound of 3.  Measured on MI355X with
N(0, 1.8) pre-activations: S2 bf16 GELU 1 element of 549120 at 2.36 x the bound, S2 fp16 GELU 13 at up to 3.31 x, S2 fp16 residual 1 at 1.10 x, S2 bf16 SwiGLU 1 at
1.03 x - every GELU one at a moved pre-activation (34 resp. 343 of them per case), and every output the exact GELU of the kernel's own pre-activation (bf16: the
oracle's bits on it; fp16: 0.51 of the bound)."""
import functools

import numpy as np
import pytest

import gemm_ref as R
import glue_ref as G
from attn_ref import rounder
from gpu_common import BIG_TILE, FORCE128, SHALLOW128, assert_128, assert_big_tile, bits, load_oracle, make_engine, route_options
from sonicscribe_amd import spec
from sonicscribe_amd.engine import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_QKV_VT, EPI_SWIGLU, MODE_F16, MODE_INT8, MODE_NATIVE

pytestmark = pytest.mark.gpu

F = np.float32
S1, S2 = (520, 272, 256), (1040, 528, 320)
SWIGLU_N = {272: 288, 528: 544}
SHAPE128 = {520: 2, 1040: 1}              # the launch shape the 128x128 kernel takes at its default for S1 / S2 (SwiGLU: 1 for both, it has no 32 x 32 form)
FILL = -24576.0                           # what C and V^T hold before a launch: a value of both element types that no result takes


@pytest.fixture(scope="module")
def engines():
    e = {"bf16": make_engine(mode=MODE_NATIVE, max_batch=2, max_ctx=256), "f16": make_engine(mode=MODE_F16, max_batch=2, max_ctx=256)}
    yield e
    for x in e.values():
        x.close()


@pytest.fixture(scope="module")
def eng8():
    e = make_engine(mode=MODE_INT8, max_batch=2, max_ctx=256)
    yield e
    e.close()


@pytest.fixture(scope="module")
def orc():
    return load_oracle()


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def routed(eng, opts, check, **form_args):
    """one form-hook launch under the routing options `opts`; check(eng) asserts the route from the witness before the options go back"""
    with route_options(eng, opts):
        out = eng.test_gemm_form(**form_args)
        check(eng)
    return out


def big(M, split=None):
    return lambda e: assert_big_tile(e, M, split)


def small(M, shape=None):
    return lambda e: assert_128(e, M, shape)


def untouched(buf, fill=FILL):
    return bool(np.all(bits(buf) == bits(np.full(1, fill, F))[0]))


# ------------------------------------------------------------------------------------------ the 16-bit matrix
def operands(rng, kind, data, shape, scale):
    """"exact": integers in [-4, 4] times scale rounded down to a power of two (a handful of dyadic values: products and sums of a few hundred exact in fp32);
    "random": N(0, scale) rounded to the element type"""
    if data == "exact":
        return (rng.integers(-4, 5, shape) * 2.0 ** np.floor(np.log2(scale / 2.0))).astype(F)
    return rounder(kind)((rng.standard_normal(shape) * scale).astype(F))


@functools.lru_cache(maxsize=None)
def case16(kind, M, N, K, epi, data="exact"):
    """operands and the float64-based reference of one case, made once: (A, W, bias, resid, ref, bound)"""
    rng = np.random.default_rng(1000 * epi + M + N + K + (data == "random"))
    A = operands(rng, kind, data, (M, K), 0.5); b = operands(rng, kind, data, N, 0.25)
    assert same(A, rounder(kind)(A)) and len(np.unique(A)) >= 9
    if epi == EPI_SWIGLU:
        Wg, Wu = (operands(rng, kind, data, (N // 2, K), 0.25) for _ in range(2))
        ref = R.swiglu(R.to_kind(R.linear(A, R.interleave(Wg, Wu)), kind), kind)
        assert same(ref, R.swiglu(R.to_kind(R.linear(A, R.interleave(Wg, Wu, 8)), kind), kind, gu8=True))      # the 8-row interleave names the same columns
        return A, R.interleave(Wg, Wu), None, None, ref, R.ulp_tol(ref, 4, kind) + 1e-3
    W = operands(rng, kind, data, (N, K), 0.25)
    l = R.to_kind(R.linear(A, W, b), kind)
    if epi == EPI_BIAS:
        return A, W, b, None, l, R.ulp_tol(l, 2, kind)
    if epi == EPI_BIAS_GELU:
        ref = R.gelu(l, kind)
        return A, W, b, None, ref, R.ulp_tol(ref, 3, kind)
    Rs = operands(rng, kind, data, (M, N), 1.0)
    ref, mag = R.resid(l, Rs, kind)
    return A, W, b, Rs, ref, R.ulp_tol(mag, 3, kind)


def epilogue_of(l, kind, epi, Rs=None):
    """(reference, bound) of epilogue `epi` on the pre-activation l (element-type values), at the bound the epilogue has"""
    if epi == EPI_BIAS_GELU:
        ref = R.gelu(l, kind)
        return ref, R.ulp_tol(ref, 3, kind)
    if epi == EPI_BIAS_RESID:
        ref, mag = R.resid(l, Rs, kind)
        return ref, R.ulp_tol(mag, 3, kind)
    if epi == EPI_SWIGLU:
        ref = R.swiglu(l, kind)
        return ref, R.ulp_tol(ref, 4, kind) + 1e-3
    return l, R.ulp_tol(l, 2, kind)


def routes16(M, epi):
    d128 = 1 if epi == EPI_SWIGLU else SHAPE128[M]
    return [("big", BIG_TILE, big(M)), (f"128/{d128}", FORCE128, small(M, d128)), ("128/0", SHALLOW128, small(M, 0))]


@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_SWIGLU])
@pytest.mark.parametrize("shape", [S1, S2], ids=["S1", "S2"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_matrix(engines, kind, shape, epi):
    """kind x epilogue x {256x256 tile, 128x128 kernel at each launch shape the case reaches} x {row-major, tiled (SwiGLU: also gu8)}: every result within the
    epilogue's bound of the float64 reference (random operands: of the reference on the kernel's own pre-activation), and all of one case the same bits"""
    M, N, K = shape
    N = SWIGLU_N[N] if epi == EPI_SWIGLU else N
    eng = engines[kind]
    for data in ("exact", "random"):
        A, W, b, Rs, ref, bound = case16(kind, M, N, K, epi, data)
        n_out = ref.shape[1]
        if data == "random" and epi != EPI_BIAS:      # module docstring: the epilogue's bound on the kernel's own pre-activation, that within 2 ulp of the float64 linear
            l_own = eng.test_gemm_form(A=A, W=W, bias=b, M=M, epi=EPI_BIAS)[:M]
            l64 = R.to_kind(R.linear(A, W, b), kind)
            assert (np.abs(l_own - l64) <= R.ulp_tol(l64, 2, kind)).all()
            ref, bound = epilogue_of(l_own, kind, epi, Rs)
        first = None
        for layout in ({}, {"w_tiled": 1}) + (({"w_tiled": 1, "gu8": 1},) if epi == EPI_SWIGLU else ()):
            for tag, opts, check in routes16(M, epi):
                out = routed(eng, opts, check, A=A, W=W, bias=b, resid=Rs, M=M, epi=epi, C_fill=FILL, **layout)
                assert out.shape == (M + 8, n_out) and untouched(out[M:]), (data, tag, layout)
                err = np.abs(out[:M] - ref)
                assert (err <= bound).all(), (data, tag, layout, float((err / bound).max()), int((err > bound).sum()))
                first = out if first is None else first
                assert same(out, first), (data, tag, layout, float(np.mean(out != first)))


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_identity_asymmetric_on_the_big_tile(engines, kind):
    """A made of unit rows (K = 256, M = 512: the identity, then a second, permuted one) against a W of 272 distinct rows returns columns of W exactly: a swapped
    lane or k map of the 256x256 tile cannot hide, in either weight layout"""
    eng = engines[kind]
    M, N, K = 512, 272, 256
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    W = ((n * 31 + k * 17 + (n // 251) * 7 + (k // 251) * 3 * n) % 251 / 16.0).astype(F)     # (n * 31 and k * 17 repeat mod 251: the last two terms tell row / column 251 .. apart from 0 ..)
    assert same(W, rounder(kind)(W)) and len(np.unique(W, axis=0)) == N and len(np.unique(W.T, axis=0)) == K and not np.array_equal(W[:K], W[:K].T)
    k_of = np.concatenate([np.arange(256), (3 * np.arange(256) + 1) % 256])
    A = np.zeros((M, K), F); A[np.arange(M), k_of] = 1.0
    for layout in ({}, {"w_tiled": 1}):
        out = routed(eng, BIG_TILE, big(M), A=A, W=W, M=M, epi=EPI_BIAS, C_fill=FILL, **layout)
        assert same(out[:M], W.T[k_of]) and untouched(out[M:]), layout


@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in_place"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_strides_and_aliasing(engines, kind, in_place):
    """S1 with a residual at lda = K + 64, ldc = N + 24, ldr = N + 40, and the same with R == C (o_proj, fc2, down_proj; the 256x256 tile prefetches R into
    registers before it stores): the same bits as the dense launch, and every element of the pitched C outside [0, M) x [0, N) back bit for bit"""
    eng = engines[kind]
    M, N, K = S1
    lda, ldc, ldr = K + 64, N + 24, N + 40
    junk = rounder(kind)(np.random.default_rng(5).standard_normal((M, max(lda, ldr))).astype(F) * 3)          # what lies between the rows: read by nothing
    for data in ("exact", "random"):
        A, W, b, Rs, ref, bound = case16(kind, M, N, K, EPI_BIAS_RESID, data)
        Ap = junk[:, :lda].copy(); Ap[:, :K] = A
        Rp = junk[:, :ldr].copy(); Rp[:, :N] = Rs
        Cf = np.full((M + 8, ldc), FILL, F)
        if in_place:
            Cf[:M, :N] = Rs
        dense = routed(eng, BIG_TILE, big(M), A=A, W=W, bias=b, resid=Rs, M=M, epi=EPI_BIAS_RESID)[:M]
        if data == "random":
            l_own = eng.test_gemm_form(A=A, W=W, bias=b, M=M, epi=EPI_BIAS)[:M]
            assert (np.abs(l_own - R.to_kind(R.linear(A, W, b), kind)) <= R.ulp_tol(l_own, 2, kind)).all()
            ref, bound = epilogue_of(l_own, kind, EPI_BIAS_RESID, Rs)
        assert (np.abs(dense - ref) <= bound).all(), (data, float((np.abs(dense - ref) / bound).max()))
        for tag, opts, check in routes16(M, EPI_BIAS_RESID):
            for layout in ({}, {"w_tiled": 1}):
                out = routed(eng, opts, check, A=Ap, W=W, bias=b, resid=None if in_place else Rp, M=M, epi=EPI_BIAS_RESID,
                             lda=lda, ldc=ldc, ldr=0 if in_place else ldr, resid_in_place=int(in_place), C_fill=Cf, **layout)
                assert out.shape == (M + 8, ldc)
                assert same(out[:M, :N], dense), (data, tag, layout, float(np.mean(out[:M, :N] != dense)))
                assert untouched(out[M:]) and untouched(out[:M, N:]), (data, tag, layout)


@pytest.mark.parametrize("kind,M,epi,layout", [("bf16", 8320, EPI_BIAS_RESID, {}), ("bf16", 8300, EPI_SWIGLU, {}), ("bf16", 8300, EPI_SWIGLU, {"w_tiled": 1, "gu8": 1}),
                                               ("f16", 8300, EPI_SWIGLU, {"w_tiled": 1, "gu8": 1})], ids=["resid", "swiglu", "swiglu_gu8", "swiglu_gu8_f16"])
def test_ragged_tail_split(engines, kind, M, epi, layout):
    """8320 / 8300 x 2048 x 256 (test_gemm256_path's shapes): 33 x 8 tiles would take a second round for its last row of tiles, so rows [0, 8192) run on the 256x256
    tile and the tail on the 128x128 kernel - two launches that must meet without a seam, in the tiled layouts too"""
    eng = engines[kind]
    N, K = 2048, 256
    A, W, b, Rs, ref, bound = case16(kind, M, N, K, epi)
    out = routed(eng, BIG_TILE, big(M, split=(8192, M - 8192)), A=A, W=W, bias=b, resid=Rs, M=M, epi=epi, C_fill=FILL, **layout)
    err = np.abs(out[:M] - ref)
    assert (err <= bound).all() and untouched(out[M:]), (float((err / bound).max()), np.unique(np.where(err > bound)[0] // 256).tolist())
    rng = np.random.default_rng(M + epi)                         # full-mantissa operands: the split against one 128x128 launch over all rows, bit for bit
    A = operands(rng, kind, "random", (M, K), 0.5); W = operands(rng, kind, "random", (N, K), 0.2)
    Rs = None if Rs is None else operands(rng, kind, "random", (M, N), 1.0)
    out = routed(eng, BIG_TILE, big(M, split=(8192, M - 8192)), A=A, W=W, bias=b, resid=Rs, M=M, epi=epi, C_fill=FILL, **layout)
    whole = routed(eng, FORCE128, small(M), A=A, W=W, bias=b, resid=Rs, M=M, epi=epi, C_fill=FILL, **layout)
    assert same(out, whole), float(np.mean(out != whole))
    l_own = eng.test_gemm_form(A=A, W=W, bias=b, M=M, epi=EPI_BIAS)[:M]              # and against the reference on the kernel's own pre-activation (module docstring)
    assert (np.abs(l_own - R.to_kind(R.linear(A, W, b), kind)) <= R.ulp_tol(l_own, 2, kind)).all()
    ref, bound = epilogue_of(l_own, kind, epi, Rs)
    err = np.abs(out[:M] - ref)
    assert (err <= bound).all(), (float((err / bound).max()), np.unique(np.where(err > bound)[0] // 256).tolist())


# ------------------------------------------------------------------------------------------ conv stem
@functools.lru_cache(maxsize=None)
def conv_case(kind, which, data):
    """conv1: n_mels = 128 -> C = 256 over 600 frames, stride 1; conv2: C -> C over an h1 of 1040 rows (1042 with its pad rows), stride 2, T = 520; two windows each"""
    rng = np.random.default_rng(40 + which + 2 * (data == "random"))
    Ci, T, stride = (128, 600, 1) if which == 1 else (256, 1040, 2)
    xs = operands(rng, kind, data, (2, T, Ci), 0.5); w = operands(rng, kind, data, (256, Ci, 3), 0.125); b = operands(rng, kind, data, 256, 0.25)
    buf, Wm = R.conv_operands(xs, w)
    ref = np.stack([R.gelu(R.to_kind(R.conv1d(xs[i], w, b, stride), kind), kind) for i in range(2)])
    return buf, Wm, b, ref, stride


@pytest.mark.parametrize("which", [1, 2], ids=["conv1", "conv2"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_conv_stem_forms(engines, kind, which):
    """the conv stem as run_encoder launches it: a batched GEMM (one batch per window) over overlapping rows of the padded buffer (lda < K), GELU epilogue; conv1
    writes behind the first pad row of every window of the next padded buffer.  Against the float64 sliding window; the output's pad rows come back untouched"""
    eng = engines[kind]
    for data in ("exact", "random"):                              # (module docstring: random operands are held to the reference on the kernel's own pre-activation)
        buf, Wm, b, ref, stride = conv_case(kind, which, data)
        Wn, rows, Ci = buf.shape
        M = ref.shape[1]
        form = dict(M=M, epi=EPI_BIAS_GELU, lda=stride * Ci, ldc=256, batch=Wn, strideA=rows * Ci, strideC=(rows if which == 1 else M) * 256, c_row_offset=int(which == 1),
                    gelu_arith=1)                         # run_encoder hands the conv GEMMs no GELU table
        assert (M, Wm.shape[1], form["lda"]) == ((600, 384, 128) if which == 1 else (520, 768, 512))
        first = None
        pitch, c0 = form["strideC"] // 256, form["c_row_offset"]
        if data == "random":                                      # the GELU reference on the kernel's own pre-activation: the same batched form with the plain epilogue
            l_own = eng.test_gemm_form(A=buf, W=Wm, bias=b, **{**form, "epi": EPI_BIAS, "gelu_arith": 0})
            l_own = np.stack([l_own[c0 + w * pitch:c0 + w * pitch + M] for w in range(Wn)])
            l64 = np.stack([R.to_kind(R.conv1d(buf[w, 1:-1], Wm.reshape(256, 3, Ci).transpose(0, 2, 1), b, stride), kind) for w in range(Wn)])
            assert (np.abs(l_own - l64) <= R.ulp_tol(l64, 2, kind)).all()
            ref = np.stack([R.gelu(l_own[w], kind) for w in range(Wn)])
        for tag, opts, check in (("big", BIG_TILE, big(M)), ("128", FORCE128, small(M))):
            out = routed(eng, opts, check, A=buf, W=Wm, bias=b, C_fill=FILL, **form)
            seen = np.zeros(out.shape[0], bool)
            for w in range(Wn):
                r0 = form["c_row_offset"] + w * pitch
                err = np.abs(out[r0:r0 + M] - ref[w])
                assert (err <= R.ulp_tol(ref[w], 3, kind)).all(), (data, tag, w, float((err / R.ulp_tol(ref[w], 3, kind)).max()))
                seen[r0:r0 + M] = True
            assert (~seen).sum() == (8 + 2 * Wn - 1 if which == 1 else 8) and untouched(out[~seen]), (data, tag, np.flatnonzero(~seen).tolist())
            first = out if first is None else first
            assert same(out, first), (data, tag)


# ------------------------------------------------------------------------------------------ q|k|v
QKV = dict(M=600, N=768, K=256, n_split=512, seg_T=300, vt_ld=320)      # C = 256 = four heads of 64, two windows of 300 rows; vt_ld: seg_T padded to T_PAD_ALIGN = 64


@functools.lru_cache(maxsize=None)
def qkv_case(kind, K=256, data="random"):
    rng = np.random.default_rng(77 + K + (data == "exact"))
    A = operands(rng, kind, data, (QKV["M"], K), 0.5); W = operands(rng, kind, data, (QKV["N"], K), 0.2); b = operands(rng, kind, data, QKV["N"], 0.125)
    return A, W, b, R.enc_rope_table(QKV["seg_T"])


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_qkv_vt_and_fused_rope(engines, kind):
    """EPI_QKV_VT at M = 600 = 2 x 300: tiles of both sizes straddle the segment boundary and the last is ragged.  Without the rotation (128x128 kernel; 256x256 tile
    under no_fused_rope) q|k are the bits of a plain EPI_BIAS product; with it they are held to the reference rotation, and - the epilogue rotates the ROUNDED
    linear, x = rT(acc + bias), with rope_enc_kernel's operations - they are the bits of that kernel's arithmetic on the plain product.  V^T is the exact transpose
    per segment in all three, and its pad columns [seg_T, vt_ld) come back untouched.
    Measured (MI355X), fused q|k against the reference rotation of the unrounded linear, max |err| / bound and share of elements with the reference's bits:
    random operands bf16 0.949, 87.3 %; fp16 0.817, 86.6 % (the moved pre-activations of x1 and x2 are inside the figure);
    exact operands bf16 0.907, 99.6 % (the rest: |x| >= 4, where the kernel rotates the rounded linear); fp16 0, 100 %."""
    eng = engines[kind]
    A, W, b, cs = qkv_case(kind)
    M, N, K, n_split, seg_T, vt_ld = (QKV[k] for k in ("M", "N", "K", "n_split", "seg_T", "vt_ld"))
    plain = eng.test_gemm_form(A=A, W=W, bias=b, M=M, epi=EPI_BIAS)[:M]
    lin64 = R.linear(A, W, b)
    assert (np.abs(plain - R.to_kind(lin64, kind)) <= R.ulp_tol(plain, 2, kind)).all()
    qk_plain, vt_plain = R.qkv_split(plain, n_split, seg_T)
    form = dict(A=A, W=W, bias=b, rope=cs, M=M, epi=EPI_QKV_VT, n_split=n_split, seg_T=seg_T, vt_ld=vt_ld, rope_ncols=n_split, C_fill=FILL, Vt_fill=FILL)
    runs = {"128": routed(eng, FORCE128, small(M, 0), **form),
            "big_unfused": routed(eng, {**BIG_TILE, "no_fused_rope": 1}, big(M), **form),
            "big_fused": routed(eng, BIG_TILE, big(M), **form)}
    for tag, (C, Vt) in runs.items():
        assert C.shape == (M + 8, n_split) and Vt.shape == (2, N - n_split, vt_ld) and untouched(C[M:]), tag
        assert same(Vt[:, :, :seg_T], vt_plain) and untouched(Vt[:, :, seg_T:]), (tag, float(np.mean(Vt[:, :, :seg_T] != vt_plain)))
        if tag != "big_fused":
            assert same(C[:M], qk_plain), (tag, float(np.mean(C[:M] != qk_plain)))
    got = runs["big_fused"][0][:M]
    separate = G.rope(qk_plain.reshape(M, n_split // 64, 64), cs[np.arange(M) % seg_T][:, None, :], 32, kind).reshape(M, n_split)
    assert not same(separate, qk_plain) and same(got, separate), float(np.mean(got != separate))
    # against the reference rotation of the UNROUNDED linear, on both kinds of operands
    Ax, Wx, bx, _ = qkv_case(kind, K, "exact")
    gotx = routed(eng, BIG_TILE, big(M), **{**form, "A": Ax, "W": Wx, "bias": bx})[0][:M]
    for data, g, l64 in (("random", got, lin64), ("exact", gotx, R.linear(Ax, Wx, bx))):
        ref, mag = R.rope_fused(l64[:, :n_split], cs, kind)
        ratio = np.abs(g - ref) / R.rope_bound(mag, kind)
        print(f"fused RoPE {kind} {data}: max |err| / bound = {ratio.max():.4f}, max |err| = {np.abs(g - ref).max():.6f}, {100 * np.mean(bits(g) == bits(ref)):.2f} % of the elements exact")
        assert ratio.max() <= 1.0, (data, float(ratio.max()), int((ratio > 1).sum()))


# ------------------------------------------------------------------------------------------ int8 (Linear8bitLt)
def f16(x):
    return rounder("f16")(np.asarray(x, F))


@functools.lru_cache(maxsize=None)
def case8(M, N, K, epi):
    """test_linear8bit_bias_exact's data with its planted outliers (6.0 is one, the fp16 below it is not), in groups of 260 rows"""
    orc = load_oracle()
    rng = np.random.default_rng(M + N + K + epi)
    X = f16(rng.standard_normal((M, K)) * 1.2); b = f16(rng.standard_normal(N) * 0.1)
    X[0, 3] = 6.0; X[M // 2, K - 1] = -11.5; X[M - 1, 64] = 7.25; X[M // 2, 17] = 5.99609375
    if epi == EPI_SWIGLU:
        Wg, Wu = f16(rng.standard_normal((N // 2, K)) * 0.06), f16(rng.standard_normal((N // 2, K)) * 0.06)
        gg, uu = R.linear_int8(orc, X, Wg, None, 260), R.linear_int8(orc, X, Wu, None, 260)
        ref = f16(f16(gg / (1.0 + np.exp(-gg.astype(np.float64))).astype(F)) * uu)
        return X, R.interleave(Wg, Wu), None, None, ref, 2.0 ** -9 * max(1.0, float(np.abs(ref).max()))
    W = f16(rng.standard_normal((N, K)) * 0.06)
    lin = R.linear_int8(orc, X, W, b, 260)
    if epi == EPI_BIAS:
        return X, W, b, None, lin, 0.0
    if epi == EPI_BIAS_RESID:
        Rs = f16(rng.standard_normal((M, N)))
        return X, W, b, Rs, f16(lin + Rs), 0.0
    ref = R.gelu(lin, "f16")
    return X, W, b, None, ref, 2.0 ** -10 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_SWIGLU])
@pytest.mark.parametrize("shape", [(520, 272, 512), (1040, 528, 640)], ids=["S1", "S2"])
def test_int8_matrix(eng8, shape, epi):
    """the int8 kinds on the 256x256 tile and the 128x128 kernel, from row-major codes and from the tiled copy (whose outlier columns are gathered out of the tiles):
    bias and residual bit-exact against the oracle, GELU and SwiGLU within test_linear8bit_epilogues' bounds; one case's results the same bits"""
    M, N, K = shape
    N = SWIGLU_N[N] if epi == EPI_SWIGLU else N
    X, W, b, Rs, ref, bound = case8(M, N, K, epi)
    first = None
    if epi == EPI_BIAS_GELU:                 # no tiled form: the int8 GELU epilogue walks outlier columns in row-major codes only (gemm_lin's WK), and the hook says so
        with pytest.raises(RuntimeError, match="tiled"):
            eng8.test_gemm_form(A=X, W=W, bias=b, M=M, epi=epi, group_rows=260, w_tiled=1)
    for layout in ({},) if epi == EPI_BIAS_GELU else ({}, {"w_tiled": 1}):
        for tag, opts, check in (("big", BIG_TILE, big(M)), ("128", FORCE128, small(M))):
            out = routed(eng8, opts, check, A=X, W=W, bias=b, resid=Rs, M=M, epi=epi, group_rows=260, C_fill=FILL, **layout)
            assert untouched(out[M:]), (tag, layout)
            if bound == 0.0:
                assert np.array_equal(out[:M], ref), (tag, layout, int((out[:M] != ref).sum()), float(np.abs(out[:M] - ref).max()))
            else:
                assert np.abs(out[:M] - ref).max() <= bound, (tag, layout, float(np.abs(out[:M] - ref).max()), bound)
            first = out if first is None else first
            assert same(out, first), (tag, layout, float(np.mean(out != first)))


def test_int8_ragged_tail_groups(eng8, orc):
    """the ragged-tail split of an int8 GEMM: the per-row quantisation data and the row -> group map travel with the tail rows.  Three groups, the last of them
    (rows 8300 ..) wholly inside the tail, each with outlier columns of its own"""
    M, N, K, G3 = 8320, 2048, 512, 4150
    rng = np.random.default_rng(83)
    X = f16(rng.standard_normal((M, K)) * 1.2); W = f16(rng.standard_normal((N, K)) * 0.06); b = f16(rng.standard_normal(N) * 0.1)
    X[7, 3] = 6.0; X[5000, K - 1] = -11.5; X[8200, 64] = 7.25; X[8310, 17] = 9.5; X[8301, 200] = 5.99609375
    ref = R.linear_int8(orc, X, W, b, G3)
    for layout in ({}, {"w_tiled": 1}):
        out = routed(eng8, BIG_TILE, big(M, split=(8192, 128)), A=X, W=W, bias=b, M=M, epi=EPI_BIAS, group_rows=G3, C_fill=FILL, **layout)
        assert np.array_equal(out[:M], ref) and untouched(out[M:]), (layout, np.unique(np.where(out[:M] != ref)[0] // 128).tolist())


def test_int8_long_outlier_lists_from_the_tiled_copy(eng8, orc):
    """test_linear8bit_long_outlier_lists_go_to_the_dense_side_product's case on the 256x256 tile (the only kernel with a DEFER instantiation) reading the tiled copy,
    as the decoder's o_proj and down_proj do in an int8 prefill: the same one-ulp bound on the deferred request, the short list exact"""
    rng = np.random.default_rng(99)
    M, N, K, Gr = 520, 256, 512, 260
    assert (2 * spec.TINY.enc_T + 128) * spec.TINY.enc_d >= M * N          # the engine's deferral buffer (engine.cpp: defer_cap) holds the rows; else nothing is deferred
    X = f16(rng.standard_normal((M, K))); W = f16(rng.standard_normal((N, K)) * 0.08); b = f16(rng.standard_normal(N) * 0.1)
    Rs = f16(rng.standard_normal((M, N)))
    X[rng.integers(0, Gr, 70), rng.choice(K, 70, replace=False)] = f16(rng.choice([-1.0, 1.0], 70) * rng.uniform(6.0, 14.0, 70))
    X[Gr + rng.integers(0, Gr, 5), rng.choice(K, 5, replace=False)] = f16(rng.uniform(6.5, 9.0, 5))
    lin = R.linear_int8(orc, X, W, b, Gr)
    ref = f16(lin + Rs)
    ulp16 = lambda v: np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14))) - 10), 2.0 ** -24)
    ulp = ulp16(lin) + ulp16(ref)
    for in_place in (False, True):
        Cf = np.full((M + 8, N), FILL, F)
        if in_place:
            Cf[:M] = Rs
        out = routed(eng8, BIG_TILE, big(M), A=X, W=W, bias=b, resid=None if in_place else Rs, resid_in_place=int(in_place), M=M, epi=EPI_BIAS_RESID, group_rows=Gr,
                     w_tiled=1, C_fill=Cf)
        assert eng8.debug_gemm_route()["deferred"] == 1           # the linear did hand request 0 to the side product (else the result would be exact and prove nothing)
        diff = np.abs(out[:M] - ref)
        assert (diff <= ulp).all() and np.array_equal(out[Gr:M], ref[Gr:]) and float((diff[:Gr] > 0).mean()) < 0.02 and untouched(out[M:]), (in_place, float((diff / ulp).max()))


def test_int8_qkv_fused_equals_the_separate_passes(eng8):
    """the int8 encoder's q|k|v (K = 512: four int8 k tiles): RoPE on the staged tile and V^T inside the GEMM against i8_no_qkv_fuse, rope_enc_kernel and a transpose"""
    A, W, b, cs = qkv_case("f16", 512)
    M, N, n_split, seg_T, vt_ld = (QKV[k] for k in ("M", "N", "n_split", "seg_T", "vt_ld"))
    form = dict(A=A, W=W, bias=b, rope=cs, M=M, epi=EPI_QKV_VT, n_split=n_split, seg_T=seg_T, vt_ld=vt_ld, rope_ncols=n_split, C_fill=FILL, Vt_fill=FILL)
    C, Vt = routed(eng8, BIG_TILE, big(M), **form)
    Cu, Vtu = routed(eng8, {**BIG_TILE, "i8_no_qkv_fuse": 1}, big(M), **form)
    assert C.shape == Cu.shape == (M + 8, N) and untouched(C[M:]) and untouched(Cu[M:]) and untouched(C[:M, n_split:]) and untouched(Vtu)
    qk = eng8.test_rope_enc(np.ascontiguousarray(Cu[:M, :n_split]), seg_T, n_split // 64, 32, cs)
    assert not same(qk, Cu[:M, :n_split]) and same(C[:M, :n_split], qk), float(np.mean(C[:M, :n_split] != qk))
    _, vt_ref = R.qkv_split(Cu[:M], n_split, seg_T)
    assert same(Vt[:, :, :seg_T], vt_ref) and untouched(Vt[:, :, seg_T:])
