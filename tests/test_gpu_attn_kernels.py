"""The two attention kernels of csrc/attn.hip launched the way production launches them, checked key by key.

decode_attn_kernel through sonic_test_decode_attention_cache: fused mode as decode_step() runs it (slab sum, RoPE at kv_len - 1, K / V append, kv_len - 1 keys
from the cache and the new one from LDS) and the given-q mode, both over caller-filled caches with per-row kv_len, default build and decode_attn_occ2.
flash_attn_kernel<128, causal> through sonic_test_prefill_attention: packed ragged queries, K in cache layout, V^T with the context as leading dimension.

Two kinds of check:
  * accounting, bit-exact: K = 0 makes every score 0 and every probability exactly 1 (exp(0) = 1; no fast-math in the build), V[t] is the one-hot of
    t mod 128, so output column c is count{visible t : t mod 128 == c} / n - sums of small integers, exact in fp32 in any order, one fp32 division, one
    rounding.  A dropped, repeated or unmasked key moves a column by at least a quarter of its value.
  * random and spiked data against the float64 reference with the derived bound |got - o| <= 1.5 u (A + |o|) (tests/attn_ref.py; each test prints the
    worst share of the c = 1 bound it saw).

Everything behind kv_len in K, V and V^T is large FINITE poison (+-1e4, alternating): stale cache contents in production are finite, and the kernels
legitimately multiply masked value rows by a probability of exactly 0 - NaN or infinity there would poison a correct kernel too.
"""
import numpy as np
import pytest

import attn_ref as R
from gpu_common import make_engine
from sonicscribe_amd.engine import MODE_F16

pytestmark = pytest.mark.gpu

CTX = 448                      # not a multiple of 128: the 8-wave round-robin of 16-key slices ends unevenly
SCALE = 1.0 / np.sqrt(128.0)
KINDS = ["bf16", "f16"]
MODES = ["fused", "q"]
SPIKE = 3.5                    # k = 3.5 q: score 3.5 |q|^2 / sqrt(128) ~ 40 nats above the rest for q ~ N(0, 1); values up to ~15, inside fp16's range


@pytest.fixture(scope="module")
def eng():
    e = make_engine(max_ctx=256)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng16():
    e = make_engine(mode=MODE_F16, max_ctx=256)
    yield e
    e.close()


@pytest.fixture
def E(request, eng, eng16):
    """kind -> engine, with the attention knobs back at their defaults afterwards"""
    engines = {"bf16": eng, "f16": eng16}
    yield lambda kind: engines[kind]
    for e in engines.values():
        e.set_option("decode_attn_occ2", 0); e.set_option("flash_variant", 2); e.set_option("flash_enc", 1)


def poison(shape, kind):
    n = int(np.prod(shape))
    return R.rounder(kind)(np.where(np.arange(n) % 2 == 0, 1e4, -1e4).astype(np.float32)).reshape(shape)


def one_hot_rows(n_rows, width=128):
    v = np.zeros((n_rows, width), np.float32)
    v[np.arange(n_rows), np.arange(n_rows) % width] = 1.0
    return v


def expected_counts(n_vis, kind, width=128):
    """column c of a row that sees keys 0 .. n - 1: count{t < n : t mod width == c} / n, one fp32 division, rounded to the element type"""
    n_vis = np.asarray(n_vis)
    c = np.arange(width)[None, :]
    cnt = (n_vis[:, None] - c + width - 1) // width
    return R.rounder(kind)((cnt.astype(np.float32) / n_vis[:, None].astype(np.float32)).astype(np.float32))


IDENTITY_CS = np.concatenate([np.ones((CTX, 64), np.float32), np.zeros((CTX, 64), np.float32)], axis=1)


def run_decode(e, kind, mode, kc, vc, kv_len, q, occ2=0, ksplit=1):
    """kc / vc [B][Hkv][ctx][128] hold the keys of every row INCLUDING the newest (position kv_len - 1) and poison behind; q [B][Hq][128] is the final query.
    Given-q mode: launched as is, the caches must come back untouched.  Fused mode: q and the newest K / V row travel through the slabs (all in slab 0, the
    others zero; RoPE table = identity, so the prologue passes these element-type values through unchanged) while the cache holds poison at kv_len - 1: the
    kernel has to append the row - the caches must come back equal to kc / vc, every element, poison included - and take the new key from LDS."""
    B, Hq = q.shape[:2]
    Hkv, ctx = kc.shape[1], kc.shape[2]
    e.set_option("decode_attn_occ2", occ2)
    if mode == "q":
        out, ko, vo = e.test_decode_attention_cache(kc, vc, kv_len, Hq, q=q)
    else:
        mpad = (B + 15) // 16 * 16 + 16
        slabs = np.zeros((ksplit, mpad, (Hq + 2 * Hkv) * 128), np.float32)
        slabs[:, B:] = 1e4                                        # rows no sequence owns: a mis-indexed row shows
        rows = np.arange(B)
        last = np.asarray(kv_len) - 1
        slabs[0, :B, :Hq * 128] = q.reshape(B, -1)
        slabs[0, :B, Hq * 128:(Hq + Hkv) * 128] = kc[rows, :, last].reshape(B, -1)
        slabs[0, :B, (Hq + Hkv) * 128:] = vc[rows, :, last].reshape(B, -1)
        k_in, v_in = kc.copy(), vc.copy()
        k_in[rows, :, last] = poison((B, Hkv, 128), kind); v_in[rows, :, last] = -poison((B, Hkv, 128), kind)
        cs = IDENTITY_CS if ctx == CTX else np.concatenate([np.ones((ctx, 64), np.float32), np.zeros((ctx, 64), np.float32)], axis=1)
        out, ko, vo = e.test_decode_attention_cache(k_in, v_in, kv_len, Hq, slabs=slabs, rope_cs=cs)
    bad_k, bad_v = np.argwhere(ko != kc), np.argwhere(vo != vc)
    assert bad_k.size == 0 and bad_v.size == 0, (mode, "cache differs at [b, kv head, position, dim]", bad_k[:4].tolist(), bad_v[:4].tolist())
    return out


def decode_ratio(got, q, kc, vc, kv_len, kind):
    """worst err / (u (A + |o|)) over all rows and heads, and where"""
    B, Hq = q.shape[:2]
    G = Hq // kc.shape[1]
    worst, where = 0.0, None
    for b in range(B):
        for h in range(Hq):
            o, A = R.attention(q[b, h][None], kc[b, h // G], vc[b, h // G], [kv_len[b]], SCALE)
            r = R.worst_ratio(got[b, h][None], o, A, kind)
            if r > worst:
                worst, where = r, (b, h, int(kv_len[b]))
    return worst, where


def random_caches(rng, B, Hkv, kv_len, kind, ctx=CTX, qk_scale=1.0):
    rt = R.rounder(kind)
    kc = poison((B, Hkv, ctx, 128), kind); vc = -poison((B, Hkv, ctx, 128), kind)
    for b in range(B):
        n = int(kv_len[b])
        kc[b, :, :n] = rt(rng.standard_normal((Hkv, n, 128)) * qk_scale); vc[b, :, :n] = R.values(rng, (Hkv, n, 128), kind)
    return kc, vc


# ------------------------------------------------------------------------------------------ decode attention
@pytest.mark.parametrize("occ2", [0, 1])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_decode_key_accounting(E, kind, mode, occ2):
    """every kv_len from 1 to 448, 64 rows of different lengths per launch in shuffled order"""
    e = E(kind)
    rng = np.random.default_rng(448)
    lens = rng.permutation(np.arange(1, CTX + 1))
    Hq, Hkv, B = 4, 1, 64
    rt = R.rounder(kind)
    for i in range(0, CTX, B):
        kv_len = lens[i:i + B].astype(np.int32)
        kc = poison((B, Hkv, CTX, 128), kind); vc = -poison((B, Hkv, CTX, 128), kind)
        for b in range(B):
            kc[b, 0, :kv_len[b]] = 0.0; vc[b, 0, :kv_len[b]] = one_hot_rows(int(kv_len[b]))
        q = rt(rng.standard_normal((B, Hq, 128)))
        got = run_decode(e, kind, mode, kc, vc, kv_len, q, occ2)
        want = expected_counts(kv_len, kind)
        bad = np.argwhere(got != want[:, None, :])
        assert bad.size == 0, (kind, mode, occ2, "first wrong [row, head, column]:", bad[0].tolist(), "kv_len", int(kv_len[bad[0][0]]),
                               "got", float(got[tuple(bad[0])]), "want", float(want[bad[0][0], bad[0][2]]), "wrong kv_lens", sorted(set(kv_len[bad[:, 0]].tolist()))[:16])


@pytest.mark.parametrize("kind,Hq,Hkv", [("bf16", 1, 1), ("bf16", 2, 1), ("bf16", 4, 1), ("bf16", 4, 2), ("bf16", 8, 4), ("bf16", 16, 4), ("bf16", 4, 4),
                                         ("f16", 16, 4)])
@pytest.mark.parametrize("mode", MODES)
def test_decode_gqa_maps(E, kind, mode, Hq, Hkv):
    """a different V per kv head and a different q per q head: a head that reads another's q or cache is off by O(1)"""
    e = E(kind)
    rng = np.random.default_rng(Hq * 10 + Hkv)
    B = 6
    kv_len = np.array([1, 2, 17, 129, CTX, int(rng.integers(3, CTX))], np.int32)
    kc, vc = random_caches(rng, B, Hkv, kv_len, kind)
    q = R.rounder(kind)(rng.standard_normal((B, Hq, 128)))
    outs = [run_decode(e, kind, mode, kc, vc, kv_len, q, occ2) for occ2 in (0, 1)]
    worst, where = decode_ratio(outs[0], q, kc, vc, kv_len, kind)
    print(f"decode {kind} {mode} Hq:Hkv {Hq}:{Hkv}: worst err / (u (A + |o|)) = {worst:.3f} at (row, head, kv_len) {where}")
    assert worst <= R.C_BOUND, (worst, where)
    assert np.array_equal(outs[0], outs[1]), "decode_attn_occ2 changes the bits"


def spike_cases(rng, kind):
    """rows of one launch, Hq:Hkv = 4:1, the spike built for head 1 only (the other heads keep ordinary scores, so their rescale factors differ from head 1's).
    -> kc, vc, kv_len, q, [(row, dominating key)]"""
    rt = R.rounder(kind)
    rows = []                                                     # (kv_len, [(key, factor)])
    for w in range(8):
        rows.append((300, [(16 * w + 3, SPIKE)]))                 # (a) in the first slice of each of the 8 waves
    rows.append((CTX, [(16 * 2 + 5, SPIKE / 2), (16 * (2 + 16) + 9, SPIKE)]))   # (b) wave 2: a smaller spike in its first slice, the dominant one in its third
    rows.append((333, [(331, SPIKE)]))                            # (c) the last cached key, kv_len - 2
    rows.append((333, [(332, SPIKE)]))                            # (d) the newest key, kv_len - 1 (fused mode: it comes from LDS)
    rows.append((1, [(0, SPIKE)]))
    B = len(rows)
    kv_len = np.array([r[0] for r in rows], np.int32)
    kc, vc = random_caches(rng, B, 1, kv_len, kind)
    q = rt(rng.standard_normal((B, 4, 128)))
    dom = []
    for b, (_, spikes) in enumerate(rows):
        for key, f in spikes:
            kc[b, 0, key] = rt(q[b, 1] * f)
        dom.append((b, spikes[-1][0]))
    return kc, vc, kv_len, q, dom


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_decode_rescale_and_merge(E, kind, mode):
    e = E(kind)
    rng = np.random.default_rng(40)
    kc, vc, kv_len, q, dom = spike_cases(rng, kind)
    outs = [run_decode(e, kind, mode, kc, vc, kv_len, q, occ2) for occ2 in (0, 1)]
    worst, where = decode_ratio(outs[0], q, kc, vc, kv_len, kind)
    print(f"decode {kind} {mode} spikes: worst err / (u (A + |o|)) = {worst:.3f} at (row, head, kv_len) {where}")
    assert worst <= R.C_BOUND, (worst, where)
    for b, key in dom:                                            # the dominated head is (almost) a copy of one value row
        v = vc[b, 0, key]
        assert np.all(np.abs(outs[0][b, 1] - v) <= 2 * R.U[kind] * np.abs(v)), (b, key, float(np.abs(outs[0][b, 1] - v).max()))
    assert np.array_equal(outs[0], outs[1]), "decode_attn_occ2 changes the bits"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_decode_rising_scores(E, kind, mode):
    """scores that rise with the key index (to ~34 nats for head 0, ~17 for head 2): every slice of every wave moves the running maximum"""
    e = E(kind)
    rng = np.random.default_rng(41)
    rt = R.rounder(kind)
    kv_len = np.array([CTX, 200, 37], np.int32)
    kc, vc = random_caches(rng, 3, 1, kv_len, kind, qk_scale=0.2)
    q = rt(rng.standard_normal((3, 4, 128)))
    for b in range(3):
        n = int(kv_len[b])
        ramp = (np.arange(n, dtype=np.float32) / n)[:, None]
        kc[b, 0, :n] = rt(kc[b, 0, :n] + ramp * (3.0 * q[b, 0] + 1.5 * q[b, 2])[None, :])
    got = run_decode(e, kind, mode, kc, vc, kv_len, q)
    worst, where = decode_ratio(got, q, kc, vc, kv_len, kind)
    print(f"decode {kind} {mode} rising scores: worst err / (u (A + |o|)) = {worst:.3f} at (row, head, kv_len) {where}")
    assert worst <= R.C_BOUND, (worst, where)


@pytest.mark.parametrize("kind,ksplit", [("bf16", 1), ("bf16", 2), ("bf16", 4), ("bf16", 8), ("f16", 4)])
def test_decode_fused_rope_and_append(E, kind, ksplit):
    """the fused prologue against its rounding sequence written out in numpy (attn_ref.fused_prologue): appended rows bit for bit, every other element of
    both caches as uploaded, O within the bound of the float64 attention over the cache WITH the emulated new row and the emulated q"""
    e = E(kind)
    rng = np.random.default_rng(100 + ksplit)
    Hq, Hkv = 4, 2
    pos = np.array([0, 1, 63, 64, CTX - 1, 0, CTX - 1, 127, 128] + rng.integers(2, CTX - 1, 5).tolist(), np.int32)
    pos = pos[rng.permutation(len(pos))]
    B, mpad = len(pos), 32
    kv_len = (pos + 1).astype(np.int32)
    kc, vc = random_caches(rng, B, Hkv, pos, kind)                # keys 0 .. pos - 1; poison from pos on
    slabs = rng.standard_normal((ksplit, mpad, (Hq + 2 * Hkv) * 128)).astype(np.float32) / np.sqrt(ksplit)
    if kind == "f16":                                            # value rows away from zero (attn_ref's docstring), split over the slabs
        slabs[:, :B, (Hq + Hkv) * 128:] = R.values(rng, (B, Hkv * 128), kind)[None] / ksplit + (rng.standard_normal((ksplit, B, Hkv * 128)) * 1e-3).astype(np.float32)
    slabs[:, B:] = 1e4
    cs = R.rope_table(CTX)
    q, k_new, v_new = R.fused_prologue(slabs[:, :B], cs[pos], Hq, Hkv, kind)
    out, ko, vo = e.test_decode_attention_cache(kc, vc, kv_len, Hq, slabs=slabs, rope_cs=cs)
    rows = np.arange(B)
    assert np.array_equal(ko[rows, :, pos], k_new), ("appended K rows differ; first [row, kv head, dim]", np.argwhere(ko[rows, :, pos] != k_new)[0].tolist())
    assert np.array_equal(vo[rows, :, pos], v_new), ("appended V rows differ; first [row, kv head, dim]", np.argwhere(vo[rows, :, pos] != v_new)[0].tolist())
    want_k, want_v = kc.copy(), vc.copy()
    want_k[rows, :, pos] = k_new; want_v[rows, :, pos] = v_new
    assert np.array_equal(ko, want_k) and np.array_equal(vo, want_v), ("cache touched outside the appended row", np.argwhere(ko != want_k)[:4].tolist(), np.argwhere(vo != want_v)[:4].tolist())
    worst, where = decode_ratio(out, q, want_k, want_v, kv_len, kind)
    print(f"decode {kind} fused RoPE + append ksplit {ksplit}: worst err / (u (A + |o|)) = {worst:.3f} at (row, head, kv_len) {where}")
    assert worst <= R.C_BOUND, (worst, where)
    e.set_option("decode_attn_occ2", 1)
    out2, ko2, vo2 = e.test_decode_attention_cache(kc, vc, kv_len, Hq, slabs=slabs, rope_cs=cs)
    assert np.array_equal(out2, out) and np.array_equal(ko2, ko) and np.array_equal(vo2, vo), "decode_attn_occ2 changes the bits"


@pytest.mark.parametrize("mode", MODES)
def test_decode_batch_invariance(E, mode):
    """a row's output bits depend neither on the batch size nor on its neighbours' lengths"""
    kind = "bf16"
    e = E(kind)
    rng = np.random.default_rng(64)
    B, Hq, Hkv = 64, 16, 4
    kv_len = rng.integers(1, CTX + 1, B).astype(np.int32)
    kc, vc = random_caches(rng, B, Hkv, np.full(B, CTX), kind)    # every position holds data, so any kv_len is meaningful
    q = R.rounder(kind)(rng.standard_normal((B, Hq, 128)))
    full = run_decode(e, kind, mode, kc, vc, kv_len, q)
    keep = [0, 17, 63]
    for b in keep:
        alone = run_decode(e, kind, mode, kc[b:b + 1], vc[b:b + 1], kv_len[b:b + 1], q[b:b + 1])
        assert np.array_equal(alone[0], full[b]), ("B = 1 differs from B = 64", b)
    other = rng.integers(1, CTX + 1, B).astype(np.int32)
    other[keep] = kv_len[keep]
    moved = run_decode(e, kind, mode, kc, vc, other, q)
    assert np.array_equal(moved[keep], full[keep]), "a row depends on its neighbours' kv_len"
    assert np.array_equal(run_decode(e, kind, mode, kc, vc, kv_len, q, occ2=1), full), "decode_attn_occ2 changes the bits"


# ------------------------------------------------------------------------------------------ ragged causal prefill attention
PCTX = 512
SENTINEL = 77.0


def pack(q_lens, gap=3):
    """sequences packed in reverse order with `gap` rows nobody owns in front of each: q_off is neither sorted nor dense"""
    off, q_off = gap, [0] * len(q_lens)
    for b in reversed(range(len(q_lens))):
        q_off[b] = off
        off += q_lens[b] + gap
    return np.array(q_off, np.int32), off


def run_prefill(e, q, kc, vc, q_off, q_len, kv_len, n_tok):
    """kc / vc [B][Hkv][ctx][128]; V is handed over transposed as run_prefill keeps it.  Rows outside every sequence must keep the sentinel."""
    vt = np.ascontiguousarray(vc.transpose(0, 1, 3, 2))
    init = np.full(q.shape, SENTINEL, np.float32)
    out = e.test_prefill_attention(q, kc, vt, q_off, q_len, kv_len, out_init=init)
    owned = np.zeros(n_tok, bool)
    for b in range(len(q_len)):
        owned[q_off[b]:q_off[b] + q_len[b]] = True
    assert np.all(out[~owned] == SENTINEL), ("rows outside every sequence written", np.argwhere(out[~owned] != SENTINEL)[:4].tolist())
    return out


PREFILL_SHAPES = [([1, 63, 64, 65, 130], [200, 64, 63, 1, 0]), ([264, 130, 65, 64, 1], [200, 63, 64, 0, 1])]      # (q_len, kv_len - q_len) per sequence


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_prefill_causal_accounting(E, kind, variant):
    """row t of sequence b sees keys 0 .. kv_len - q_len + t: pins the diagonal at every position across the 64-key and 128-query tile edges and the
    clipping of the tile count, with the causal offset in play"""
    e = E(kind)
    e.set_option("flash_variant", variant)
    rng = np.random.default_rng(7)
    Hq, Hkv = 4, 1
    for q_lens, offs in PREFILL_SHAPES:
        B = len(q_lens)
        q_len = np.array(q_lens, np.int32); kv_len = q_len + np.array(offs, np.int32)
        q_off, n_tok = pack(q_lens)
        kc = poison((B, Hkv, PCTX, 128), kind); vc = -poison((B, Hkv, PCTX, 128), kind)
        for b in range(B):
            kc[b, 0, :kv_len[b]] = 0.0; vc[b, 0, :kv_len[b]] = one_hot_rows(int(kv_len[b]))
        q = R.rounder(kind)(rng.standard_normal((n_tok, Hq, 128)))
        got = run_prefill(e, q, kc, vc, q_off, q_len, kv_len, n_tok)
        for b in range(B):
            n_vis = offs[b] + np.arange(q_lens[b]) + 1
            want = expected_counts(n_vis, kind)
            g = got[q_off[b]:q_off[b] + q_lens[b]]
            bad = np.argwhere(g != want[:, None, :])
            assert bad.size == 0, (kind, variant, "sequence", b, "q_len", q_lens[b], "kv_len", int(kv_len[b]), "first wrong [query, head, column]", bad[0].tolist(),
                                   "got", float(g[tuple(bad[0])]), "want", float(want[bad[0][0], bad[0][2]]), "wrong queries", sorted(set(bad[:, 0].tolist()))[:16])


def prefill_random(rng, kind, Hq, Hkv):
    rt = R.rounder(kind)
    q_lens, offs = [130, 65, 264, 1], [64, 200, 0, 300]
    B = len(q_lens)
    q_len = np.array(q_lens, np.int32); kv_len = q_len + np.array(offs, np.int32)
    q_off, n_tok = pack(q_lens)
    kc, vc = random_caches(rng, B, Hkv, kv_len, kind, ctx=PCTX)
    q = rt(rng.standard_normal((n_tok, Hq, 128)))
    dom = []
    for b in range(B):                                            # a dominant key just below the diagonal of a late query, for head 1
        t = q_lens[b] - 1 - (q_lens[b] // 5)
        key = offs[b] + t - 1
        if key >= 0:
            kc[b, 1 // (Hq // Hkv), key] = rt(q[q_off[b] + t, 1] * SPIKE)
            dom.append((b, t, key))
    return q, kc, vc, q_off, q_len, kv_len, n_tok, offs, dom


def prefill_ratio(got, q, kc, vc, q_off, q_len, offs, kind):
    Hq = q.shape[1]
    G = Hq // kc.shape[1]
    worst, where = 0.0, None
    for b in range(len(q_len)):
        n_vis = offs[b] + np.arange(q_len[b]) + 1
        for h in range(Hq):
            sl = slice(q_off[b], q_off[b] + q_len[b])
            o, A = R.attention(q[sl, h], kc[b, h // G], vc[b, h // G], n_vis, SCALE)
            r = R.worst_ratio(got[sl, h], o, A, kind)
            if r > worst:
                worst, where = r, (b, h)
    return worst, where


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("Hq,Hkv", [(16, 4), (4, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_prefill_random_and_late_dominant_key(E, kind, Hq, Hkv, variant):
    e = E(kind)
    e.set_option("flash_variant", variant)
    rng = np.random.default_rng(Hq)
    q, kc, vc, q_off, q_len, kv_len, n_tok, offs, dom = prefill_random(rng, kind, Hq, Hkv)
    got = run_prefill(e, q, kc, vc, q_off, q_len, kv_len, n_tok)
    worst, where = prefill_ratio(got, q, kc, vc, q_off, q_len, offs, kind)
    print(f"prefill {kind} {Hq}:{Hkv} flash_variant {variant}: worst err / (u (A + |o|)) = {worst:.3f} at (sequence, head) {where}")
    assert worst <= R.C_BOUND, (worst, where)
    for b, t, key in dom:
        v = vc[b, 1 // (Hq // Hkv), key]
        assert np.all(np.abs(got[q_off[b] + t, 1] - v) <= 2 * R.U[kind] * np.abs(v)), (b, t, key)


def test_prefill_default_variant_is_deterministic():
    """an engine nobody has set a knob on runs what production runs: inside the bound, the same bits on a rerun"""
    e = make_engine(max_ctx=256)
    try:
        rng = np.random.default_rng(16)
        q, kc, vc, q_off, q_len, kv_len, n_tok, offs, _ = prefill_random(rng, "bf16", 16, 4)
        a = run_prefill(e, q, kc, vc, q_off, q_len, kv_len, n_tok)
        b = run_prefill(e, q, kc, vc, q_off, q_len, kv_len, n_tok)
        worst, where = prefill_ratio(a, q, kc, vc, q_off, q_len, offs, "bf16")
        print(f"prefill bf16 16:4 default variant: worst err / (u (A + |o|)) = {worst:.3f} at (sequence, head) {where}")
        assert worst <= R.C_BOUND and np.array_equal(a, b)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------ encoder forms, accounting only
@pytest.mark.parametrize("T", [1, 64, 65, 1500])
@pytest.mark.parametrize("form", [0, 1, 3, 5, 6])
def test_encoder_key_accounting(E, form, T):
    """the same pattern (c = t mod 64) through the existing test_attention hook.  Forms 5 and 6 are included in the exact check: like the others they compute
    p = v_exp_f32(fma(s, c, -m c)), which is exactly 1 for s = m = 0, accumulate integers in fp32 and divide once (csrc/attn_enc.hip)"""
    e = E("bf16")
    e.set_option("flash_enc", form)
    rng = np.random.default_rng(T)
    B, H = 2, 2
    q = R.rounder("bf16")(rng.standard_normal((B, T, H, 64)))
    k = np.zeros((B, T, H, 64), np.float32)
    v = np.broadcast_to(one_hot_rows(T, 64)[None, :, None, :], (B, T, H, 64)).copy()
    got = e.test_attention(q, k, v, False)
    want = expected_counts(np.array([T]), "bf16", 64)[0]
    bad = np.argwhere(got != want[None, None, None, :])
    assert bad.size == 0, (form, T, "first wrong [b, query, head, column]", bad[0].tolist(), float(got[tuple(bad[0])]), float(want[bad[0][3]]))
