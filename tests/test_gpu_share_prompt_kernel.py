"""The shared-prefix prefill attention (flash_attn_kernel<T, 128, true, 2, PFX>; option forced_share_prompt) through sonic_test_prefill_attention with
sonic_load_tensor "share_prompt.hook" armed: the launch goes through prefill_flash_args, the builder run_prefill uses.  Sequence b reads keys [0, pre_len[b]) from cache
row pre_row[b] and keys [pre_len[b], kv_len[b]) from its own row; query i sits at position kv_len - q_len + i.

Reference: tests/attn_ref.attention in float64 over `prefix || own keys` gathered per sequence, n_vis = kv_len - q_len + i + 1, held to the derived bound
|got - o| <= C_BOUND u (A + |o|) (attn_ref's docstring; not fitted).  Everything that must not be read is large finite poison, as in tests/test_gpu_attn_kernels.py:
a sequence's own row below pre_len and behind kv_len, an owner's row behind its kv_len - in K, and in V^T, where a 16-byte chunk of 8 keys straddles pre_len whenever
pre_len % 8 != 0.  One launch mixes the prefix lengths around the 8-key chunk and the 64-key tile, the query counts around the 64-key tile and the 128-query block
(129 and 200: a second q block, whose tile count must include the prefix), two owners, one of them between its sharers, and own keys in front of the first query."""
import numpy as np
import pytest

import attn_ref as R
from gpu_common import make_engine
from sonicscribe_amd.engine import MODE_F16, SonicError

pytestmark = pytest.mark.gpu

CTX = 512
SCALE = 1.0 / np.sqrt(128.0)
SENTINEL = 77.0
# (pre_row, pre_len, q_len, own keys in front of the first query).  Rows 0 and 7 are the owners (pre_len 0: ordinary causal sequences, 200 keys each)
SEQS = [(0, 0, 200, 0), (0, 1, 200, 0), (0, 7, 129, 0), (0, 8, 65, 0), (0, 63, 64, 0), (7, 64, 63, 0), (7, 65, 2, 0), (7, 0, 129, 71),
        (7, 130, 1, 0), (7, 200, 129, 0), (0, 200, 65, 3), (0, 130, 200, 0)]


@pytest.fixture(scope="module")
def engines():
    es = {"bf16": make_engine(max_ctx=256), "f16": make_engine(mode=MODE_F16, max_ctx=256)}
    yield es
    for e in es.values():
        e.close()


def poison(shape, kind):
    n = int(np.prod(shape))
    return R.rounder(kind)(np.where(np.arange(n) % 2 == 0, 1e4, -1e4).astype(np.float32)).reshape(shape)


def build(rng, kind, Hq, Hkv):
    rt = R.rounder(kind)
    B = len(SEQS)
    pre_row = np.array([s[0] for s in SEQS], np.int32); pre_len = np.array([s[1] for s in SEQS], np.int32)
    q_len = np.array([s[2] for s in SEQS], np.int32); kv_len = np.array([s[1] + s[3] + s[2] for s in SEQS], np.int32)
    assert kv_len.max() <= CTX and all(pre_len[b] <= kv_len[pre_row[b]] and pre_len[pre_row[b]] == 0 for b in range(B))
    off, q_off = 3, np.zeros(B, np.int32)                         # packed in reverse order with rows nobody owns in front of each
    for b in reversed(range(B)):
        q_off[b] = off
        off += q_len[b] + 3
    kc = poison((B, Hkv, CTX, 128), kind); vc = -poison((B, Hkv, CTX, 128), kind)
    for b in range(B):
        lo, hi = int(pre_len[b]), int(kv_len[b])
        kc[b, :, lo:hi] = rt(rng.standard_normal((Hkv, hi - lo, 128))); vc[b, :, lo:hi] = R.values(rng, (Hkv, hi - lo, 128), kind)
    q = rt(rng.standard_normal((off, Hq, 128)))
    return q, kc, vc, q_off, q_len, kv_len, pre_row, pre_len, off


def gathered(kc, vc, pre_row, pre_len):
    """every sequence's keys in a row of its own: prefix || own (what the unshared form would hold)"""
    km, vm = kc.copy(), vc.copy()
    for b in range(len(pre_row)):
        km[b, :, :pre_len[b]] = kc[pre_row[b], :, :pre_len[b]]; vm[b, :, :pre_len[b]] = vc[pre_row[b], :, :pre_len[b]]
    return km, vm


def launch(e, q, kc, vc, q_off, q_len, kv_len, n_tok, pre_row=None, pre_len=None):
    vt = np.ascontiguousarray(vc.transpose(0, 1, 3, 2))
    out = e.test_prefill_attention(q, kc, vt, q_off, q_len, kv_len, out_init=np.full(q.shape, SENTINEL, np.float32), pre_row=pre_row, pre_len=pre_len)
    owned = np.zeros(n_tok, bool)
    for b in range(len(q_len)):
        owned[q_off[b]:q_off[b] + q_len[b]] = True
    assert np.all(out[~owned] == SENTINEL), ("rows outside every sequence written", np.argwhere(out[~owned] != SENTINEL)[:4].tolist())
    return out


@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (16, 4)])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_shared_prefix_against_float64(engines, kind, Hq, Hkv):
    e = engines[kind]
    rng = np.random.default_rng(100 + Hq)
    q, kc, vc, q_off, q_len, kv_len, pre_row, pre_len, n_tok = build(rng, kind, Hq, Hkv)
    got = launch(e, q, kc, vc, q_off, q_len, kv_len, n_tok, pre_row, pre_len)
    km, vm = gathered(kc, vc, pre_row, pre_len)
    G = Hq // Hkv
    worst, where = 0.0, None
    for b in range(len(SEQS)):
        n_vis = kv_len[b] - q_len[b] + np.arange(q_len[b]) + 1
        sl = slice(q_off[b], q_off[b] + q_len[b])
        for h in range(Hq):
            o, A = R.attention(q[sl, h], km[b, h // G], vm[b, h // G], n_vis, SCALE)
            r = R.worst_ratio(got[sl, h], o, A, kind)
            if r > worst:
                worst, where = r, (b, h)
    print(f"shared prefix {kind} {Hq}:{Hkv}: worst err / (u (A + |o|)) = {worst:.3f} at (sequence, head) {where}")
    assert worst <= R.C_BOUND, (worst, where, SEQS[where[0]])
    # the same sequences, every one in a row of its own, through the unarmed hook (the ordinary kernel): reported, not asserted - the prefix form takes the tile that
    # holds pre_len twice, so its online softmax may round differently
    plain = launch(e, q, km, vm, q_off, q_len, kv_len, n_tok)
    same = [bool(np.array_equal(got[q_off[b]:q_off[b] + q_len[b]], plain[q_off[b]:q_off[b] + q_len[b]])) for b in range(len(SEQS))]
    print(f"shared prefix {kind} {Hq}:{Hkv}: bit-equal to the materialised sequences through the ordinary kernel, per sequence: {same}; max |d| = {np.abs(got - plain).max():.3e}")


def test_hook_is_consumed_and_validated(engines):
    e = engines["bf16"]
    rng = np.random.default_rng(5)
    q, kc, vc, q_off, q_len, kv_len, pre_row, pre_len, n_tok = build(rng, "bf16", 4, 1)
    km, vm = gathered(kc, vc, pre_row, pre_len)
    a = launch(e, q, km, vm, q_off, q_len, kv_len, n_tok)
    launch(e, q, kc, vc, q_off, q_len, kv_len, n_tok, pre_row, pre_len)
    assert np.array_equal(launch(e, q, km, vm, q_off, q_len, kv_len, n_tok), a)        # the launch before took the hook with it
    bad_row = pre_row.copy(); bad_row[3] = len(SEQS)
    with pytest.raises(SonicError, match="share_prompt.hook"):
        launch(e, q, kc, vc, q_off, q_len, kv_len, n_tok, bad_row, pre_len)
    bad_len = pre_len.copy(); bad_len[4] = kv_len[4] - q_len[4] + 1                      # a prefix that reaches the first query
    with pytest.raises(SonicError, match="share_prompt.hook"):
        launch(e, q, kc, vc, q_off, q_len, kv_len, n_tok, pre_row, bad_len)
    with pytest.raises(SonicError, match="share_prompt.hook"):
        e.arm_share_prompt_hook(pre_row[:3], pre_len[:3]); launch(e, q, kc, vc, q_off, q_len, kv_len, n_tok)   # armed for another batch size
    assert np.array_equal(launch(e, q, km, vm, q_off, q_len, kv_len, n_tok), a)        # ... and every refusal consumed it
