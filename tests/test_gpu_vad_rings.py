"""The VAD network over audio that lies in device rings (sonic_vad_probs_rings, VADProcessor.probs_rings): every probability equals,
BIT FOR BIT, what VADProcessor.probs gives for the same int16 samples taken from the host - each is one thread's fixed-order sum over
the same values, so there is no tolerance anywhere in this file.  Ring positions put a range's start, a window's context and a window's
body across the buffer's wrap; pieces, batches, ordering behind appends, refusals, a running decode beside it, and the gate."""
import threading

import numpy as np
import pytest

from gpu_common import make_engine
from sonicscribe_amd import spec, synth, vad_net

pytestmark = pytest.mark.gpu

SEED = 7
CHUNK = 1024
LENGTHS = [1, 511, 512, 513, 10239, 10240, 7 * 16000 + 3]


@pytest.fixture(scope="module")
def vad():
    from sonicscribe_amd.vad import VADProcessor
    v = VADProcessor(weights=vad_net.synthetic_weights(SEED, **vad_net.RESPONSIVE))
    yield v
    v.close()


@pytest.fixture(scope="module")
def eng():
    e = make_engine(max_batch=2, max_ctx=512)
    yield e
    e.close()


def loud(seed, n):
    """garbage that would change every probability it leaked into"""
    return np.random.default_rng(seed).integers(-30000, 30000, size=n).astype(np.int16)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def place(eng, cap, pos, x, seed):
    """a ring of `cap` samples in which x starts at buffer position pos (mod cap), loud garbage right before and right after it;
    returns (ring, absolute index of x[0])"""
    ring = eng.ring_create(cap)
    lead = cap + (pos % cap)                       # one full lap of garbage first, so the ring has wrapped before x begins
    ring.append(loud(seed, cap))
    if lead > cap:
        ring.append(loud(seed + 1, lead - cap))
    first = ring.append(x)
    assert first == lead and first % cap == pos % cap
    tail = min(256, cap - len(x))                  # garbage behind x that does not overwrite x
    if tail > 0:
        ring.append(loud(seed + 2, tail))
    return ring, first


def test_lengths_and_wrap_positions(vad, eng):
    cap = 8 * 16000
    for k, n in enumerate(LENGTHS):
        x = synth.synth_pcm(50 + k, n)
        want = vad.probs([x])[0]
        assert len(want) == vad_net.n_windows(n)
        # across the wrap in turn: the range's start (first window's body), the second window's context, its body; then a window boundary
        # exactly at the wrap (context before, body behind), a range at the buffer's start, and no wrap inside at all
        positions = [cap - 1, cap - 480, cap - 700, cap - 512, 0, 12345]
        for j, pos in enumerate(positions):
            ring, first = place(eng, cap, pos, x, 1000 * k + 10 * j)
            got = vad.probs_rings(eng, [[(ring, first, n)]])[0]
            ring.close()
            assert np.array_equal(got, want), (n, pos)
    # the first window has no context: the same samples behind silence and behind loud garbage
    x = synth.synth_pcm(99, 2048)
    quiet = eng.ring_create(4096)
    quiet.append(np.zeros(1000, np.int16))
    a = quiet.append(x)
    noisy, b = place(eng, 4096, 1000, x, 77)
    pa, pb = vad.probs_rings(eng, [[(quiet, a, 2048)]])[0], vad.probs_rings(eng, [[(noisy, b, 2048)]])[0]
    assert np.array_equal(pa, pb) and np.array_equal(pa, vad.probs([x])[0])
    # ... and the last window is zero-padded: what follows the range in the ring does not matter
    assert np.array_equal(vad.probs_rings(eng, [[(noisy, b, 1500)]])[0], vad.probs([x[:1500]])[0])
    quiet.close(); noisy.close()


def test_multi_piece_sequences(vad, eng):
    cap = 16 * CHUNK
    ring = eng.ring_create(cap)
    ring.append(loud(1, cap - 3 * CHUNK - 100))        # the chunks below straddle the wrap
    chunks = [synth.synth_pcm(200 + i, CHUNK) for i in range(11)]
    firsts = [ring.append(c) for c in chunks]
    # the gate's ten-chunk window with one id skipped: chunks 0-3 and 5-10
    ids = [0, 1, 2, 3, 5, 6, 7, 8, 9, 10]
    want = vad.probs([np.concatenate([chunks[i] for i in ids])])[0]
    merged = [(ring, firsts[0], 4 * CHUNK), (ring, firsts[5], 6 * CHUNK)]
    single = [(ring, firsts[i], CHUNK) for i in ids]
    got = vad.probs_rings(eng, [merged, single])
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    # pieces that are no multiple of 512 (windows and contexts straddle piece boundaries), an empty piece, a tiny piece
    cuts = [(firsts[0] + 7, 700), (firsts[2], 0), (firsts[2] + 5, 1), (firsts[3], 30), (firsts[4] + 100, 1333), (firsts[7], 2 * CHUNK + 17)]
    host = np.concatenate(chunks)
    base = firsts[0]
    want = vad.probs([np.concatenate([host[a - base:a - base + n] for a, n in cuts])])[0]
    got = vad.probs_rings(eng, [[(ring, a, n) for a, n in cuts]])[0]
    assert np.array_equal(got, want)
    # pieces of two rings in one sequence; an empty sequence between two others
    other = eng.ring_create(4096)
    o = other.append(chunks[3])
    got = vad.probs_rings(eng, [[(ring, firsts[1], 800), (other, o + 10, 900)], [], [(other, o, 0)], [(other, o, CHUNK)]])
    assert np.array_equal(got[0], vad.probs([np.concatenate([chunks[1][:800], chunks[3][10:910]])])[0])
    assert len(got[1]) == 0 and len(got[2]) == 0 and np.array_equal(got[3], vad.probs([chunks[3]])[0])
    ring.close(); other.close()


def test_batch_invariance(vad, eng):
    rng = np.random.default_rng(3)
    S, n = 128, 10240
    seqs = [np.rint(synth.synth_pcm(300 + i, n) * rng.uniform(0.05, 1.0)).astype(np.int16) for i in range(S)]
    rings, firsts = [], []
    for i, x in enumerate(seqs):
        r = eng.ring_create(n + 1024)
        r.append(loud(i, int(rng.integers(1, n + 1024))))
        firsts.append(r.append(x))
        rings.append(r)
    want = vad.probs(seqs)
    batch = vad.probs_rings(eng, [[(rings[i], firsts[i], n)] for i in range(S)])
    assert same(batch, want)
    for i in range(S):
        assert np.array_equal(vad.probs_rings(eng, [[(rings[i], firsts[i], n)]])[0], want[i]), i
    perm = rng.permutation(S)
    shuffled = vad.probs_rings(eng, [[(rings[i], firsts[i], n)] for i in perm])
    assert same(shuffled, [want[i] for i in perm])
    for r in rings:
        r.close()


def test_ordering_behind_appends(vad, eng):
    # an append immediately followed by a score of those samples: no synchronise in between
    ring = eng.ring_create(60 * 16000)
    x = synth.synth_pcm(400, 50 * 16000)
    first = ring.append(x)
    assert np.array_equal(vad.probs_rings(eng, [[(ring, first, len(x))]])[0], vad.probs([x])[0])
    ring.close()
    # 200 ticks over a ring that wraps many times: each tick appends a chunk and scores the newest ten
    cap = 12 * CHUNK + 300
    ring = eng.ring_create(cap)
    rng = np.random.default_rng(5)
    hist, firsts = [], []
    for t in range(200):
        c = np.rint(synth.synth_pcm(500 + t, CHUNK) * rng.uniform(0.05, 1.0)).astype(np.int16)
        hist.append(c)
        firsts.append(ring.append(c))
        k = min(10, t + 1)
        got = vad.probs_rings(eng, [[(ring, firsts[t + 1 - k], k * CHUNK)]])[0]
        assert np.array_equal(got, vad.probs([np.concatenate(hist[t + 1 - k:])])[0]), t
    assert ring.head > 15 * cap
    ring.close()


def test_refusals(vad, eng):
    from sonicscribe_amd.engine import Engine
    from sonicscribe_amd.vad import VADProcessor
    ring = eng.ring_create(2048)
    ring.append(loud(1, 2048))
    ring.append(loud(2, 1000))                     # holds [1000, 3048)
    with pytest.raises(RuntimeError, match=r"piece 0: samples \[999, 1511\) are not in the ring \(holds \[1000, 3048\)\)"):
        vad.probs_rings(eng, [[(ring, 999, 512)]])
    with pytest.raises(RuntimeError, match=r"piece 1: samples \[3000, 3049\) are not in the ring"):
        vad.probs_rings(eng, [[(ring, 1000, 512), (ring, 3000, 49)]])
    with pytest.raises(RuntimeError, match=r"are not in the ring"):
        vad.probs_rings(eng, [[(ring, -5, 10)]])
    assert len(vad.probs_rings(eng, [[(ring, 1000, 2048)]])[0]) == 4      # the whole of what it holds is fine
    other = Engine(spec.TINY, 0, max_batch=2, max_ctx=512)
    other.load_synthetic(1)
    try:
        foreign = other.ring_create(2048)
        foreign.append(loud(3, 2048))
        with pytest.raises(RuntimeError, match="ring belongs to another engine"):
            vad.probs_rings(eng, [[(foreign, 0, 512)]])
        assert len(vad.probs_rings(other, [[(foreign, 0, 512)]])[0]) == 1
        slot = other.slot()                        # a slot sees its owner's rings
        assert len(vad.probs_rings(slot, [[(foreign, 0, 512)]])[0]) == 1
    finally:
        other.close()

    import ctypes as C
    import types
    stale = types.SimpleNamespace(h=C.c_void_p(ring.h.value), engine=eng)     # a destroyed ring: the stale handle is looked up, never dereferenced
    ring.close()
    with pytest.raises(RuntimeError, match="or was destroyed"):
        vad.probs_rings(eng, [[(stale, 1000, 512)]])
    empty = VADProcessor.__new__(VADProcessor)     # a handle without weights
    empty.lib, empty.sampling_rate, empty._lock = vad.lib, 16000, threading.Lock()
    h = C.c_void_p()
    assert vad.lib.sonic_vad_create(0, 16, C.byref(h)) == 0
    empty.h = h
    live = eng.ring_create(2048)
    live.append(loud(4, 2048))
    try:
        with pytest.raises(RuntimeError, match="sonic_vad_probs_rings: weight tensor .* not loaded"):
            empty.probs_rings(eng, [[(live, 0, 512)]])
    finally:
        empty.close()
    # nothing faulted: the handle still scores
    assert np.array_equal(vad.probs_rings(eng, [[(live, 0, 2048)]])[0], vad.probs([loud(4, 2048)])[0])
    live.close()


def test_rings_beside_decode(vad):
    """ring VAD calls while a dispatcher decodes on the rings' engine: the same bits as the host path, the same tokens as without"""
    from sonicscribe_amd import frontend
    from sonicscribe_amd.asr import ASRModel
    m = ASRModel.from_synthetic(spec.TINY, device="cuda:0", max_batch=8, max_ctx=512)
    try:
        pcms = [synth.synth_pcm(300 + i, 16000 * (2 + i % 3)) for i in range(8)]
        audio = [frontend.pcm_bytes_to_float(p.tobytes()) for p in pcms]
        alone = m.transcribe_batch(audio, 16000, max_new_tokens=24)
        rng = np.random.default_rng(8)
        seqs = [np.rint(synth.synth_pcm(i, 10240) * rng.uniform(0.05, 1.0)).astype(np.int16) for i in range(128)]
        rings = [m.model.ring_create(10240 + 512) for _ in seqs]
        for r, s in zip(rings, seqs):
            r.append(loud(9, 300))
        firsts = [r.append(s) for r, s in zip(rings, seqs)]
        want = vad.probs(seqs)
        got, res = [], []
        th = threading.Thread(target=lambda: res.append(m.transcribe_batch(audio, 16000, max_new_tokens=24)))
        th.start()
        for _ in range(10):
            got.append(vad.probs_rings(m, [[(r, f, 10240)] for r, f in zip(rings, firsts)]))
        th.join()
        assert res == [alone]
        for g in got:
            assert same(g, want)
    finally:
        m.close()


def test_gate_equivalence(vad):
    """tests/test_gpu_sessions.py's scenario through the Silero gate twice: host windows (scorer) and ring ranges (device_vad + ring_scorer)
    give the same events and the same transcripts; the device run keeps no chunk bytes on the host"""
    from sonicscribe_amd.asr import ASRModel
    from sonicscribe_amd.sessions import GatedSessions
    S = 128
    rng = np.random.default_rng(5)
    lead = rng.integers(3, 25, size=S)
    n_speech = rng.integers(18, 60, size=S)
    n_ticks = int((lead + n_speech).max()) + 45
    wire = []
    for s in range(S):
        x = np.zeros(n_ticks * CHUNK, np.int16)
        sp = synth.synth_pcm(100 + s, int(n_speech[s]) * CHUNK).astype(np.float64)
        sp = sp / max(1.0, np.abs(sp).max()) * 30000.0
        x[lead[s] * CHUNK:(lead[s] + n_speech[s]) * CHUNK] = np.rint(sp).astype(np.int16)
        wire.append(x)

    def run(device_vad):
        m = ASRModel.from_synthetic(spec.TINY, device="cuda:0", max_batch=32, max_ctx=512)
        try:
            g = GatedSessions(m, [f"client-{i}" for i in range(S)], device_vad=device_vad)
            score = vad.ring_scorer() if device_vad else vad.scorer()
            events = []
            for t in range(n_ticks):
                for s in range(S):
                    g.add_audio_chunk(s, wire[s][t * CHUNK:(t + 1) * CHUNK].tobytes(), timestamp=1000.0 + 0.064 * (t + 1))
                events.extend(g.tick(score, now=1000.0 + 0.064 * (t + 1)))
            if device_vad:
                assert all(len(r) == 0 for r in g.recent)
            out = [(e["session"], e["type"], e.get("start_chunk_id"), e.get("end_chunk_id"), e.get("first_sample"), e.get("n_samples"),
                    e["future"].result(timeout=120) if "future" in e else None) for e in events]
            g.close()
            return out
        finally:
            m.close()

    host, dev = run(False), run(True)
    assert dev == host
    kinds = [e[1] for e in host]
    assert kinds.count("speech_start") >= S // 2 and kinds.count("final") >= S // 2 and kinds.count("partial") >= S // 2
