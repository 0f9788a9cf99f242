"""Word timestamps, host side: tests/align_ref.py - the numpy restatement the GPU tests compare against - checked on cases whose answer is
known by hand, sonicscribe_amd/timestamps.py against it, the unpacking of an align run's records, and ASRModel's refusals that need no device."""
import numpy as np
import pytest

import align_ref as R
from sonicscribe_amd import spec, timestamps
from sonicscribe_amd.engine import AlignedScores, TokenScores, unpack_logprobs

F = np.float32


def staircase(L, A, f):
    """M with 1 on (n, a) for f[n] <= a < f[n + 1] and -1 elsewhere"""
    M = -np.ones((L, A), F)
    edges = list(f) + [A]
    for n in range(L):
        M[n, edges[n]:edges[n + 1]] = 1
    return M


def test_planted_staircase_is_recovered_exactly():
    f = [0, 2, 3, 7, 8, 12]
    assert np.array_equal(R.times_of(staircase(6, 15, f)), f)
    text, audio = R.dtw_f32(staircase(6, 15, f))
    assert np.all(np.diff(text) >= 0) and np.all(np.diff(audio) >= 0) and (text[0], audio[0], text[-1], audio[-1]) == (0, 0, 5, 14)
    assert np.all((np.diff(text) + np.diff(audio)) >= 1) and np.all(np.diff(text) <= 1) and np.all(np.diff(audio) <= 1)


def test_one_row():
    p = np.random.default_rng(1).random((3, 1, 9))
    assert np.array_equal(R.normalise(p), np.zeros_like(p))                  # std = 0 over one row: z = 0, not Whisper's nan
    assert np.array_equal(R.matrix(p), np.zeros((1, 9)))
    assert np.array_equal(R.times_of(np.zeros((1, 9), F)), [0])


@pytest.mark.parametrize("A", [1, 3, 4])
def test_median_filter_edge(A):
    z = np.random.default_rng(A).standard_normal((5, A))
    got = R.median_filter(z)
    if A <= 3:
        assert np.array_equal(got, z)                                        # passes unchanged (whisper/timing.py::median_filter)
        return
    # A = 4, by hand: reflect padding of [a b c d] by 3 is [d c b | a b c d | c b a]
    for r in range(5):
        a, b, c, d = z[r]
        want = [np.median([d, c, b, a, b, c, d]), np.median([c, b, a, b, c, d, c]), np.median([b, a, b, c, d, c, b]), np.median([a, b, c, d, c, b, a])]
        assert np.array_equal(got[r], want)


def test_all_equal_matrix_follows_the_tie_rule():
    # every cell costs the same, so every comparison between finite costs of equal path length ties and the rule decides: c0 needs to be STRICTLY below both others,
    # else c1 strictly below both, else c2.  Column 1 can only come from above (c1); row 1 beyond column 1 only from the left (c2); inside, cost[i][j] = -(i + j - 1)
    # and c0 = -(i + j - 3) is never the smallest, c1 = c2: the rule says c2.  Walking back from (3, 4): left, left, left in row 3 until column 1, then up, up.
    text, audio = R.dtw_f32(np.ones((3, 4), F))
    assert list(zip(text, audio)) == [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (2, 3)]
    assert np.array_equal(R.times_of(np.ones((3, 4), F)), [0, 0, 0])
    assert np.array_equal(R.times_of(np.zeros((3, 4), F)), [0, 0, 0])


def test_more_rows_than_columns():
    M = staircase(3, 3, [0, 1, 2])
    M = np.repeat(M, 2, axis=0)                                              # 6 rows over 3 columns: two rows per column
    t = R.times_of(M)
    assert np.array_equal(t, [0, 0, 1, 1, 2, 2]) and np.all(np.diff(t) >= 0)


def test_two_windows_second_starts_at_30_s():
    n = 40 * 16000
    total, per_win = spec_counts(n)
    assert len(per_win) == 2 and total == sum(per_win)
    idx = np.array([0, per_win[0] - 1, per_win[0], per_win[0] + 5, total - 1])
    want = [0.0, (per_win[0] - 1) * 0.08, 30.0, 30.0 + 5 * 0.08, 30.0 + (per_win[1] - 1) * 0.08]
    assert np.allclose(R.index_seconds(idx, per_win), want, rtol=0, atol=1e-12)
    assert np.allclose(timestamps.audio_index_seconds(idx, per_win, total), want, rtol=0, atol=1e-12)
    # placeholder count and per-window rows disagree: the rule is the run's own, i * 0.08
    assert np.allclose(timestamps.audio_index_seconds(idx, per_win, total + 1), idx * 0.08, rtol=0, atol=1e-12)
    s, e = timestamps.token_spans([0.0, 1.0, 1.0, 31.0], 40.0)
    assert np.array_equal(s, [0.0, 1.0, 1.0, 31.0]) and np.array_equal(e, [1.0, 1.0, 31.0, 40.0])


def spec_counts(n):
    from sonicscribe_amd import frontend
    return frontend.request_audio_tokens(n, spec.FULL)


def test_word_grouping():
    pieces = [" he", "llo", ",", " wor", "ld", " 世", "界", "ok", " สวัส", " 가", "x"]
    want = [[0, 1, 2], [3, 4], [5], [6], [7], [8], [9], [10]]
    assert R.group_words(pieces) == want
    got = timestamps.group_words([(t, [i]) for i, t in enumerate(pieces)])
    assert [w[1] for w in got] == want and got[0][0] == " hello," and sorted(sum((w[1] for w in got), [])) == list(range(len(pieces)))
    # pieces that do not yet decode to valid text merge forward
    table = {(1,): "�", (1, 2): " é", (3,): "t", (4,): "�"}
    sp = timestamps.split_pieces([1, 2, 3, 4], lambda ids: table[tuple(ids)])
    assert sp == [(" é", [0, 1]), ("t", [2]), ("�", [3])]
    al = timestamps.build_alignment([5, 6, 7, 2], [-0.1, -0.3, -0.2, -0.5], [0, 3, 3, 9], [2], [10], 10, 0.8, lambda ids: [(" a", [0]), ("b", [1]), (" c", [2])])
    assert al.token_ids.tolist() == [5, 6, 7] and np.allclose(al.token_start, [0, 0.24, 0.24]) and np.allclose(al.token_end, [0.24, 0.24, 0.8])      # EOS dropped
    assert [(w.word, w.tokens) for w in al.words] == [("ab", [0, 1]), ("c", [2])]
    assert al.words[0].probability == pytest.approx(np.exp(-0.2)) and (al.words[0].start, al.words[0].end) == (0.0, pytest.approx(0.24))
    sh = al.shifted(12.5)
    assert sh.words[1].start == pytest.approx(12.74) and sh.token_end[-1] == pytest.approx(13.3)


@pytest.mark.parametrize("K", [0, 8])
def test_unpack_align_records(K):
    n, W = 5, 1 + 2 * K + 1
    rng = np.random.default_rng(K)
    rec = rng.standard_normal((n + 2, W)).astype(F)
    rec[:, 1 + K:1 + 2 * K] = rng.integers(0, 1000, (n + 2, K))
    rec[:, W - 1] = rng.integers(0, 375, n + 2)
    got = unpack_logprobs(rec.reshape(-1), n, K, align=True)
    assert isinstance(got, AlignedScores) and got.times.dtype == np.int32
    assert np.array_equal(got.lp, rec[:n, 0]) and np.array_equal(got.times, rec[:n, W - 1].astype(np.int32))
    assert got.top_logprobs.shape == (n, K) and np.array_equal(got.top_logprobs, rec[:n, 1:1 + K]) and np.array_equal(got.top_ids, rec[:n, 1 + K:1 + 2 * K].astype(np.int32))
    # the narrow records are unpacked as before
    narrow = np.ascontiguousarray(rec[:, :W - 1]).reshape(-1)
    old = unpack_logprobs(narrow, n, K)
    assert (isinstance(old, TokenScores) and np.array_equal(old.lp, got.lp)) if K else np.array_equal(old, got.lp)


def test_constructor_refusals():
    from sonicscribe_amd.asr import ASRModel
    with pytest.raises(ValueError, match="timestamps=True needs scoring=True"):
        ASRModel.from_synthetic(spec.TINY, token_logprobs=True, timestamps=True)      # raised before any device work: passes on a machine without a GPU
    with pytest.raises(ValueError, match="alignment_heads needs timestamps=True"):
        ASRModel.from_synthetic(spec.TINY, token_logprobs=True, scoring=True, alignment_heads=[[0, 0]])
    with pytest.raises(ValueError, match=r"alignment_heads\[0\] = \[2, 0\] is outside the decoder"):
        ASRModel.from_synthetic(spec.TINY, token_logprobs=True, scoring=True, timestamps=True, alignment_heads=[[2, 0]])
    with pytest.raises(ValueError, match="not a \\[layer, head\\] pair"):
        timestamps.check_timestamps(True, True, [[1]])
    assert timestamps.check_timestamps(True, True, [[1, 0], (1, 0), [0, 1]], 2, 2) == [(1, 0), (0, 1)]
    assert timestamps.check_timestamps(False, False, None) is None


def test_kernel_test_seeds_stay_within_the_thin_cap():
    """the GPU kernel test leaves thin columns out of the M comparison; the restatement alone shows that its seeds draw at most THIN_CAP of them, and that the
    planted alignment is recovered by the restated pipeline itself"""
    for kind in ("bf16", "f16"):
        for shape in R.KERNEL_SHAPES:
            q, k = R.kernel_data(shape, kind)
            for b in range(shape[0]):
                r = R.matrix_bound(q[b], k[b])
                assert r["thin_share"] <= R.THIN_CAP, (kind, shape, b, r["thin_share"])
                assert np.allclose(r["M"], R.matrix(r["p"]), rtol=0, atol=1e-9)
        q, k, f = R.planted(17, 4, 2, kind)
        assert np.array_equal(R.times_of(R.matrix_bound(q[0], k[0])["M"].astype(F)), f)
    assert {s[1] for s in R.KERNEL_SHAPES} == {1, 2, 17, 65} and {s[2] for s in R.KERNEL_SHAPES} == {1, 3, 4, 7, 16, 65, 375}
    assert {s[0] for s in R.KERNEL_SHAPES} == {1, 3} and {s[3:] for s in R.KERNEL_SHAPES} == {(2, 1), (4, 2)}
