"""Host side of transcript scoring (sonicscribe_amd/scoring.py): packing and padding of candidates, the EOS rule, the split over several runs, the
Score record.  No GPU and no library."""
import math
import os
import re

import numpy as np
import pytest

from sonicscribe_amd import scoring, spec

EOS = spec.TINY.eos_ids


def test_scored_length_is_hf_rule():
    assert scoring.scored_length([5, 6, 7], EOS) == 3                                  # no EOS: the budget
    assert scoring.scored_length([5, EOS[1], 7, EOS[0]], EOS) == 2                     # 1 + the index of the FIRST EOS id, whichever of them
    assert scoring.scored_length([EOS[2]], EOS) == 1
    assert scoring.scored_length([5, 6, EOS[0]], EOS, budget=2) == 2                   # an EOS beyond the budget is never read
    assert scoring.scored_length([5, 6, 7], ()) == 3


def test_pack_targets_lists_and_arrays():
    a, lens = scoring.pack_targets([[1, 2, 3], [4], [5, 6]], EOS, pad_id=9)
    assert a.dtype == np.int32 and a.shape == (3, 3) and lens == [3, 1, 2]
    assert a.tolist() == [[1, 2, 3], [4, 9, 9], [5, 6, 9]]                             # [R][ld], padded beyond a sequence's own length
    arr = np.arange(8, dtype=np.int64).reshape(2, 4)
    b, lens = scoring.pack_targets(arr)
    assert b.dtype == np.int32 and b.flags["C_CONTIGUOUS"] and np.array_equal(b, arr) and lens == [4, 4]
    with pytest.raises(ValueError):
        scoring.pack_targets([[1], []])
    with pytest.raises(ValueError):
        scoring.pack_targets([])


def test_with_eos():
    assert scoring.with_eos([1, 2], EOS, True) == [1, 2, EOS[0]]
    assert scoring.with_eos([1, EOS[2]], EOS, True) == [1, EOS[2]]                     # already closed
    assert scoring.with_eos([1, 2], EOS, False) == [1, 2]
    assert scoring.with_eos([], EOS, True) == [EOS[0]]


def _check_cover(runs, cand_lens, prompt_lens, max_batch, tok_cap):
    seen = set()
    for run in runs:
        R = len(run.groups) * run.fanout
        assert 1 <= run.fanout and R <= max_batch
        tokens = 0
        for a, part in run.groups:
            assert len(part) == run.fanout                                             # dummies fill a group to the fan-out
            for c in part:
                tokens += prompt_lens[a] + (cand_lens[a][c] - 1 if c is not None else 0)
                if c is not None:
                    assert (a, c) not in seen
                    seen.add((a, c))
        assert tokens <= tok_cap
    assert seen == {(a, c) for a in range(len(cand_lens)) for c in range(len(cand_lens[a]))}   # every candidate once; the dummies are cut again


def test_plan_runs_unequal_counts_get_dummies():
    prompt_lens, cand_lens = [72, 260], [[5, 9, 3], [7]]
    runs = scoring.plan_runs(prompt_lens, cand_lens, max_batch=8, tok_cap=5000, max_ctx=1024)
    assert len(runs) == 1 and runs[0].fanout == 3
    assert runs[0].groups == [(0, [0, 1, 2]), (1, [0, None, None])]
    _check_cover(runs, cand_lens, prompt_lens, 8, 5000)
    t = scoring.run_targets(runs[0], [[[1] * 5, [2] * 9, [3] * 3], [[4] * 7]], dummy_id=0)
    assert [len(x) for x in t] == [5, 9, 3, 7, 1, 1] and t[4] == [0]


def test_plan_runs_splits_by_rows_and_tokens():
    prompt_lens, cand_lens = [100, 100, 100], [[10] * 5, [20] * 2, [4]]
    runs = scoring.plan_runs(prompt_lens, cand_lens, max_batch=4, tok_cap=100000, max_ctx=1024)      # more candidates than rows
    assert all(r.fanout == 4 for r in runs) and len(runs) == 4
    _check_cover(runs, cand_lens, prompt_lens, 4, 100000)
    runs = scoring.plan_runs(prompt_lens, cand_lens, max_batch=64, tok_cap=250, max_ctx=1024)        # rows to spare, tokens are the limit: 2 sequences per run
    assert all(r.fanout == 2 for r in runs)
    _check_cover(runs, cand_lens, prompt_lens, 64, 250)
    assert scoring.plan_runs([10], [[]], 4, 100, 64) == []
    with pytest.raises(ValueError, match="max_ctx"):
        scoring.plan_runs([60], [[5]], 4, 1000, 64)
    with pytest.raises(ValueError, match="does not fit"):
        scoring.plan_runs([60], [[50]], 4, 100, 1024)


def test_score_record():
    lp = np.array([-0.5, -1.5, -0.25], np.float32)
    s = scoring.Score("a b", [4, 5, 6], lp)
    assert s.token_ids.dtype == np.int32 and s.token_logprobs.dtype == np.float32
    assert s.sum_logprob == -2.25 and s.avg_logprob == -0.75
    assert s.top_token_ids.shape == (3, 0) and s.top_logprobs.shape == (3, 0)
    from sonicscribe_amd.engine import TokenScores
    w = scoring.Score("a", [4, 5, 6], TokenScores(lp, np.zeros((3, 2), np.float32), np.ones((3, 2), np.int32)))
    assert w.top_logprobs.shape == (3, 2) and w.top_token_ids.dtype == np.int32 and w.sum_logprob == -2.25
    assert math.isnan(scoring.Score("", [], np.zeros(0, np.float32)).avg_logprob)


def test_contract_is_documented_without_new_entry_points():
    """the feature is reached through sonic_set_option keys and the existing calls: the header names the keys beside sonic_set_forced_ids, and the engine's option
    table holds one row for each"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sonic_hip.h")).read()
    table = open(os.path.join(root, "sonicscribe_amd", "csrc", "engine_options.cpp")).read()
    for key in ("forced_parallel", "forced_fanout", "score_chunk_rows"):
        assert key in header, key
        assert len(re.findall(r'\{"%s",' % key, table)) == 1, key
    assert "rows.hip" in open(os.path.join(root, "sonicscribe_amd", "csrc", "Makefile")).read()
