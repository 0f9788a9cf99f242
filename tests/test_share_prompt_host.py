"""Host side of the shared prompt prefill (option forced_share_prompt; scoring.plan_runs(share_prompt=True), ASRModel's defaults and refusals): the
surface the feature travels through - an option row and named strings, no export - and the split of candidates over runs when a group prefills its prompt once.
No GPU."""
import pytest

import abi_pins
from sonicscribe_amd import scoring


def test_surface_adds_no_entry_point():
    abi_pins.check_surface(options=("forced_share_prompt",), header_strings=("share_prompt.hook", "score_tokens"))


def shared_tokens(run, prompt_lens, cand_lens):
    """what the engine charges a shared run: per group P + sum(L - 1) over its real candidates (a dummy is one target: no row)"""
    return sum(prompt_lens[a] + sum(cand_lens[a][c] - 1 for c in part if c is not None) for a, part in run.groups)


def check_cover(runs, prompt_lens, cand_lens, max_batch, tok_cap):
    seen = []
    for run in runs:
        assert 1 <= run.fanout and len(run.groups) * run.fanout <= max_batch
        assert all(len(part) == run.fanout and part[0] is not None for _, part in run.groups)      # a group's first sequence, the one that packs the prompt, is real
        assert shared_tokens(run, prompt_lens, cand_lens) <= tok_cap
        seen += [(a, c) for a, part in run.groups for c in part if c is not None]
    assert sorted(seen) == [(a, c) for a in range(len(cand_lens)) for c in range(len(cand_lens[a]))]


def test_token_accounting_and_dummies():
    prompt_lens, cand_lens = [72, 260], [[5, 9, 3], [7]]
    runs = scoring.plan_runs(prompt_lens, cand_lens, max_batch=8, tok_cap=5000, max_ctx=1024, share_prompt=True)
    assert len(runs) == 1 and runs[0].groups == [(0, [0, 1, 2]), (1, [0, None, None])]
    assert shared_tokens(runs[0], prompt_lens, cand_lens) == 72 + 4 + 8 + 2 + 260 + 6
    # the two dummies cost nothing: with room for exactly those tokens the plan is one run; unshared, the same list needs 3 * 72 + 14 + 3 * 260 + 6
    tight = scoring.plan_runs(prompt_lens, cand_lens, max_batch=8, tok_cap=72 + 14 + 260 + 6, max_ctx=1024, share_prompt=True)
    assert len(tight) == 1 and tight[0].fanout == 3
    check_cover(tight, prompt_lens, cand_lens, 8, 72 + 14 + 260 + 6)


def test_three_runs_unshared_fit_one_shared():
    """the phrase-list case: 32 candidates of 6 tokens behind a prompt of 260 on max_batch 32"""
    prompt_lens, cand_lens = [260], [[6] * 32]
    tok_cap = 11 * 265                                                 # eleven unshared sequences of 260 + 5 tokens: 32 of them take three runs
    plain = scoring.plan_runs(prompt_lens, cand_lens, 32, tok_cap, 1024)
    shared = scoring.plan_runs(prompt_lens, cand_lens, 32, tok_cap, 1024, share_prompt=True)
    assert len(plain) == 3 and len(shared) == 1 and shared[0].fanout == 32
    assert shared_tokens(shared[0], prompt_lens, cand_lens) == 260 + 32 * 5 == 420
    check_cover(shared, prompt_lens, cand_lens, 32, tok_cap)


def test_fanout_caps():
    # by max_batch
    runs = scoring.plan_runs([100], [[10] * 9], max_batch=4, tok_cap=100000, max_ctx=1024, share_prompt=True)
    assert [r.fanout for r in runs] == [4, 4, 4] and runs[2].groups == [(0, [8, None, None, None])]
    check_cover(runs, [100], [[10] * 9], 4, 100000)
    # by P + N (longest L - 1) <= tok_cap: 100 + N * 19 <= 160 -> N = 3, where the unshared form holds one sequence per run
    prompt_lens, cand_lens = [100, 60], [[20, 4, 4, 4], [4]]
    runs = scoring.plan_runs(prompt_lens, cand_lens, max_batch=16, tok_cap=160, max_ctx=1024, share_prompt=True)
    assert all(r.fanout == 3 for r in runs)
    check_cover(runs, prompt_lens, cand_lens, 16, 160)
    assert all(r.fanout == 1 for r in scoring.plan_runs(prompt_lens, cand_lens, 16, 160, 1024))
    # the longest prompt and the longest candidate belong to different audios and do not fit together: one sequence per group, each of which fits
    runs = scoring.plan_runs([150, 20], [[5], [100, 100]], max_batch=8, tok_cap=160, max_ctx=1024, share_prompt=True)
    assert all(r.fanout == 1 for r in runs)
    check_cover(runs, [150, 20], [[5], [100, 100]], 8, 160)


def test_value_errors_are_the_unshared_ones():
    for share in (False, True):
        with pytest.raises(ValueError, match="max_ctx"):
            scoring.plan_runs([60], [[5]], 4, 1000, 64, share_prompt=share)
        with pytest.raises(ValueError, match="does not fit"):
            scoring.plan_runs([60], [[50]], 4, 100, 1024, share_prompt=share)
        with pytest.raises(ValueError, match="no target ids"):
            scoring.plan_runs([60], [[0]], 4, 100, 1024, share_prompt=share)
        with pytest.raises(ValueError, match="candidate lists"):
            scoring.plan_runs([60, 60], [[5]], 4, 100, 1024, share_prompt=share)
        assert scoring.plan_runs([10], [[]], 4, 100, 64, share_prompt=share) == []


def test_default_call_is_what_it_was():
    """share_prompt defaults to off, and off is the plan of the parent commit, restated here: N from tok_cap // longest sequence, a dummy charged its prompt"""
    cases = [([72, 260], [[5, 9, 3], [7]], 8, 5000), ([100, 100, 100], [[10] * 5, [20] * 2, [4]], 4, 100000), ([100, 100, 100], [[10] * 5, [20] * 2, [4]], 64, 250),
             ([260], [[6] * 32], 32, 2827)]
    for prompt_lens, cand_lens, max_batch, tok_cap in cases:
        longest = max(max([p + L - 1 for L in cl] + [p]) for p, cl in zip(prompt_lens, cand_lens))
        N = max(1, min(max_batch, max(len(c) for c in cand_lens), tok_cap // longest))
        want, cur, used = [], [], 0
        for a, cl in enumerate(cand_lens):
            for i in range(0, len(cl), N):
                part = list(range(len(cl)))[i:i + N]
                tokens = sum(prompt_lens[a] + cl[c] - 1 for c in part) + (N - len(part)) * prompt_lens[a]
                if cur and ((len(cur) + 1) * N > max_batch or used + tokens > tok_cap):
                    want.append(scoring.Run(N, cur)); cur, used = [], 0
                cur.append((a, part + [None] * (N - len(part)))); used += tokens
        want.append(scoring.Run(N, cur))
        assert scoring.plan_runs(prompt_lens, cand_lens, max_batch, tok_cap, 1024) == want
        assert scoring.plan_runs(prompt_lens, cand_lens, max_batch, tok_cap, 1024, False) == want


def test_asrmodel_defaults_and_refusals():
    from sonicscribe_amd.asr import ASRModel, check_share_prompt
    m = ASRModel.__new__(ASRModel)                                     # a model that was never built reads the flags' "off" values
    assert m.score_share_prompt is False and m.share_prompt_refusal() is None
    assert check_share_prompt(True, True, "native", False) is True and check_share_prompt(False, False, "int8", True) is False
    m.timestamps = True
    assert "timestamps" in m.share_prompt_refusal()
    with pytest.raises(ValueError, match="share_prompt.*timestamps"):
        check_share_prompt(True, True, "native", True)
    m.timestamps, m.mode = False, "int8"
    assert "int8" in m.share_prompt_refusal()
    with pytest.raises(ValueError, match="share_prompt.*int8"):
        check_share_prompt(True, True, "int8", False)
    with pytest.raises(ValueError, match="scoring=True"):
        check_share_prompt(True, False, "native", False)
    for kw in (dict(token_logprobs=True, score_share_prompt=True), dict(mode="int8", token_logprobs=True, scoring=True, score_share_prompt=True),
               dict(token_logprobs=True, scoring=True, timestamps=True, score_share_prompt=True)):
        with pytest.raises(ValueError, match="share_prompt"):           # ahead of any engine: no device is touched
            ASRModel("<none>", **kw)
