"""Host side of transcript scoring (ASRModel.score / Engine.score_batch): what a candidate is, how candidates are packed into the forced-id
array of the parallel forced run, and how more candidates than one run holds are split over several.

A run scores R sequences in one prefill pass: R / N audio requests with N candidates each (engine option forced_fanout = N), so the candidates of one
audio share its encoder pass.  Candidate lists of unequal size are padded with a one-token dummy, which is cut from the results again.

This file is host logic only (no GPU, no library).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np


class Score:
    """One candidate's score under the model, given the audio: `token_ids` (the candidate as it was scored - up to and including its first EOS id), every
    token's log-probability (float32; HF's compute_transition_scores over `logits` with normalize_logits=True: the raw distribution at temperature 1, no logits
    processor), their sum (float64 accumulation: HF's sequence score before any length penalty) and mean.  `top_token_ids` [n, K] / `top_logprobs` [n, K]
    (a model built with top_logprobs=K; [n, 0] without): the K best ids at every position with their log-probabilities."""
    __slots__ = ("text", "token_ids", "token_logprobs", "sum_logprob", "avg_logprob", "top_token_ids", "top_logprobs")

    def __init__(self, text: str, token_ids, token_logprobs):
        self.text = text
        self.token_ids = np.asarray(token_ids, np.int32)
        top_lp = top_ids = None
        if isinstance(token_logprobs, tuple) and len(token_logprobs) == 3:      # engine.TokenScores: (lp, top_logprobs, top_ids)
            token_logprobs, top_lp, top_ids = token_logprobs
        self.token_logprobs = np.asarray(token_logprobs, np.float32)
        n = self.token_logprobs.shape[0]
        self.top_logprobs = np.zeros((n, 0), np.float32) if top_lp is None else np.asarray(top_lp, np.float32)
        self.top_token_ids = np.zeros((n, 0), np.int32) if top_ids is None else np.asarray(top_ids, np.int32)
        self.sum_logprob = float(np.sum(self.token_logprobs, dtype=np.float64)) if n else 0.0
        self.avg_logprob = self.sum_logprob / n if n else float("nan")

    def __repr__(self):
        return f"Score(text={self.text!r}, tokens={self.token_ids.size}, sum_logprob={self.sum_logprob:.4f}, avg_logprob={self.avg_logprob:.4f})"


def scored_length(ids: Sequence[int], eos_ids: Sequence[int], budget: Optional[int] = None) -> int:
    """How many of `ids` a forced run scores: 1 + the index of the first EOS id among ids[0 .. budget), or budget if there is none (HF's stopping rule, the one
    include/sonic_hip.h states for forcing)."""
    m = len(ids) if budget is None else min(int(budget), len(ids))
    eos = set(int(e) for e in eos_ids)
    for n in range(m):
        if int(ids[n]) in eos:
            return n + 1
    return m


def pack_targets(targets, eos_ids: Sequence[int] = (), pad_id: int = 0) -> Tuple[np.ndarray, List[int]]:
    """targets -> (forced ids [R][ld] int32, each sequence's own length).  A 2-D integer array is taken as it stands (every sequence has length ld: rows are
    padded by the caller with any valid id, and only [0 .. L_r) is read); a list of id sequences is padded with `pad_id` to the longest.  Empty sequences are
    refused: a forced run scores at least one token per sequence."""
    if isinstance(targets, np.ndarray) and targets.ndim == 2:
        a = np.ascontiguousarray(targets, dtype=np.int32)
        if a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("targets: an empty forced-id array")
        return a, [int(a.shape[1])] * int(a.shape[0])
    seqs = [np.asarray(t, np.int64).reshape(-1) for t in targets]
    if not seqs or any(s.size == 0 for s in seqs):
        raise ValueError("targets: every sequence needs at least one id")
    ld = max(int(s.size) for s in seqs)
    a = np.full((len(seqs), ld), int(pad_id), np.int32)
    for r, s in enumerate(seqs):
        a[r, : s.size] = s
    return a, [int(s.size) for s in seqs]


def with_eos(ids: Sequence[int], eos_ids: Sequence[int], append_eos: bool) -> List[int]:
    """a candidate's target ids: append_eos adds the first EOS id as the last target unless the candidate already ends in an EOS id, so that hypotheses of
    different length compare as HF's sequence scores do"""
    out = [int(i) for i in ids]
    if append_eos and eos_ids and (not out or out[-1] not in set(int(e) for e in eos_ids)):
        out.append(int(eos_ids[0]))
    return out


class Run(NamedTuple):
    """One parallel forced run: `fanout` sequences per audio request; groups[i] = (audio index, its candidate indices in this run - None marks a dummy)."""
    fanout: int
    groups: List[Tuple[int, List[Optional[int]]]]


def plan_runs(prompt_lens: Sequence[int], cand_lens: Sequence[Sequence[int]], max_batch: int, tok_cap: int, max_ctx: int, share_prompt: bool = False) -> List[Run]:
    """Split A audios with their candidates over runs.  prompt_lens[a]: audio a's prompt tokens; cand_lens[a][c]: the target ids of its candidate c.  A run holds
    at most max_batch sequences and tok_cap tokens, a sequence of P prompt tokens and L targets counting P + L - 1 (the last target is only scored, never fed); a
    dummy is one target: P tokens.  Every run has ONE fan-out N: the largest candidate count, capped by max_batch and by how many of the longest sequence fit
    tok_cap; an audio with more candidates appears in several groups, its last group padded with dummies.  ValueError for a candidate that cannot be scored at
    all: prompt + targets beyond max_ctx, or one sequence beyond tok_cap.
    share_prompt (engine option forced_share_prompt): a group prefills its prompt once - it counts P + the sum of its candidates' L - 1, a dummy
    counts nothing, and N is capped by how many suffixes of the longest candidate fit tok_cap beside the longest prompt."""
    A = len(prompt_lens)
    if A != len(cand_lens):
        raise ValueError(f"{A} audios but {len(cand_lens)} candidate lists")
    longest = 1
    for a in range(A):
        for c, L in enumerate(cand_lens[a]):
            if L < 1:
                raise ValueError(f"candidate {c} of audio {a} has no target ids")
            if prompt_lens[a] + L > max_ctx:
                raise ValueError(f"candidate {c} of audio {a}: prompt ({prompt_lens[a]}) + targets ({L}) exceed max_ctx ({max_ctx})")
            longest = max(longest, prompt_lens[a] + L - 1)
        longest = max(longest, int(prompt_lens[a]))
    if longest > tok_cap:
        raise ValueError(f"a sequence of {longest} tokens does not fit one run ({tok_cap} tokens)")
    most = max((len(c) for c in cand_lens), default=0)
    if most == 0:
        return []
    if share_prompt:
        p_max = max(int(p) for p in prompt_lens)
        l_max = max(int(L) for c in cand_lens for L in c)
        fit = (tok_cap - p_max) // max(1, l_max - 1)      # P + N (L - 1) <= tok_cap for the longest P and L: no group of N outgrows a run
    else:
        fit = tok_cap // longest
    N = max(1, min(int(max_batch), most, fit))
    groups: List[Tuple[int, List[Optional[int]], int]] = []        # (audio, candidates, tokens)
    for a in range(A):
        idx = list(range(len(cand_lens[a])))
        for i in range(0, len(idx), N):
            part: List[Optional[int]] = list(idx[i:i + N])
            if share_prompt:
                tokens = prompt_lens[a] + sum(cand_lens[a][c] - 1 for c in part)
            else:
                tokens = sum(prompt_lens[a] + cand_lens[a][c] - 1 for c in part) + (N - len(part)) * prompt_lens[a]
            groups.append((a, part + [None] * (N - len(part)), int(tokens)))
    runs: List[Run] = []
    cur: List[Tuple[int, List[Optional[int]]]] = []
    used = 0
    for a, part, tokens in groups:
        if cur and ((len(cur) + 1) * N > max_batch or used + tokens > tok_cap):
            runs.append(Run(N, cur))
            cur, used = [], 0
        cur.append((a, part))
        used += tokens
    if cur:
        runs.append(Run(N, cur))
    return runs


def run_targets(run: Run, targets: Sequence[Sequence[Sequence[int]]], dummy_id: int) -> List[List[int]]:
    """the run's R = groups x fanout target sequences in sequence order (a dummy: the one id `dummy_id`)"""
    out: List[List[int]] = []
    for a, part in run.groups:
        for c in part:
            out.append([int(dummy_id)] if c is None else [int(t) for t in targets[a][c]])
    return out
