"""What a request resolves to: Transcription, the function that stamps one with its call's values, and the futures from the scheduler's token ids to the caller's text."""
from __future__ import annotations

from concurrent.futures import Future
from typing import List, Sequence

import numpy as np

from .engine import TokenScores


class Transcription:
    """What a `detailed=True` request resolves to (ASRModel(token_logprobs=True)): the transcript, the emitted token ids (EOS included), every
    token's log-probability under the model (float32; HF compute_transition_scores(..., normalize_logits=True) of the greedy generate()) and their
    mean - the number a caller turns into the wire messages' "confidence" (connection_manager.py:159,274 can only send constants).  `temperature`: the one this
    transcript was decoded at (0: greedy); `compression_ratio`: fallback.compression_ratio of the text; `attempts`: how many decodes the fallback ladder took (1
    without a ladder).  The log-probabilities are at temperature 1 whatever the sampling temperature (openai-whisper's convention).
    `top_token_ids` [n, K] int32 and `top_logprobs` [n, K] float32 (ASRModel(top_logprobs=K); [n, 0] without): at every step the K best ids by (score
    descending, id ascending) with their log-probabilities - OpenAI's top_logprobs; places beyond the ids with a finite score hold (-1, -inf).  They are what
    the model scored, whatever token was emitted: on a greedy request column 0 is the token itself."""
    __slots__ = ("text", "token_ids", "token_logprobs", "avg_logprob", "temperature", "compression_ratio", "attempts", "top_token_ids", "top_logprobs",
                 "draft_len", "draft_matched",      # a request that brought a draft (ASRModel(draft_verify=True)): the ids of the draft as it was submitted, and how many of them the transcript begins with; 0 without
                 "best_of", "fork_index", "fork_avg_logprobs",      # an attempt that drew best_of samples from one forked run (ASRModel(best_of=N)): how many, which of them this is, and every sample's avg_logprob in fork order; 1, 0 and this transcript's own otherwise
                 "top_k", "top_p", "min_p",      # what a sampled transcript's tail was cut with (ASRModel(sampling=True, top_k=, top_p=, min_p=)); 0, 1.0, 0.0: nothing, and always at temperature 0
                 "grammar_status",      # a request decoded under a grammar: grammar.Grammar.walk over token_ids - "accepted", "incomplete" or "left"; None without
                 "words", "token_start", "token_end")      # word_timestamps=True (ASRModel(timestamps=True)): timestamps.Word list and the tokens' times (EOS dropped); None without

    def __init__(self, text: str, token_ids, token_logprobs, temperature: float = 0.0):
        from .fallback import compression_ratio
        self.text = text
        self.words = self.token_start = self.token_end = self.grammar_status = None
        self.draft_len = self.draft_matched = 0
        self.top_k, self.top_p, self.min_p = 0, 1.0, 0.0
        self.temperature, self.compression_ratio, self.attempts = float(temperature), compression_ratio(text), 1
        self.token_ids = np.asarray(token_ids, np.int32)
        top_lp = top_ids = None
        if isinstance(token_logprobs, TokenScores):      # a top_logprobs model: the engine's unpacked wide records
            token_logprobs, top_lp, top_ids = token_logprobs
        self.token_logprobs = np.asarray(token_logprobs, np.float32)
        n = self.token_logprobs.shape[0] if self.token_logprobs.ndim else 0
        self.top_logprobs = np.zeros((n, 0), np.float32) if top_lp is None else np.asarray(top_lp, np.float32)
        self.top_token_ids = np.zeros((n, 0), np.int32) if top_ids is None else np.asarray(top_ids, np.int32)
        # over all emitted tokens, the EOS that stopped the row included; nothing emitted: nan
        self.avg_logprob = float(np.mean(self.token_logprobs, dtype=np.float64)) if self.token_logprobs.size else float("nan")
        self.best_of, self.fork_index, self.fork_avg_logprobs = 1, 0, np.asarray([self.avg_logprob], np.float64)

    def __repr__(self):
        return f"Transcription(text={self.text!r}, tokens={self.token_ids.size}, avg_logprob={self.avg_logprob:.4f})"


def cut_draft(ids: Sequence[int], eos_ids: Sequence[int], max_new: int) -> List[int]:
    """A draft as the library takes it: cut in front of its first EOS id and at max_new - 1 ids (the last token of a budget is the model's own).  The library refuses
    such drafts instead of cutting them; a caller who hands over a previous transcript - EOS included - should not have to"""
    out: List[int] = []
    for t in ids:
        if int(t) in eos_ids or len(out) >= int(max_new) - 1:
            break
        out.append(int(t))
    return out


def draft_matched(token_ids: Sequence[int], draft: Sequence[int]) -> int:
    """the length of the common prefix of a transcript's ids and its draft"""
    n = 0
    for a, b in zip(token_ids, draft):
        if int(a) != int(b):
            break
        n += 1
    return n


def stamp(tr: Transcription, temperature: float, cut=(), grammar=None, draft=None) -> Transcription:
    """A Transcription under its call's values: the (top_k, top_p, min_p) it was decoded under - the call's at a temperature above 0, none at 0 (greedy rows ignore
    them) -, its grammar's verdict on its ids, and how much of its draft it begins with"""
    if cut and temperature > 0:
        tr.top_k, tr.top_p, tr.min_p = cut
    if grammar is not None:
        tr.grammar_status = grammar.grammar.walk(tr.token_ids)
    if draft:
        tr.draft_len, tr.draft_matched = len(draft), draft_matched(tr.token_ids, draft)
    return tr


def then(inner: "Future", fn) -> "Future":
    """Future of fn(inner's result).  An exception from either is its exception; cancelling it cancels `inner` (a session that went away: the queued request never
    reaches the device); nothing is set on it once it is done."""
    out: "Future" = Future()

    def done(f):
        if out.done():
            return
        try:
            out.set_result(fn(f.result()))
        except BaseException as ex:
            if not out.done():
                out.set_exception(ex)
    inner.add_done_callback(done)
    out.add_done_callback(lambda f: inner.cancel() if f.cancelled() else None)
    return out


def _only_text(fut: "Future") -> "Future[str]":
    """Future of the text behind a future of a Transcription; cancelling it cancels that one"""
    return then(fut, lambda tr: tr.text)


def _text_future(inner: "Future", decode, detailed: bool = False, temperature: float = 0.0, grammar=None, draft=None, cut=()) -> "Future[str]":
    """Future of the transcript behind a dispatcher future of token ids.  Cancelling it (a session that went away) cancels the queued
    request as well, so it never reaches the device.  detailed: the inner future carries (ids, log-probabilities), the result is a Transcription."""
    def transcript(res):
        if not detailed:
            return decode(res).strip()
        ids, lps = res
        return stamp(Transcription(decode(ids).strip(), ids, lps, temperature), temperature, cut, grammar, draft)
    return then(inner, transcript)
