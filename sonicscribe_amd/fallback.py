"""Decoding with temperature fallback: openai-whisper's decode_with_fallback, which faster-whisper follows.

A segment is decoded at the first temperature of the ladder (0: greedy).  If the transcript compresses too well (a repeat loop) or its average
log-probability is too low, it is decoded again at the next temperature, with the same seed, the same prompt and the same tables.  The first attempt that
passes is returned; when every attempt fails the LAST one is returned (Whisper's rule).  A retry is a new request for the same audio: it encodes and
prefills again (KV reuse across attempts is out of scope).

best_of: on a model built with best_of = N > 1, an attempt at a temperature above 0 draws N samples and keeps the most likely one (pick_best),
as Whisper and faster-whisper do; the ladder then judges that winner as it judges any attempt.  The N samples are the rows of ONE forked run - one encoder pass,
one prefill - on a handle of their own, driven by a worker thread per replica (a Retrier); an attempt at temperature 0 is one greedy decode, whatever N.

Retries are never submitted from a completion callback: the dispatchers complete futures on their own threads - the native one while it holds the lock
that `put` takes, the continuous one on the thread that steps every running row - so a small worker thread (Retrier) judges an attempt and submits the next.
The thread that called `submit` never blocks.
"""
from __future__ import annotations

import queue
import threading
import zlib
from concurrent.futures import Future
from typing import Any, Callable, Optional, Sequence

from . import sampling

WHISPER_TEMPERATURES = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)


def compression_ratio(text: str) -> float:
    """len(utf-8) / len(zlib of it): openai-whisper's measure of repetition.  An empty text has ratio 0 (it never fails the threshold)."""
    raw = text.encode("utf-8")
    return len(raw) / len(zlib.compress(raw)) if raw else 0.0


def pick_best(avg_logprobs: Sequence[float]) -> int:
    """Whisper's MaximumLikelihoodRanker without length penalty: the index of the sample with the highest average log-probability (the mean over its emitted
    tokens, EOS included, as Transcription.avg_logprob computes it).  Ties go to the lowest index; a nan average (nothing emitted) ranks below every number."""
    vals = [float(v) for v in avg_logprobs]
    if not vals:
        raise ValueError("pick_best: no sample")
    best = 0
    for j in range(1, len(vals)):
        if vals[j] == vals[j] and (vals[best] != vals[best] or vals[j] > vals[best]):
            best = j
    return best


class FallbackPolicy:
    """Whisper's defaults.  Either threshold may be None (ignored).  An attempt fails when its compression ratio is ABOVE compression_ratio_threshold or its
    average log-probability is BELOW logprob_threshold (a nan average - nothing emitted - fails neither)."""
    __slots__ = ("temperatures", "compression_ratio_threshold", "logprob_threshold")

    def __init__(self, temperatures: Sequence[float] = WHISPER_TEMPERATURES, compression_ratio_threshold: Optional[float] = 2.4,
                 logprob_threshold: Optional[float] = -1.0):
        self.temperatures, _ = sampling.temperatures(tuple(temperatures))
        self.compression_ratio_threshold = None if compression_ratio_threshold is None else float(compression_ratio_threshold)
        self.logprob_threshold = None if logprob_threshold is None else float(logprob_threshold)

    def failed(self, ratio: float, avg_logprob: float) -> bool:
        if self.compression_ratio_threshold is not None and ratio > self.compression_ratio_threshold:
            return True
        return self.logprob_threshold is not None and avg_logprob < self.logprob_threshold

    def __repr__(self):
        return f"FallbackPolicy(temperatures={self.temperatures}, compression_ratio_threshold={self.compression_ratio_threshold}, logprob_threshold={self.logprob_threshold})"


class Retrier:
    """One daemon thread that runs posted callables in order (started on first use)."""

    def __init__(self, name: str = "sonic-fallback"):
        self._q: "queue.Queue[Optional[Callable[[], None]]]" = queue.Queue()
        self._name, self._thread, self._lock = name, None, threading.Lock()

    def post(self, fn: Callable[[], None]):
        with self._lock:
            if self._thread is None:
                self._thread = threading.Thread(target=self._loop, name=self._name, daemon=True)
                self._thread.start()
        self._q.put(fn)

    def _loop(self):
        while True:
            fn = self._q.get()
            if fn is None:
                return
            try:
                fn()
            except BaseException:
                pass                      # (every posted step reports into its own future)

    def close(self):
        with self._lock:
            t, self._thread = self._thread, None
        if t is not None:
            self._q.put(None)
            t.join(timeout=10)


class _Inline:
    """Retrier for callers that have no thread to spare and complete their futures outside any lock (tests, synchronous stubs)."""

    @staticmethod
    def post(fn):
        fn()


def decode_with_fallback(submit: Callable[..., "Future[Any]"], policy: FallbackPolicy, seed: int = 0, retrier=None, **kw) -> "Future[Any]":
    """`submit(temperature=t, seed=seed, **kw)` queues one attempt and returns a future of a result with `.text` and `.avg_logprob` (a Transcription).  The
    returned future resolves after the last attempt, to that attempt's result with `.temperature`, `.compression_ratio` and `.attempts` filled in.  seed and
    kw (prompt, tables, budgets ...) go unchanged to every attempt."""
    out: "Future[Any]" = Future()
    retrier = retrier or _Inline
    state = {"inner": None}
    out.add_done_callback(lambda f: state["inner"].cancel() if f.cancelled() and state["inner"] is not None else None)

    def attempt(k: int):
        if out.done():
            return
        try:
            inner = submit(temperature=policy.temperatures[k], seed=seed, **kw)
        except BaseException as ex:
            if not out.done():
                out.set_exception(ex)
            return
        state["inner"] = inner
        inner.add_done_callback(lambda f, k=k: retrier.post(lambda: judge(k, f)))

    def judge(k: int, f: "Future[Any]"):
        if out.done():
            return
        try:
            res = f.result()
            ratio = compression_ratio(res.text)
            if k + 1 < len(policy.temperatures) and policy.failed(ratio, res.avg_logprob):
                attempt(k + 1)
                return
            res.temperature, res.compression_ratio, res.attempts = float(policy.temperatures[k]), ratio, k + 1
            out.set_result(res)
        except BaseException as ex:
            if not out.done():
                out.set_exception(ex)

    attempt(0)
    return out
