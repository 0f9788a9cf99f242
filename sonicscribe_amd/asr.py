"""Drop-in ``ASRModel`` (reference: backend/asr.py) backed by the MI355X HIP engine.

Same constructor, ``transcribe`` signature, return types, error behaviour and auxiliary members
(``.model``, ``get_model_info``) as the reference class, so ``backend/models_manager.py:32`` only has to
import this class instead of ``asr.ASRModel``.  What changed underneath:

  * asr.py:230-278  temp-WAV round trip          -> frontend.normalise_to_int16 (no disk)
  * asr.py:393-399  HF processor feature step    -> log-mel HIP kernel (csrc/logmel.hip)
  * asr.py:407-422  HF model.generate            -> HIP encoder / prefill / hipGraph greedy loop
  * asr.py:425-429  batch_decode                 -> unchanged (tokenizer stays in Python)

Concurrent callers (3 executor threads + the event loop, main.py:429-430, transcription_manager.py:58) are
batched per device by ``dispatch.Dispatcher`` instead of serialising on the model; with ``device="cuda:*"`` one engine
replica runs on every visible MI355X inside this one process (the reference is a single process, main.py:1001).
``submit()`` / ``transcribe_async()`` return without blocking the caller, so the WebSocket event loop can keep all
sessions' decodes in flight (INTEGRATION.md shows the change in transcription_manager.py).
"""
from __future__ import annotations

import asyncio
import math
import time
from concurrent.futures import Future
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np

from . import frontend, reqvalues
from .dispatch import Dispatcher
from .engine import Engine, MODE_INT8, MODE_NATIVE, SonicError, TokenScores, device_count, device_info
from .scoring import Score
from .spec import FULL, ModelDims


# Batches in flight per replica on ONE weight copy (engine slots, include/sonic_hip.h sonic_slot_create).  The reference's file mode keeps up to
# three decodes in flight on its one model object (backend/main.py:429-445); here they overlap on the device instead of serialising.
DEFAULT_SLOTS = 2
# Row-level scheduling (dispatch._ContinuousReplica): the replica's engine decodes forever over its rows, the slot prefills; requests join and
# leave row by row.  False: batch by batch (dispatch._Replica), every slot runs whole batches.
DEFAULT_CONTINUOUS = True


# --------------------------------------------------------------------------------------- prompts
class SyntheticPrompt:
    """Stand-in for the checkpoint's tokenizer + chat template (absent offline): fixed prefix / suffix ids
    around the audio placeholders.  Decoding renders ids as text so the call surface stays str-valued."""

    def __init__(self, dims: ModelDims, prefix: Sequence[int] = (1, 17, 23, 5), suffix: Sequence[int] = (7, 301, 302, 303, 9, 11)):
        self.dims, self.prefix, self.suffix = dims, list(prefix), list(suffix)

    def build(self, instruction: str, n_audio: int) -> List[int]:
        extra = [] if instruction == frontend.BASE_INSTRUCTION else [2 + (sum(instruction.encode()) % 200)]
        return self.prefix + [self.dims.audio_token_id] * n_audio + self.suffix + extra

    def decode(self, ids: Sequence[int]) -> str:
        eos = set(self.dims.eos_ids)
        return " ".join(str(int(i)) for i in ids if int(i) not in eos)


class HFPrompt:
    """Tokenizer + chat template of a real checkpoint (processing_glmasr.py:178-180: the audio placeholder string is
    repeated ``num_audio_tokens`` times before tokenisation).  Prompts are cached per (instruction, n_audio) -- SURVEY §8f4."""

    def __init__(self, processor, dims: ModelDims):
        self.processor, self.dims = processor, dims
        self.audio_token = getattr(processor, "audio_token", "<|pad|>")
        self._cache: Dict[Any, List[int]] = {}

    def build(self, instruction: str, n_audio: int) -> List[int]:
        key = (instruction, n_audio)
        if key not in self._cache:
            messages = [{"role": "user", "content": [{"type": "audio", "url": ""}, {"type": "text", "text": instruction}]}]
            text = self.processor.tokenizer.apply_chat_template(messages, tokenize=False, add_generation_prompt=True,
                                                                chat_template=self.processor.chat_template)
            text = text.replace(self.audio_token, self.audio_token * n_audio, 1)
            self._cache[key] = list(self.processor.tokenizer(text, add_special_tokens=False)["input_ids"])
        return self._cache[key]

    def decode(self, ids: Sequence[int]) -> str:
        return self.processor.batch_decode([list(map(int, ids))], skip_special_tokens=True)[0]


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


def check_top_logprobs(top_logprobs, token_logprobs: bool, bulk: bool) -> int:
    """ASRModel's top_logprobs argument -> K, or ValueError by name: outside 0 .. 8, without token_logprobs, with bulk=True (the library's own refusals,
    made before an engine is built)"""
    if isinstance(top_logprobs, bool) or not isinstance(top_logprobs, (int, np.integer)) or not 0 <= int(top_logprobs) <= 8:
        raise ValueError(f"top_logprobs must be an integer in 0 .. 8 (got {top_logprobs!r})")
    K = int(top_logprobs)
    if K and not token_logprobs:
        raise ValueError("top_logprobs needs token_logprobs=True: the alternatives share the log-probability kernels' sum (ASRModel(..., token_logprobs=True, top_logprobs=K))")
    if K and bool(bulk):
        raise ValueError("top_logprobs is not supported with bulk=True: the bulk pipeline carries one log-probability per token")
    return K


def check_best_of(best_of, max_batch: int, sampling: bool = True, bulk: bool = False) -> int:
    """ASRModel's best_of argument -> N, or ValueError by name: not an integer in 1 .. max_batch; above 1 without sampling=True or with bulk=True"""
    if isinstance(best_of, bool) or not isinstance(best_of, (int, np.integer)) or not 1 <= int(best_of) <= int(max_batch):
        raise ValueError(f"best_of must be an integer in 1 .. {int(max_batch)} (max_batch; got {best_of!r})")
    N = int(best_of)
    if N > 1 and not sampling:
        raise ValueError("best_of > 1 needs sampling=True: the samples are drawn at a temperature (ASRModel(..., token_logprobs=True, sampling=True, best_of=N))")
    if N > 1 and bool(bulk):
        raise ValueError("best_of is not supported with bulk=True: the bulk pipeline carries no per-request values")
    return N


def _only_text(fut: "Future") -> "Future[str]":
    """Future of the text behind a future of a Transcription; cancelling it cancels that one"""
    out: "Future[str]" = Future()

    def done(f):
        if out.done():
            return
        try:
            out.set_result(f.result().text)
        except BaseException as ex:
            if not out.done():
                out.set_exception(ex)
    fut.add_done_callback(done)
    out.add_done_callback(lambda f: fut.cancel() if f.cancelled() else None)
    return out


def _stamp_cut(tr, temperature: float, cut) -> None:
    """the (top_k, top_p, min_p) a Transcription was decoded under: the call's at a temperature above 0, none at 0 (greedy rows ignore them)"""
    if cut and temperature > 0:
        tr.top_k, tr.top_p, tr.min_p = cut


def _text_future(inner: "Future", decode, detailed: bool = False, temperature: float = 0.0, grammar=None, draft=None, cut=()) -> "Future[str]":
    """Future of the transcript behind a dispatcher future of token ids.  Cancelling it (a session that went away) cancels the queued
    request as well, so it never reaches the device.  detailed: the inner future carries (ids, log-probabilities), the result is a Transcription."""
    out: "Future[str]" = Future()

    def done(f):
        if out.done():
            return
        try:
            if detailed:
                ids, lps = f.result()
                tr = Transcription(decode(ids).strip(), ids, lps, temperature)
                _stamp_cut(tr, temperature, cut)
                if grammar is not None:
                    tr.grammar_status = grammar.grammar.walk(tr.token_ids)
                if draft:
                    tr.draft_len, tr.draft_matched = len(draft), draft_matched(tr.token_ids, draft)
                out.set_result(tr)
            else:
                out.set_result(decode(f.result()).strip())
        except BaseException as ex:
            if not out.done():
                out.set_exception(ex)
    inner.add_done_callback(done)
    out.add_done_callback(lambda f: inner.cancel() if f.cancelled() else None)
    return out


class AudioStream:
    """Device-resident counterpart of the reference's per-connection chunk store.

    The reference keeps every 2048-byte WebSocket chunk in a host dict keyed by chunk id (backend/audio_manager.py:21-33, fed from
    backend/main.py:813-842), and for every partial / final decode concatenates a chunk range on the host
    (audio_manager.py:99-123), converts it to float (backend/transcription_manager.py:45-54) and hands the tensor to
    ASRModel.transcribe.  Here a chunk goes straight into a ring in HBM on the session's GPU; a decode names a chunk range and the
    int16 -> float -> peak-normalise -> PCM_16 steps run on the device (csrc/ingest.hip), bit-identical with the host path.
    """

    def __init__(self, model: "ASRModel", session: str, replica: int, buffer_seconds: float, margin_seconds: float = 10.0,
                 sampling_rate: int = 16000):
        self.model, self.session, self.replica = model, session, replica
        # wire chunks at another rate than the model's (8 kHz telephony, 48 kHz capture) are resampled by the ring's append
        # (engine.Ring rate=): chunk c maps to the 16 kHz range [head before, head after) of its append - possibly empty - and
        # everything below stays in 16 kHz samples
        self.sampling_rate = int(sampling_rate)
        # A decode names a sample range and the range is only read when the replica reaches the request, so the ring is LARGER than the
        # buffer the session sees: chunks stay addressable for `buffer_seconds` (the reference's MAX_AUDIO_BUFFER_SECONDS, config.py:25),
        # and a queued request survives `margin_seconds` of further appends before the ring overwrites its oldest samples (the
        # reference concatenates on the host at call time and cannot lose audio that way).
        self.visible = int(buffer_seconds * model.target_sr)
        cap = int((buffer_seconds + margin_seconds) * model.target_sr)
        self.ring = model.models[replica].ring_create(cap) if self.sampling_rate == model.target_sr else model.models[replica].ring_create(cap, rate=self.sampling_rate)
        self._chunks: Dict[int, tuple] = {}       # chunk id -> (first sample index, samples)
        self.next_chunk_id = 0
        self._oldest = 0                          # smallest chunk id still in the buffer

    def add_audio_chunk(self, audio_data: bytes, timestamp: Optional[float] = None) -> int:
        """audio_manager.py:21-33: store one wire chunk (with its arrival time, data_basic.py:11-20), return its chunk id."""
        first = self.ring.append(audio_data)
        cid = self.next_chunk_id
        self.next_chunk_id += 1
        n = len(audio_data) // 2 if self.sampling_rate == self.model.target_sr else self.ring.head - first     # a rate ring: what the append emitted
        self._chunks[cid] = (first, n, time.time() if timestamp is None else float(timestamp))
        floor = first + n - self.visible           # chunks older than the buffer (audio_manager.py:35-59 drops them by age)
        while self._oldest < cid and self._chunks[self._oldest][0] < floor:
            del self._chunks[self._oldest]
            self._oldest += 1
        return cid

    @property
    def oldest_chunk_id(self) -> int:
        return self._oldest

    def chunk_timestamp(self, chunk_id: int, default: float = 0.0) -> float:
        """arrival time of a chunk still in the buffer (AudioChunk.timestamp); `default` once it left"""
        c = self._chunks.get(int(chunk_id))
        return c[2] if c is not None else default

    def chunk_range_samples(self, start_chunk_id: int, end_chunk_id: int):
        """(first sample index, sample count) of chunks start..end inclusive, restricted to what the buffer still holds
        (audio_manager.py:76-79: ids that left the buffer are skipped)."""
        ids = [c for c in range(max(start_chunk_id, self._oldest), end_chunk_id + 1) if c in self._chunks]
        if not ids:
            raise ValueError(f"no audio left in the buffer for chunks {start_chunk_id}..{end_chunk_id}")
        for a, b in zip(ids, ids[1:]):
            if b != a + 1:
                raise ValueError("chunk range is not contiguous in the buffer")
        return self._chunks[ids[0]][0], sum(self._chunks[c][1] for c in ids)

    def chunk_samples(self, chunk_id: int):
        """(first sample index, sample count) of a chunk still in the buffer, else None"""
        c = self._chunks.get(int(chunk_id))
        return None if c is None else (c[0], c[1])

    def submit_samples(self, first: int, n: int, max_new_tokens: int = 128, hotwords: Optional[List[str]] = None, detailed: bool = False,
                       sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None, temperature: Optional[float] = None,
                       seed: Optional[int] = None, word_timestamps: bool = False, grammar=None, draft=None, top_k=None, top_p=None, min_p=None) -> "Future[str]":
        """Transcribe ring samples [first, first + n) (the >30 s split of connection_manager.py:206-214 cuts at byte offsets, not chunks).
        detailed (a model built with token_logprobs=True): the future gives a Transcription instead of the text.  temperature / seed (a model built with
        sampling=True): one attempt at that temperature - a float only, stream decodes take no fallback ladder.  draft (a model built with draft_verify=True): what the
        transcript is expected to begin with - the previous partial's text or ids (ASRModel.submit)."""
        m = self.model
        if word_timestamps:
            raise ValueError("word_timestamps is not supported on submit() / transcribe_async() / stream decodes: align a finished transcript with ASRModel.align(), or use transcribe(..., word_timestamps=True)")
        m._check_detailed(detailed)
        values = m._request_values(hotwords, sequence_bias, bad_words_ids, hotword_boost, temperature, seed, grammar, draft, int(max_new_tokens), ladder_ok=False, cut=(top_k, top_p, min_p))
        windows = [self.ring.slice(first + s, e - s) for s, e in frontend.split_windows(n, m.dims)]
        n_audio, _ = frontend.request_audio_tokens(n, m.dims)
        prompt = m.prompt.build(frontend.build_instruction(hotwords), n_audio)
        return m._dispatch(windows, prompt, int(max_new_tokens), detailed, *values, replica=self.replica)

    def submit_chunks(self, start_chunk_id: int, end_chunk_id: int, max_new_tokens: int = 128, hotwords: Optional[List[str]] = None,
                      detailed: bool = False, sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None,
                      temperature: Optional[float] = None, seed: Optional[int] = None, word_timestamps: bool = False, grammar=None, draft=None, top_k=None, top_p=None, min_p=None) -> "Future[str]":
        """Transcribe chunks start..end inclusive (audio_manager.py:76-79 get_chunks_by_range + :115-123 concatenation)."""
        first, n = self.chunk_range_samples(start_chunk_id, end_chunk_id)
        return self.submit_samples(first, n, max_new_tokens, hotwords, detailed, sequence_bias, bad_words_ids, hotword_boost, temperature, seed, word_timestamps, grammar, draft, top_k=top_k, top_p=top_p, min_p=min_p)

    async def transcribe_chunks(self, start_chunk_id: int, end_chunk_id: int, max_new_tokens: int = 128, hotwords: Optional[List[str]] = None) -> str:
        return await asyncio.wrap_future(self.submit_chunks(start_chunk_id, end_chunk_id, max_new_tokens, hotwords))

    def close(self):
        self.ring.close()
        self._chunks.clear()


# --------------------------------------------------------------------------------------- façade
class ASRModel:
    def __init__(self, checkpoint_dir: str, device: str = "cuda", mode: str = "native",
                 cpu_threads: Optional[int] = None, cpu_interop_threads: Optional[int] = None,
                 *, max_batch: int = 32, max_ctx: int = 1024, slots: int = DEFAULT_SLOTS, continuous: bool = DEFAULT_CONTINUOUS, decoders: int = 1, bulk: bool = False, native_dispatch: Optional[bool] = None, token_logprobs: bool = False, top_logprobs: int = 0,
                 repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None, suppress_tokens: Optional[Sequence[int]] = None,
                 request_bias: bool = False, sequence_bias=None, bad_words_ids=None, hotword_boost: float = 0.0,
                 sampling: bool = False, temperature=0.0, seed: int = 0, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0, compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0, best_of: int = 1,
                 scoring: bool = False, timestamps: bool = False, alignment_heads=None, grammar: bool = False, draft_verify: bool = False,
                 _dims: Optional[ModelDims] = None,
                 _synthetic_seed: Optional[int] = None, _allow_synthetic_prompt: bool = False, _options: Optional[Dict[str, int]] = None,
                 _engine_mode: Optional[int] = None):
        """The reference's ASRModel surface over the HIP engine.  `repetition_penalty`, `no_repeat_ngram_size`, `suppress_tokens`: None = the value of the
        checkpoint's generation_config.json, anything else overrides it (genconfig.py).  `request_bias`: requests may bring their own sequence-bias table
        (HF's sequence_bias / bad_words_ids, and `hotword_boost` > 0: the call's hotwords as entries; reqbias.py); `sequence_bias`, `bad_words_ids`,
        `hotword_boost` here are defaults for every request and switch `request_bias` on.  `top_logprobs` = K in 1 .. 8 (needs token_logprobs=True; not with
        bulk=True): every `detailed=True` result also carries the K best ids of every step with their log-probabilities.  `sampling` (needs token_logprobs=True): requests may be decoded at a
        temperature with a seed, or down a fallback ladder of temperatures (fallback.py); `temperature` (a float: one attempt; a sequence: the
        ladder), `seed` and the two thresholds of the ladder here are the defaults of every call.  `best_of` = N in 2 .. max_batch (needs sampling=True; not with bulk=True): Whisper's
        best_of - every attempt at a temperature above 0 draws N samples and keeps the one with the highest avg_logprob; the N samples are the rows of one forked run
        (one encoder pass, one prefill) on one further handle per replica; N is the default of the `best_of=` of transcribe / submit / transcribe_batch.  `scoring` (needs token_logprobs=True): score() / score_batch() give the log-probability of transcripts the caller
        brings, in one prefill pass per run on a handle of their own per replica; off, no such handle exists.  `timestamps` (needs scoring=True): align() and
        word_timestamps=True give the time at which every token and word was spoken, from the decoder's attention onto the audio on that scoring handle;
        `grammar` (needs token_logprobs=True; not with bulk=True): requests may be
        restricted to the transcripts of a grammar - compile_grammar() of a phrase list or of a grammar.Grammar, passed as `grammar=` of the transcribe calls; the mask and
        the state run inside the greedy kernel.  `draft_verify` (not with mode="int8", not with bulk=True): requests may bring a draft of their transcript
        as `draft=` of the transcribe calls - a previous partial, a first-pass model's output, an edited transcript; the prefill accepts the prefix the model itself would
        have emitted and decoding starts behind it, so a right draft costs one prefill instead of its tokens' steps and a wrong one only its prefill rows.  `alignment_heads`: the [layer, head] pairs to read (None: the `alignment_heads` entry of the checkpoint's generation_config.json, else every head of the last half of the layers).  The arguments with a leading underscore are not part of the
        supported surface: they exist for the test-suite and the benchmark and may change without notice.  `_engine_mode` in particular (an engine.MODE_*
        value in place of the one `mode` selects) is unsupported outside the tests: MODE_F32 has no slots, so it needs slots=1, continuous=False."""
        if mode not in ["native", "int8"]:
            raise ValueError("mode must be either 'native' or 'int8'")            # asr.py:46-47
        self.top_logprobs = check_top_logprobs(top_logprobs, token_logprobs, bulk)
        from . import fallback as fallback_, sampling as sampling_
        self.sampling = bool(sampling)
        self._default_temperature, self._default_seed = temperature, sampling_.check_seed(seed)
        ts_, _ = sampling_.temperatures(temperature)
        fallback_.FallbackPolicy(ts_, compression_ratio_threshold, logprob_threshold)      # (validates the values)
        self.compression_ratio_threshold, self.logprob_threshold = compression_ratio_threshold, logprob_threshold
        if not self.sampling and (any(t != 0.0 for t in ts_) or self._default_seed != 0):
            raise ValueError("temperature / seed need a model built with sampling=True (ASRModel(..., token_logprobs=True, sampling=True))")
        self._default_cut = sampling_.check_truncation(top_k, top_p, min_p)      # every sampled decode's tail cut: each rung of a ladder above 0, every fork of best_of
        if not self.sampling and self._default_cut != (0, 1.0, 0.0):
            raise ValueError("top_k / top_p / min_p need a model built with sampling=True (ASRModel(..., token_logprobs=True, sampling=True))")
        if self.sampling and not token_logprobs:
            raise ValueError("sampling=True needs token_logprobs=True: the sampling kernels are log-probability kernels, and the fallback ladder reads avg_logprob")
        if self.sampling and bool(bulk):
            raise ValueError("sampling is not supported with bulk=True: the bulk pipeline carries no per-request values")
        self.best_of = check_best_of(best_of, max_batch, self.sampling, bulk)
        self._max_batch = int(max_batch)
        # grammar: requests may be restricted to the transcripts of a grammar made by compile_grammar() - a phrase list, or any token automaton (grammar.py;
        # DESIGN.md 6.10; engine option of the same name, behind token_logprobs and before the slots exist)
        self.grammar = bool(grammar)
        if self.grammar and not token_logprobs:
            raise ValueError("grammar=True needs token_logprobs=True: the grammar kernels are log-probability kernels (ASRModel(..., token_logprobs=True, grammar=True))")
        if self.grammar and bool(bulk):
            raise ValueError("grammar is not supported with bulk=True: the bulk pipeline carries no per-request grammar state")
        self._grammars: List[Any] = []
        # draft_verify: requests may bring a draft of their transcript (engine option of the same name, before the slots exist)
        self.draft_verify = bool(draft_verify)
        if self.draft_verify and mode == "int8":
            raise ValueError("draft_verify is not supported with mode='int8': its prefill quantises per request group, so a draft would change the prompt's own values")
        if self.draft_verify and bool(bulk):
            raise ValueError("draft_verify is not supported with bulk=True: the bulk pipeline verifies no drafts")
        self.scoring = bool(scoring)
        if self.scoring and not token_logprobs:
            raise ValueError("scoring=True needs token_logprobs=True: a score is the candidates' token log-probabilities (ASRModel(..., token_logprobs=True, scoring=True))")
        from . import timestamps as timestamps_
        self.timestamps = bool(timestamps)
        self.alignment_heads = timestamps_.check_timestamps(self.timestamps, self.scoring, alignment_heads, *((_dims.dec_layers, _dims.dec_heads) if _dims is not None else ()))
        dev = str(device)
        if dev.startswith("cpu"):
            raise RuntimeError("sonicscribe_amd runs on MI355X only: DEVICE=cpu has no HIP path (no CPU fallback by design)")
        n_dev = device_count()
        # "cuda" / "cuda:1" = one replica (the reference's surface); "cuda:*" = every visible GPU; "cuda:0,2,3" = those
        spec_ = dev.split(":", 1)[1] if ":" in dev else "0"
        self.device_indices = list(range(n_dev)) if spec_ in ("*", "all") else [int(x) for x in spec_.split(",") if x != ""]
        if not self.device_indices or max(self.device_indices) >= n_dev:
            raise RuntimeError(f"HIP device {spec_} not available ({n_dev} visible)")
        self.device_index = self.device_indices[0]
        self.device = f"cuda:{self.device_index}" if len(self.device_indices) == 1 else "cuda:" + ",".join(map(str, self.device_indices))
        self.mode = mode
        self.model_dtype = "bfloat16" if mode == "native" else "float16"                     # asr.py:61
        emode = MODE_NATIVE if mode == "native" else MODE_INT8
        if _engine_mode is not None:                 # tests only, unsupported (docstring): another kind behind the same façade
            emode = int(_engine_mode)
        self.checkpoint_dir = Path(checkpoint_dir)
        self.target_sr = 16000
        self.is_glm_asr = True
        self.processor = None
        self.models: List[Engine] = []
        # The checkpoint's generation_config.json, as generate() would merge it into the reference's call (asr.py:411-422): repetition_penalty,
        # no_repeat_ngram_size and suppress_tokens run inside the greedy kernel; a field that would change a do_sample=False run and that the engine
        # does not implement raises here, by name (genconfig.py).  None = the checkpoint's value; an explicit argument overrides it
        from . import genconfig
        file_guards = genconfig.GenerationGuards() if _synthetic_seed is not None else genconfig.load(str(checkpoint_dir))
        self.generation_guards = file_guards.override(repetition_penalty, no_repeat_ngram_size, suppress_tokens)
        if _synthetic_seed is not None:
            self.dims = _dims or FULL
            for di in self.device_indices:
                eng = Engine(self.dims, di, emode, max_batch, max_ctx)
                eng.load_synthetic(_synthetic_seed)
                self.models.append(eng)
            self.prompt = SyntheticPrompt(self.dims)
        else:
            from . import weights
            self.dims = weights.load_dims(str(self.checkpoint_dir))
            for di in self.device_indices:
                eng = Engine(self.dims, di, emode, max_batch, max_ctx)
                weights.load_checkpoint(eng, str(self.checkpoint_dir))
                self.models.append(eng)
            try:
                from transformers import AutoProcessor
                self.processor = AutoProcessor.from_pretrained(str(self.checkpoint_dir))
                self.target_sr = self.processor.feature_extractor.sampling_rate
                self.prompt = HFPrompt(self.processor, self.dims)
            except Exception as ex:
                # The reference fails loudly when the processor / tokenizer is missing (asr.py:66, 120-146).  Feeding placeholder
                # prompt ids to a real model would return garbage "transcripts" without an error, so the stand-in prompt is
                # strictly opt-in (loader tests on tokenizer-less synthetic checkpoints).
                if not _allow_synthetic_prompt:
                    raise RuntimeError(f"could not load the processor / tokenizer from {self.checkpoint_dir}: {ex}") from ex
                self.prompt = SyntheticPrompt(self.dims)
        # token_logprobs: every greedy step also returns the emitted token's log-probability (engine option of the same name; off by default:
        # nothing changes).  Set on every replica before its slots exist; `detailed=True` requests and transcribe(return_debug_info=True) read it
        self.token_logprobs = bool(token_logprobs)
        for eng in self.models:                      # experiment knobs (sonic_set_option) before the slots copy them
            for k, v in (_options or {}).items():
                eng.set_option(k, int(v))
            if self.token_logprobs:
                eng.set_option("token_logprobs", 1)
            if self.top_logprobs:                    # (behind token_logprobs, before the slots exist: the library's order)
                eng.set_option("top_logprobs", self.top_logprobs)
            if self.generation_guards.active:
                g = self.generation_guards
                eng.set_generation(g.repetition_penalty, g.no_repeat_ngram_size, g.suppress_tokens)
        # request_bias: every request may carry a sequence-bias table of its own (engine option of the same name, set before the slots exist).  The three
        # value arguments are defaults for every request and switch the option on.  Combined per call as lists - these sequence_bias entries, these bad words, the
        # call's own, then the hotword entries - and de-duplicated as HF de-duplicates one list (reqbias.combine)
        from . import reqbias
        self.hotword_boost = float(hotword_boost or 0.0)
        self._default_bias = reqbias.RequestBias(sequence_bias, bad_words_ids, self._eos_ids(), vocab=self.dims.vocab)
        reqbias.hotword_entries([], self.hotword_boost, None)         # (validates the value)
        self.request_bias = bool(request_bias) or bool(self._default_bias) or self.hotword_boost > 0
        if self.request_bias and bool(bulk):
            raise ValueError("request_bias is not supported with bulk=True: the bulk pipeline carries no per-request tables")
        if self.request_bias:
            for eng in self.models:
                eng.set_option("request_bias", 1)
        # sampling: every request may be decoded at its own temperature with its own seed (engine option of the same name, behind token_logprobs and before the slots
        # exist), or down a ladder of temperatures until its transcript passes the two thresholds (fallback.py)
        # (the values were checked before any engine was built)
        from . import fallback
        if self.sampling:
            for eng in self.models:
                eng.set_option("sampling", 1)
                eng.set_option("truncation", 1)      # (top_k / top_p / min_p ride on the sampling values; rows that state none take the kernel's branch around the select)
        if self.grammar:
            for eng in self.models:
                eng.set_option("grammar", 1)
        if self.draft_verify:
            for eng in self.models:
                eng.set_option("draft_verify", 1)
        self._retrier = fallback.Retrier()
        self.model = self.models[0]                  # main.py:84-86 checks and deletes `.model`
        # continuous: `decoders` handles per replica run a greedy loop over max_batch rows each, the other handles prefill (>= 1).  Streaming:
        # decoders=1, slots=2.  Bulk transcription of many segments: max_batch=64, decoders=3, slots=4 (the bench's pipeline shape since round 5; decoders=2, slots=3 before).
        # bulk=True (file mode: deep queues of whole segments): the same handles behind the library's native pipeline (dispatch._BulkReplica ->
        # csrc/pipeline.cpp); implies continuous decode loops.  max_batch=64, decoders=3, slots=4 is the bench's shape.
        self.bulk = bool(bulk)
        self.continuous = bool(continuous) or self.bulk
        self.decoders = max(1, int(decoders)) if self.continuous else 0
        self.slots = max(self.decoders + 1 if self.continuous else 1, int(slots))
        # scoring: one further slot per replica with option forced_parallel on, used for nothing else - score() runs on it from the caller's thread, beside the
        # dispatcher's loops, on the slot's own stream (as a prefill slot does); a lock per replica serialises the calls.  Made before the dispatcher takes the others
        import threading
        self._score_engines: List[Engine] = []
        if self.scoring:
            for eng in self.models:
                s_ = eng.slot()
                if self.draft_verify:
                    s_.set_option("draft_verify", 0)      # (a scoring handle verifies no drafts: the library refuses the two options together)
                s_.set_option("forced_parallel", 1)
                self._score_engines.append(s_)
        if self.timestamps:          # the scoring handles also align: their parallel runs return t_n per token
            heads = self.alignment_heads
            if heads is None and _synthetic_seed is None:
                heads = timestamps_.check_timestamps(True, True, timestamps_.load_alignment_heads(str(checkpoint_dir)))
            self.alignment_heads = timestamps_.check_timestamps(True, True, heads, self.dims.dec_layers, self.dims.dec_heads)
            for s_ in self._score_engines:
                s_.set_option("forced_align", 1)
                for l, h in (self.alignment_heads or []):
                    s_.set_option("align_head", l * 256 + h)
        self._score_locks = [threading.Lock() for _ in self._score_engines]
        self._score_next = 0
        # best_of > 1: one further slot per replica, the fork handle, with the model's options - a sampled attempt's N samples are ONE forked run on it (row forks;
        # DESIGN.md 6.12), driven by a worker thread per replica: submit() never blocks, and the dispatcher's handles and queues are untouched
        self._fork_engines: List[Engine] = [eng.slot() for eng in self.models] if self.best_of > 1 else []
        self._fork_workers = [fallback.Retrier(f"sonic-best-of-{i}") for i in range(len(self._fork_engines))]
        self._fork_next = 0
        self._slot_engines = [[eng.slot() for _ in range(self.slots - 1)] for eng in self.models]     # same weights, further batches in flight
        self._dispatcher = Dispatcher(self.models, slots=self._slot_engines, continuous=self.continuous, decoders=self.decoders or 1,
                                      adaptive_tiles="gemm_small_eff" not in (_options or {}), bulk=self.bulk, native=native_dispatch)
        print(f"🚀 初始化 ASR 模型 | 模式: {mode.upper()} | 设备: {self.device} (MI355X HIP engine, "
              f"{self.model.weight_bytes() / 2**20:.0f} MiB weights x {len(self.models)} replica(s), {self.slots} batch slot(s) each)")

    @classmethod
    def from_synthetic(cls, dims: ModelDims = FULL, seed: int = 20260128, device: str = "cuda", mode: str = "native", **kw) -> "ASRModel":
        return cls("<synthetic>", device=device, mode=mode, _dims=dims, _synthetic_seed=seed, **kw)

    # -- reference helpers kept under their reference names
    def _format_hotwords_prompt(self, hotwords: List[str], max_hotwords: int = 10) -> str:
        return frontend.format_hotwords_prompt(hotwords, max_hotwords)

    def _prepare(self, audio_tensor, sampling_rate: int):
        wav = audio_tensor
        if hasattr(wav, "detach"):
            wav = wav.detach().cpu().numpy()
        wav = np.asarray(wav, dtype=np.float32)
        if wav.ndim == 2:
            wav = wav[0]                                                      # first channel (asr.py:252)
        if sampling_rate != self.target_sr:
            wav = frontend.resample_sinc_hann(wav, sampling_rate, self.target_sr)   # asr.py:255-261
        pcm = frontend.normalise_to_int16(wav)
        wins = frontend.split_windows(len(pcm), self.dims)
        n_audio, _ = frontend.request_audio_tokens(len(pcm), self.dims)
        return pcm, [pcm[s:e] for s, e in wins], n_audio

    def _eos_ids(self) -> List[int]:
        return [int(t) for t in self.dims.eos_ids]       # (NoBadWordsLogitsProcessor drops a bad word equal to [eos])

    def _request_bias(self, hotwords, sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None):
        """One call's table: the constructor's defaults, the call's sequence_bias / bad_words_ids, then - for a boost > 0 (None: the constructor's) - the call's
        hotwords as entries (reqbias.hotword_entries: each hotword as it stands and with one leading space, every prefix of 1 .. 8 tokens).  None when nothing
        applies.  ValueError naming request_bias when the call gives a value and the model was built without the option."""
        from . import reqbias
        explicit = sequence_bias is not None or bad_words_ids is not None or (hotword_boost is not None and float(hotword_boost) != 0.0)
        if explicit and not getattr(self, "request_bias", False):
            raise ValueError("sequence_bias / bad_words_ids / hotword_boost need a model built with request_bias=True (ASRModel(..., request_bias=True))")
        if not getattr(self, "request_bias", False):
            return None
        if getattr(self, "bulk", False):
            raise ValueError("a sequence bias is not supported with bulk=True")
        boost = self.hotword_boost if hotword_boost is None else float(hotword_boost)
        hot = None
        if boost != 0.0 and hotwords:
            if not isinstance(self.prompt, HFPrompt):
                raise ValueError("hotword_boost needs a tokenizer (a checkpoint with its processor): the synthetic prompt has none")
            tok = self.prompt.processor.tokenizer
            hot = reqbias.RequestBias(reqbias.hotword_entries(hotwords, boost, lambda t: tok.encode(t, add_special_tokens=False)), vocab=self.dims.vocab)
        else:
            reqbias.hotword_entries([], boost, None)     # (validates the value)
        call = reqbias.RequestBias(sequence_bias, bad_words_ids, self._eos_ids(), vocab=self.dims.vocab) if explicit else None
        out = reqbias.combine(self._default_bias, call, hot)
        return out if out else None

    def _request_sampling(self, temperature=None, seed=None, ladder_ok: bool = True, cut=None):
        """One call's sampling: None (a model without the option, nothing asked), or (temperatures, is it a ladder, seed) from the call's values over the
        constructor's defaults, with a fourth member (top_k, top_p, min_p) unless all three are off - such a request states pairs, as it always did.  `cut` in: the
        call's three values, None for one it does not state.  ValueError naming sampling when the call gives a value and the model was built without the option."""
        from . import sampling as sampling_
        cut = (None, None, None) if cut is None else tuple(cut)
        if not getattr(self, "sampling", False):
            if temperature is not None or seed is not None:
                raise ValueError("temperature / seed need a model built with sampling=True (ASRModel(..., token_logprobs=True, sampling=True))")
            if any(v is not None for v in cut):
                raise ValueError("top_k / top_p / min_p need a model built with sampling=True (ASRModel(..., token_logprobs=True, sampling=True))")
            return None
        if getattr(self, "bulk", False):
            raise ValueError("a temperature is not supported with bulk=True")
        ts, ladder = sampling_.temperatures(self._default_temperature if temperature is None else temperature)
        if ladder and not ladder_ok:
            raise ValueError("stream decodes take one temperature (a float), not a fallback ladder")
        dflt = getattr(self, "_default_cut", (0, 1.0, 0.0))
        c = sampling_.check_truncation(*[d if v is None else v for v, d in zip(cut, dflt)])
        base = (ts, ladder, sampling_.check_seed(self._default_seed if seed is None else seed))
        return base if c == (0, 1.0, 0.0) else base + (c,)      # (all three off: the triple it always was)

    def compile_grammar(self, phrases_or_grammar, repeat: bool = False):
        """A grammar for `grammar=` of the transcribe calls: a grammar.Grammar, or a list of phrases (grammar.Grammar.from_phrases: each phrase, cleaned as hotwords
        are, as it stands and with one leading space, ending in EOS; repeat=True: any number of phrases in a row; needs the checkpoint's tokenizer).  Returns a
        grammar.CompiledGrammar that lives on every replica and serves any number of requests; it is closed with the model, or earlier by its close() (refused while
        a request still refers to it).  Needs a model built with grammar=True."""
        from . import grammar as grammar_
        if not hasattr(self, "model"):
            raise RuntimeError("ASR model has been released")
        if not getattr(self, "grammar", False):
            raise ValueError("compile_grammar needs a model built with grammar=True (ASRModel(..., token_logprobs=True, grammar=True))")
        g = phrases_or_grammar
        if not isinstance(g, grammar_.Grammar):
            if not isinstance(self.prompt, HFPrompt):
                raise ValueError("a phrase list needs a tokenizer (a checkpoint with its processor): the synthetic prompt has none - pass a grammar.Grammar (Grammar.from_token_sequences)")
            tok = self.prompt.processor.tokenizer
            g = grammar_.Grammar.from_phrases(list(g), lambda t: tok.encode(t, add_special_tokens=False), self._eos_ids(), repeat=repeat,
                                              vocab=self.dims.vocab, audio_token_id=self.dims.audio_token_id)
        c = grammar_.CompiledGrammar(g, self.models)
        self._grammars.append(c)
        return c

    def _request_grammar(self, grammar):
        """One call's grammar: None, or the CompiledGrammar.  ValueError naming grammar when the model was built without the option, and for anything else than a
        compile_grammar() result."""
        if grammar is None:
            return None
        from . import grammar as grammar_
        if not getattr(self, "grammar", False):
            raise ValueError("grammar= needs a model built with grammar=True (ASRModel(..., token_logprobs=True, grammar=True))")
        if getattr(self, "bulk", False):
            raise ValueError("a grammar is not supported with bulk=True")
        if not isinstance(grammar, grammar_.CompiledGrammar):
            raise ValueError("grammar= takes what compile_grammar() returned (a grammar.CompiledGrammar)")
        return grammar

    def _request_draft(self, draft, max_new: int, bias=None, samp=None, gram=None):
        """One call's draft: None, or its token ids - a string goes through the tokenizer (_candidate_ids) - cut in front of the first EOS id and at max_new - 1 ids
        (cut_draft).  ValueError by name when the model was built without draft_verify=True, and beside bias values, a temperature ladder (or any temperature > 0)
        or a grammar: the verify pass applies the model's own processors only, and what it accepts is an argmax."""
        if draft is None:
            return None
        if not getattr(self, "draft_verify", False):
            raise ValueError("draft= needs a model built with draft_verify=True (ASRModel(..., draft_verify=True))")
        if bias:
            raise ValueError("draft= cannot be combined with bias values (sequence_bias / bad_words_ids / hotword_boost): the verify pass applies the model's own processors only")
        if samp is not None and (samp[1] or any(t > 0 for t in samp[0])):
            raise ValueError("draft= cannot be combined with a temperature ladder or a temperature > 0: an accepted draft token is the model's argmax, not a sample")
        if gram is not None:
            raise ValueError("draft= cannot be combined with a grammar: the verify pass applies the model's own processors only")
        ids = cut_draft(self._candidate_ids(draft), self._eos_ids(), max_new)
        return ids or None

    def _request_values(self, hotwords, sequence_bias, bad_words_ids, hotword_boost, temperature, seed, grammar, draft, max_new: int, ladder_ok: bool = True, cut=None):
        """One call's own values, checked in this order: (bias, samp, gram, draft) as _request_bias, _request_sampling, _request_grammar and _request_draft give
        them - what _dispatch takes behind `detailed`, and reqvalues.submit_keywords turns into Dispatcher.submit's keywords."""
        bias = self._request_bias(hotwords, sequence_bias, bad_words_ids, hotword_boost)
        samp = self._request_sampling(temperature, seed, ladder_ok=ladder_ok, cut=cut)
        gram = self._request_grammar(grammar)
        return bias, samp, gram, self._request_draft(draft, max_new, bias, samp, gram)

    def _request_best_of(self, best_of=None) -> int:
        """One call's best_of: the constructor's N when the call states none.  ValueError naming best_of for a value on a model built without best_of > 1, and for
        one outside 1 .. max_batch."""
        N = int(getattr(self, "best_of", 1))
        if best_of is None:
            return N
        if N <= 1:
            raise ValueError("best_of= needs a model built with best_of > 1, which holds the fork handle (ASRModel(..., token_logprobs=True, sampling=True, best_of=N))")
        return check_best_of(best_of, self._max_batch)

    def _fork_replica(self, route) -> int:
        """the replica whose fork handle takes a forked run: where the request is pinned, else its session's home, else the next in turn"""
        if route.get("replica") is not None:
            return int(route["replica"])
        if route.get("session") is not None:
            return self._dispatcher.home(route["session"])
        self._fork_next = (self._fork_next + 1) % len(self._fork_engines)
        return self._fork_next

    def _forked_run(self, replica: int, windows_per_audio, prompts, budgets, biases, grams, temperature: float, seed: int, n: int, cut=()) -> List[Transcription]:
        """ONE forked run on the replica's fork handle (the caller is that replica's worker thread): every audio becomes n rows that share its encoder pass and
        prefill; fork j decodes at `temperature` with seed sampling.fork_seed(seed, j) under the audio's own bias table, grammar and budget.  Per audio the
        Transcription fallback.pick_best selects, with best_of, fork_index and fork_avg_logprobs filled in."""
        from . import fallback, sampling as sampling_
        eng = self._fork_engines[replica]
        forks = [n] * len(prompts)
        rows = Engine.fork_rows(forks)
        samp, bias_rows, gram_rows = [None] * (n * len(prompts)), [None] * (n * len(prompts)), [None] * (n * len(prompts))
        for a, rr in enumerate(rows):
            for j, r in enumerate(rr):
                samp[r] = (temperature, sampling_.fork_seed(seed, j)) + tuple(cut)      # (every fork under the same cut)
                bias_rows[r] = biases[a] if biases[a] else None
                gram_rows[r] = None if grams[a] is None else grams[a].on(eng)
        kw = {}
        if any(b is not None for b in bias_rows):
            kw["request_bias"] = bias_rows
        if any(g is not None for g in gram_rows):
            kw["request_grammar"] = gram_rows
        segs, req_win = [], [0]
        for w in windows_per_audio:
            segs.extend(w)
            req_win.append(len(segs))
        ids, _, lps = eng.transcribe_batch(segs, prompts, budgets, req_win=req_win, want_logprobs=True, request_sampling=samp, forks=forks, **kw)
        out = []
        for a, rr in enumerate(rows):
            trs = [Transcription(self.prompt.decode(ids[r]).strip(), ids[r], lps[r], temperature) for r in rr]
            avgs = [t.avg_logprob for t in trs]
            j = fallback.pick_best(avgs)
            win = trs[j]
            win.best_of, win.fork_index, win.fork_avg_logprobs = n, j, np.asarray(avgs, np.float64)
            _stamp_cut(win, temperature, cut)
            if grams[a] is not None:
                win.grammar_status = grams[a].grammar.walk(win.token_ids)
            out.append(win)
        return out

    def _forked_post(self, replica: int, *run_args) -> "Future":
        """_forked_run(replica, ...) on that replica's worker thread -> a future of its list of winners"""
        out: "Future" = Future()

        def run():
            if not out.set_running_or_notify_cancel():
                return
            try:
                out.set_result(self._forked_run(replica, *run_args))
            except BaseException as ex:
                out.set_exception(ex)
        self._fork_workers[replica].post(run)
        return out

    def _forked_attempt(self, windows, prompt, max_new: int, bias, gram, temperature: float, seed: int, n: int, route, cut=()) -> "Future":
        """one request's sampled attempt as a forked run of n rows -> a future of the winning Transcription"""
        runs = self._forked_post(self._fork_replica(route), [windows], [prompt], [max_new], [bias], [gram], float(temperature), seed, n, cut)
        out: "Future" = Future()

        def done(f):
            if out.done():
                return
            try:
                out.set_result(f.result()[0])
            except BaseException as ex:
                if not out.done():
                    out.set_exception(ex)
        runs.add_done_callback(done)
        out.add_done_callback(lambda f: runs.cancel() if f.cancelled() else None)
        return out

    def _dispatch(self, windows, prompt, max_new: int, detailed: bool, bias, samp, gram=None, draft=None, best_of: int = 1, **route) -> "Future":
        """One request on the scheduler -> a future of its text (detailed: its Transcription).  samp (from _request_sampling): None, one attempt at a temperature,
        or the fallback ladder - each attempt a new request for the same windows, prompt, table and seed; the future resolves after the last one.  Retries
        are submitted by the model's worker thread, never by a completion callback and never by the caller (fallback.py).  best_of = n > 1 (from
        _request_best_of): an attempt at a temperature above 0 is ONE forked run of n samples on the replica's fork handle, whose winner stands for the attempt
        (_forked_run); an attempt at temperature 0 is the one greedy decode it always was."""
        from . import fallback
        kw = dict(route, **reqvalues.submit_keywords(bias, samp, gram, draft))
        cut = () if samp is None or len(samp) < 4 else samp[3]      # (top_k, top_p, min_p): every rung of a ladder above 0 and every fork repeat them
        if samp is not None and not samp[1] and best_of > 1 and samp[0][0] > 0:
            fut = self._forked_attempt(windows, prompt, max_new, bias, gram, samp[0][0], samp[2], best_of, route, cut)
            return fut if detailed else _only_text(fut)
        if samp is None or not samp[1]:
            return _text_future(self._dispatcher.submit(windows, prompt, max_new, want_logprobs=detailed, **kw), self.prompt.decode, detailed,
                                0.0 if samp is None else samp[0][0], grammar=gram, draft=draft, cut=cut)
        ts, seed = samp[0], samp[2]

        def one(temperature, seed):
            if best_of > 1 and temperature > 0:
                return self._forked_attempt(windows, prompt, max_new, bias, gram, temperature, seed, best_of, route, cut)
            return _text_future(self._dispatcher.submit(windows, prompt, max_new, want_logprobs=True, sampling=(temperature, seed) + (cut if temperature > 0 else ()), **kw), self.prompt.decode, True, temperature, grammar=gram, cut=cut)
        policy = fallback.FallbackPolicy(ts, self.compression_ratio_threshold, self.logprob_threshold)
        fut = fallback.decode_with_fallback(one, policy, seed, retrier=self._retrier)
        return fut if detailed else _only_text(fut)

    def _check_detailed(self, detailed: bool):
        if detailed and not getattr(self, "token_logprobs", False):
            raise ValueError("detailed=True needs a model built with token_logprobs=True (ASRModel(..., token_logprobs=True))")

    def submit(self, audio_tensor, sampling_rate: int = 16000, max_new_tokens: int = 128, hotwords: Optional[List[str]] = None,
               session: Optional[str] = None, detailed: bool = False, sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None,
               temperature=None, seed: Optional[int] = None, word_timestamps: bool = False, grammar=None, draft=None, best_of: Optional[int] = None, top_k=None, top_p=None, min_p=None) -> "Future[str]":
        """Non-blocking form of transcribe(): queues the request on a replica and returns a Future of the transcript.  `session`
        (e.g. the WebSocket client id) keeps a session's decodes on one GPU.  detailed (a model built with token_logprobs=True): the future
        gives a Transcription - text, token_ids, token_logprobs, avg_logprob - instead of the text.  sequence_bias / bad_words_ids / hotword_boost (a model
        built with request_bias=True): this request's own table, on top of the constructor's defaults (_request_bias).  temperature / seed (a model built with
        sampling=True): a float decodes once at that temperature, a sequence is the fallback ladder - the future resolves after its last attempt, and this
        thread never waits for one (_dispatch).  grammar (a model built with grammar=True): what compile_grammar() returned - the transcript is one of its paths;
        a detailed result carries `grammar_status`.  draft (a model built with draft_verify=True): what the transcript is expected to begin with, a string or token
        ids - cut here in front of its first EOS id and at max_new_tokens - 1; the result is the model's own greedy transcript whatever the draft says, a detailed one
        carries `draft_len` and `draft_matched`.  Not with bias values, a temperature > 0 or a grammar (ValueError).  best_of (a model built with
        best_of > 1; default: the constructor's): the samples of every attempt at a temperature above 0, drawn in one forked run; a detailed result carries
        `best_of`, `fork_index` and `fork_avg_logprobs`."""
        if not hasattr(self, "model"):
            raise RuntimeError("ASR model has been released")
        if word_timestamps:
            raise ValueError("word_timestamps is not supported on submit() / transcribe_async() / stream decodes: align a finished transcript with ASRModel.align(), or use transcribe(..., word_timestamps=True)")
        self._check_detailed(detailed)
        n_best = self._request_best_of(best_of)
        values = self._request_values(hotwords, sequence_bias, bad_words_ids, hotword_boost, temperature, seed, grammar, draft, int(max_new_tokens), cut=(top_k, top_p, min_p))
        pcm, windows, n_audio = self._prepare(audio_tensor, sampling_rate)
        prompt = self.prompt.build(frontend.build_instruction(hotwords), n_audio)
        return self._dispatch(windows, prompt, int(max_new_tokens), detailed, *values, best_of=n_best, session=session)

    def open_stream(self, session: str, buffer_seconds: float = 30.0, margin_seconds: float = 10.0, sampling_rate: int = 16000) -> AudioStream:
        """A streaming session whose audio stays on the device (config.py:25 MAX_AUDIO_BUFFER_SECONDS = 30): chunks are appended to a
        ring on the session's GPU, partial / final decodes name chunk ranges (AudioStream).  The ring holds `margin_seconds` more than
        the buffer, so a max-length final that waits in the queue is not overwritten by the chunks that keep arriving."""
        if not hasattr(self, "model"):
            raise RuntimeError("ASR model has been released")
        if sampling_rate == self.target_sr:
            return AudioStream(self, session, self._dispatcher.home(session), buffer_seconds, margin_seconds)
        return AudioStream(self, session, self._dispatcher.home(session), buffer_seconds, margin_seconds, sampling_rate=sampling_rate)

    async def transcribe_async(self, audio_tensor, sampling_rate: int = 16000, max_new_tokens: int = 128,
                               hotwords: Optional[List[str]] = None, session: Optional[str] = None, detailed: bool = False,
                               sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None, temperature=None, seed: Optional[int] = None,
                               word_timestamps: bool = False, grammar=None, draft=None, best_of: Optional[int] = None, top_k=None, top_p=None, min_p=None) -> str:
        """Awaitable transcribe() for the asyncio callers (connection_manager.py:127-245): the event loop is not blocked while the
        device works, so all sessions' partial and final decodes can be in flight (and batched) together."""
        return await asyncio.wrap_future(self.submit(audio_tensor, sampling_rate, max_new_tokens, hotwords, session, detailed, sequence_bias, bad_words_ids, hotword_boost, temperature, seed, word_timestamps, grammar, draft, best_of, top_k=top_k, top_p=top_p, min_p=min_p))

    def transcribe(self, audio_tensor, sampling_rate: int = 16000, max_new_tokens: int = 128,
                   hotwords: Optional[List[str]] = None, return_debug_info: bool = False,
                   sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None, temperature=None, seed: Optional[int] = None,
                   word_timestamps: bool = False, grammar=None, draft=None, best_of: Optional[int] = None, top_k=None, top_p=None, min_p=None) -> Union[str, Dict[str, Any]]:
        """best_of (a model built with best_of > 1): see submit(); the debug dictionary gains `best_of` and `fork_index`.
        draft (a model built with draft_verify=True): see submit(); the debug dictionary gains `draft_len` and `draft_matched`.
        grammar (a model built with grammar=True): what compile_grammar() returned; the debug dictionary gains `grammar_status` (grammar.Grammar.walk over
        the returned ids: "accepted", "incomplete" at a budget that ended inside the grammar, "left").
        word_timestamps (a model built with timestamps=True): the request is decoded as always, then its tokens are aligned on the scoring
        handle - the audio is encoded a second time there.  With return_debug_info the dictionary gains `words` (word, start, end, probability), `token_start`
        and `token_end` (seconds, EOS dropped); without, the call returns the Transcription, which carries the same members."""
        if not hasattr(self, "model"):
            raise RuntimeError("ASR model has been released")
        if word_timestamps:
            self._check_timestamps()
        t0 = time.time()
        try:
            want = bool((return_debug_info or word_timestamps) and getattr(self, "token_logprobs", False))
            res = self.submit(audio_tensor, sampling_rate, max_new_tokens, hotwords, detailed=want, sequence_bias=sequence_bias, bad_words_ids=bad_words_ids,
                              hotword_boost=hotword_boost, temperature=temperature, seed=seed, grammar=grammar, draft=draft, best_of=best_of, top_k=top_k, top_p=top_p, min_p=min_p).result()
            det, transcript = (res, res.text) if want else (None, res)
            if word_timestamps:
                self._attach_alignment([audio_tensor], [det], sampling_rate, hotwords)
            elapsed = time.time() - t0
            if return_debug_info:
                n = audio_tensor.shape[-1] if hasattr(audio_tensor, "shape") else len(audio_tensor)
                alloc, reserved = self.model.memory_info()           # asr.py:453-457: allocator state, not the weight size
                info = {"transcript": transcript, "processing_time": elapsed, "audio_length_sec": n / sampling_rate,
                        "mode": self.mode, "device": str(self.device),
                        "gpu_memory_allocated_mb": alloc / 1024 ** 2, "gpu_memory_reserved_mb": reserved / 1024 ** 2}
                if det is not None:                                  # a token_logprobs model: what fills the wire messages' "confidence"
                    info.update({"token_ids": det.token_ids, "token_logprobs": det.token_logprobs, "avg_logprob": det.avg_logprob,
                                 "confidence": math.exp(det.avg_logprob)})
                    if getattr(self, "top_logprobs", 0):             # a top_logprobs model: the K best ids of every step and their log-probabilities
                        info.update({"top_token_ids": det.top_token_ids, "top_logprobs": det.top_logprobs})
                    if getattr(self, "sampling", False):             # a sampling model: what the transcript was decoded at, and the ladder's other measure
                        info.update({"temperature": det.temperature, "compression_ratio": det.compression_ratio, "top_k": det.top_k, "top_p": det.top_p, "min_p": det.min_p})
                    if getattr(self, "best_of", 1) > 1:              # a best_of model: how many samples the returned attempt drew, and which of them this is
                        info.update({"best_of": det.best_of, "fork_index": det.fork_index})
                    if grammar is not None:
                        info["grammar_status"] = det.grammar_status
                    if draft is not None:
                        info.update({"draft_len": det.draft_len, "draft_matched": det.draft_matched})
                    if word_timestamps:
                        info.update({"words": [w.as_dict() for w in det.words], "token_start": det.token_start, "token_end": det.token_end})
                return info
            return det if word_timestamps else transcript
        except RuntimeError as e:
            if "out of memory" in str(e).lower():
                print("⚠️ 显存不足！建议：使用更短的音频 / 减少 max_new_tokens")
            raise
        except Exception as e:
            print(f"❌ 转录过程中发生错误: {e}")
            raise

    def transcribe_batch(self, audios: Sequence[Any], sampling_rate: int = 16000, max_new_tokens: Union[int, Sequence[int]] = 128,
                         hotwords: Optional[List[str]] = None, sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None,
                         temperature=None, seed: Optional[int] = None, word_timestamps: bool = False, grammar=None, drafts=None, best_of: Optional[int] = None, top_k=None, top_p=None, min_p=None) -> List[str]:
        """Batched extension (the reference is B=1 per call): one device batch, per-segment results identical to transcribe().  temperature / seed: every
        segment is decoded with them (a sequence: every segment goes down its own ladder, as independent requests on the scheduler).  word_timestamps (a model
        built with timestamps=True): every audio is decoded as its own request, then all are aligned together; the result is a list of Transcription.
        grammar (a model built with grammar=True): one compile_grammar() result for every audio, or a sequence with one (or None) per audio.
        drafts (a model built with draft_verify=True): one draft (a string, token ids or None) per audio; see submit().
        best_of (a model built with best_of > 1; default: the constructor's): at one temperature above 0, floor(max_batch / best_of) audios share a forked run on
        the fork handle and every audio's winner is returned - what transcribe() returns for it; a ladder takes every audio down its own, forked rung by rung."""
        n_best = self._request_best_of(best_of)
        if drafts is not None and len(drafts) != len(audios):
            raise ValueError(f"{len(audios)} audios but {len(drafts)} drafts")
        grams = list(grammar) if isinstance(grammar, (list, tuple)) else [grammar] * len(audios)
        if len(grams) != len(audios):
            raise ValueError(f"{len(audios)} audios but {len(grams)} grammars")
        grams = [self._request_grammar(g) for g in grams]
        if word_timestamps:
            self._check_timestamps()
            mn_ = [int(max_new_tokens)] * len(audios) if isinstance(max_new_tokens, int) else [int(x) for x in max_new_tokens]
            futs_ = [self.submit(a, sampling_rate, mn_[i], hotwords, detailed=True, sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost,
                                 temperature=temperature, seed=seed, grammar=grams[i], draft=None if drafts is None else drafts[i], best_of=best_of, top_k=top_k, top_p=top_p, min_p=min_p) for i, a in enumerate(audios)]
            dets = [f.result() for f in futs_]
            self._attach_alignment(list(audios), dets, sampling_rate, hotwords)
            return dets
        bias, samp, _, _ = self._request_values(hotwords, sequence_bias, bad_words_ids, hotword_boost, temperature, seed, None, None, 0, cut=(top_k, top_p, min_p))      # (the grammars and drafts: per audio)
        mn = [int(max_new_tokens)] * len(audios) if isinstance(max_new_tokens, int) else [int(x) for x in max_new_tokens]
        drs = [None] * len(audios) if drafts is None else [self._request_draft(d, mn[i], bias, samp, grams[i]) for i, d in enumerate(drafts)]
        segs, req_win, prompts = [], [0], []
        instruction = frontend.build_instruction(hotwords)
        for a in audios:
            _, wins, n_audio = self._prepare(a, sampling_rate)
            segs.extend(wins)
            req_win.append(len(segs))
            prompts.append(self.prompt.build(instruction, n_audio))
        if samp is not None and samp[1]:
            futs = [self._dispatch(segs[req_win[i]:req_win[i + 1]], prompts[i], mn[i], False, bias, samp, grams[i], draft=drs[i], best_of=n_best) for i in range(len(audios))]
            return [f.result() for f in futs]
        if samp is not None and n_best > 1 and samp[0][0] > 0:
            # one temperature above 0: floor(max_batch / best_of) audios per forked run, the runs spread over the replicas' fork handles in turn
            per = max(1, self._max_batch // n_best)
            runs = []
            for g0 in range(0, len(audios), per):
                g = range(g0, min(g0 + per, len(audios)))
                runs.append(self._forked_post(self._fork_replica({}), [segs[req_win[i]:req_win[i + 1]] for i in g], [prompts[i] for i in g], [mn[i] for i in g],
                                              [bias] * len(g), [grams[i] for i in g], samp[0][0], samp[2], n_best, samp[3] if len(samp) > 3 else ()))
            return [t.text for r in runs for t in r.result()]
        subs = [reqvalues.submit_keywords(bias, samp, grams[i], drs[i]) for i in range(len(audios))]
        if len(self.models) == 1 and not self.continuous:
            # one engine call: a value that some audio brings becomes its keyword's list, None for the audios without it
            kw = {v.keyword: [v.on(s.get(v.attr), self.model) for s in subs] for v in reqvalues.VALUES if any(v.attr in s for s in subs)}
            ids, _ = self.model.transcribe_batch(segs, prompts, mn, req_win=req_win, **kw)
        else:            # independent segments: spread over the replicas (least-loaded placement), results in input order
            futs = [self._dispatcher.submit(segs[req_win[i]:req_win[i + 1]], prompts[i], mn[i], **subs[i]) for i in range(len(audios))]
            ids = [f.result() for f in futs]
        return [self.prompt.decode(i).strip() for i in ids]

    # -- scoring: how probable is THIS transcript, given THIS audio
    def _candidate_ids(self, cand) -> List[int]:
        if isinstance(cand, str):
            if not isinstance(self.prompt, HFPrompt):
                raise ValueError("a text candidate needs a tokenizer (a checkpoint with its processor): the synthetic prompt has none - pass token ids")
            return [int(t) for t in self.prompt.processor.tokenizer.encode(cand, add_special_tokens=False)]
        return [int(t) for t in np.asarray(cand).reshape(-1)]

    def score(self, audio, candidates, sampling_rate: int = 16000, hotwords: Optional[List[str]] = None, append_eos: bool = True) -> List["Score"]:
        """The log-probability of each candidate transcript given the audio: n-best / hotword-list rescoring, keyword verification, comparing an edited
        transcript with the greedy one.  A candidate is a string (tokenised with the checkpoint's tokenizer) or a sequence of token ids.  The prompt is the one
        transcribe() builds (same hotword sentence, same audio-token count); all candidates share one encoder pass.  append_eos: the first EOS id is appended as a
        last target, so that hypotheses of different length compare as HF's sequence scores do.  The scores are those of the raw model distribution at temperature
        1: no logits processor (repetition penalty, bias, ...) is applied, whatever the model carries.  Needs a model built with scoring=True."""
        return self.score_batch([audio], [candidates], sampling_rate, hotwords, append_eos)[0]

    def score_batch(self, audios: Sequence[Any], candidates_per_audio: Sequence[Sequence[Any]], sampling_rate: int = 16000,
                    hotwords: Optional[List[str]] = None, append_eos: bool = True) -> List[List["Score"]]:
        """score() for several audios, each with its own candidates: as few runs as hold them (scoring.plan_runs), the same bits as one call per audio."""
        from . import scoring as scoring_
        if not hasattr(self, "model"):
            raise RuntimeError("ASR model has been released")
        if not getattr(self, "scoring", False) or not self._score_engines:
            raise ValueError("score() needs a model built with scoring=True (ASRModel(..., token_logprobs=True, scoring=True))")
        if len(audios) != len(candidates_per_audio):
            raise ValueError(f"{len(audios)} audios but {len(candidates_per_audio)} candidate lists")
        eos = self._eos_ids()
        instruction = frontend.build_instruction(hotwords)
        wins_of, prompts, targets = [], [], []
        for a, cands in zip(audios, candidates_per_audio):
            _, wins, n_audio = self._prepare(a, sampling_rate)
            wins_of.append(wins)
            prompts.append(self.prompt.build(instruction, n_audio))
            targets.append([scoring_.with_eos(self._candidate_ids(c), eos, append_eos) for c in cands])
        i = self._score_next % len(self._score_engines)
        self._score_next += 1
        eng = self._score_engines[i]
        runs = scoring_.plan_runs([len(p) for p in prompts], [[len(t) for t in ts] for ts in targets], eng.max_batch, eng.tok_cap, eng.max_ctx)
        dummy = next(t for t in range(self.dims.vocab) if t != self.dims.audio_token_id and t not in eos)
        out: List[List[Optional[scoring_.Score]]] = [[None] * len(ts) for ts in targets]
        with self._score_locks[i]:
            for run in runs:
                segs, req_win, run_prompts = [], [0], []
                for a, part in run.groups:
                    segs.extend(wins_of[a])
                    req_win.append(len(segs))
                    run_prompts.extend([prompts[a]] * len(part))
                ids, _, lps = eng.score_batch(segs, run_prompts, scoring_.run_targets(run, targets, dummy), req_win=req_win, fanout=run.fanout)
                r = 0
                for a, part in run.groups:
                    for c in part:
                        if c is not None:        # (a dummy's result is cut again)
                            out[a][c] = scoring_.Score(self.prompt.decode(ids[r]).strip(), ids[r], lps[r])
                        r += 1
        return out      # type: ignore[return-value]

    # -- word timestamps: WHEN was this transcript spoken
    def _check_timestamps(self):
        if not getattr(self, "timestamps", False) or not getattr(self, "_score_engines", None):
            raise ValueError("word timestamps need a model built with timestamps=True (ASRModel(..., token_logprobs=True, scoring=True, timestamps=True))")

    def _pieces_of(self, ids: Sequence[int]):
        """the tokens' text pieces for word grouping (timestamps.split_pieces): the tokenizer's, or - the synthetic prompt has none - one word per token"""
        from . import timestamps as timestamps_
        if isinstance(self.prompt, HFPrompt):
            tok = self.prompt.processor.tokenizer
            return timestamps_.split_pieces(ids, lambda t: tok.decode(t, skip_special_tokens=False))
        return [(" " + str(int(t)), [i]) for i, t in enumerate(ids)]

    def _align_items(self, items, replica: Optional[int] = None):
        """items: (windows, prompt ids, target ids with their EOS, samples of the audio) each -> one timestamps.Alignment each, in as few parallel forced runs on
        a scoring handle as hold them (scoring.plan_runs, one candidate per audio).  replica: the handle of that replica (ring slices live on one GPU)."""
        from . import scoring as scoring_, timestamps as timestamps_
        self._check_timestamps()
        if replica is None:
            replica = self._score_next % len(self._score_engines)
            self._score_next += 1
        eng = self._score_engines[replica]
        runs = scoring_.plan_runs([len(it[1]) for it in items], [[len(it[2])] for it in items], eng.max_batch, eng.tok_cap, eng.max_ctx)
        out: List[Any] = [None] * len(items)
        with self._score_locks[replica]:
            for run in runs:
                segs, req_win, prompts, targets, who = [], [0], [], [], []
                for a, part in run.groups:
                    for c in part:
                        if c is None:
                            continue
                        segs.extend(items[a][0]); req_win.append(len(segs)); prompts.append(items[a][1]); targets.append(items[a][2]); who.append(a)
                ids, _, sc = eng.score_batch(segs, prompts, targets, req_win=req_win, fanout=1, align=True)
                for r, a in enumerate(who):
                    n_samples = int(items[a][3])
                    total, per_win = frontend.request_audio_tokens(n_samples, self.dims)
                    out[a] = timestamps_.build_alignment(ids[r], sc[r].lp, sc[r].times, self._eos_ids(), per_win, total, n_samples / self.target_sr, self._pieces_of,
                                                         self.dims.chunk_seconds)
        return out

    def _attach_alignment(self, audios, dets, sampling_rate: int, hotwords):
        """align the decoded tokens of each Transcription and hang words / token times on it"""
        items = []
        instruction = frontend.build_instruction(hotwords)
        eos = self._eos_ids()
        from . import scoring as scoring_
        for a, det in zip(audios, dets):
            pcm, wins, n_audio = self._prepare(a, sampling_rate)
            items.append((wins, self.prompt.build(instruction, n_audio), scoring_.with_eos([int(t) for t in det.token_ids], eos, True), len(pcm)))
        for det, al in zip(dets, self._align_items(items)):
            det.words, det.token_start, det.token_end = al.words, al.token_start, al.token_end

    def align(self, audio, transcript, sampling_rate: int = 16000, hotwords: Optional[List[str]] = None):
        """When every token and word of `transcript` (a string, tokenised with the checkpoint's tokenizer, or a sequence of token ids) was spoken in `audio`: a
        timestamps.Alignment.  The prompt is the one transcribe() builds; the first EOS id is appended as a last target (its row takes part in the normalisation
        over tokens and is dropped from the result).  Needs a model built with timestamps=True."""
        return self.align_batch([audio], [transcript], sampling_rate, hotwords)[0]

    def align_batch(self, audios: Sequence[Any], transcripts: Sequence[Any], sampling_rate: int = 16000, hotwords: Optional[List[str]] = None):
        """align() for several audios, each with its transcript: as few runs as hold them, the same bits as one call per audio."""
        from . import scoring as scoring_
        if not hasattr(self, "model"):
            raise RuntimeError("ASR model has been released")
        self._check_timestamps()
        if len(audios) != len(transcripts):
            raise ValueError(f"{len(audios)} audios but {len(transcripts)} transcripts")
        instruction = frontend.build_instruction(hotwords)
        eos = self._eos_ids()
        items = []
        for a, t in zip(audios, transcripts):
            pcm, wins, n_audio = self._prepare(a, sampling_rate)
            items.append((wins, self.prompt.build(instruction, n_audio), scoring_.with_eos(self._candidate_ids(t), eos, True), len(pcm)))
        return self._align_items(items)

    def transcribe_file(self, audio, vad, vad_enabled: bool = True, hotwords: Optional[List[str]] = None,
                        max_segment_duration: Optional[float] = None, max_new_tokens: int = 256, filename: str = "", sampling_rate: int = 16000,
                        sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None, temperature=None, seed: Optional[int] = None,
                        word_timestamps: bool = False, grammar=None, top_k=None, top_p=None, min_p=None):
        """The body of the reference's /transcribe/file endpoint (main.py:193-649) as a generator of its records (dicts with the
        reference's keys: initialization, segments_summary, segment_result / segment_error in segment order, final_summary).  `audio`:
        mono int16 PCM at `sampling_rate`, or the reference's float tensor [1, N] of int16 / 32768 values; `vad`: a vad.VADProcessor.  The
        file is appended once to a device ring (resampled to 16 kHz by the append when `sampling_rate` is another rate: utils.py:18),
        VAD-scored there, and every segment is queued at once as a range of that ring on this model's scheduler; the ring is destroyed when
        the generator is exhausted or closed (filemode.py).  Sizes and times in the records are those of the 16 kHz content."""
        from . import filemode
        return filemode.transcribe_file(self, audio, vad, vad_enabled, hotwords, max_segment_duration, max_new_tokens, filename, sampling_rate,
                                        sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed,
                                        word_timestamps=word_timestamps, grammar=grammar, top_k=top_k, top_p=top_p, min_p=min_p)

    def transcribe_files(self, audios: Sequence[Any], vad, vad_enabled: bool = True, hotwords: Optional[List[str]] = None,
                         max_segment_duration: Optional[float] = None, max_new_tokens: int = 256, filenames: Optional[Sequence[str]] = None,
                         sampling_rate: int = 16000, sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None, temperature=None,
                         seed: Optional[int] = None, word_timestamps: bool = False, grammar=None, top_k=None, top_p=None, min_p=None):
        """transcribe_file for several files: all VAD passes in one device call, one record iterator per file (filemode.transcribe_files)."""
        from . import filemode
        return filemode.transcribe_files(self, audios, vad, vad_enabled, hotwords, max_segment_duration, max_new_tokens, filenames, sampling_rate,
                                         sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed,
                                         word_timestamps=word_timestamps, grammar=grammar, top_k=top_k, top_p=top_p, min_p=min_p)

    def get_model_info(self) -> Dict[str, Any]:
        """asr.py:490-513: the reference's keys for a GPU device (`cuda_version` carries the HIP runtime version: torch.version.cuda is
        the toolkit the reference's torch was built with), plus `engine`, `replicas`, `weights_mb`."""
        info = {"mode": self.mode, "device": str(self.device), "model_dtype": "torch." + self.model_dtype, "target_sampling_rate": self.target_sr,
                "checkpoint_dir": str(self.checkpoint_dir), "is_glm_asr": self.is_glm_asr}
        di = device_info(self.device_index)
        v = di["hip_runtime_version"]
        info.update({"cuda_version": f"HIP {v // 10000000}.{(v // 100000) % 100}.{v % 100000}", "gpu_name": di["name"],
                     "gpu_memory_total_mb": di["total_bytes"] / 1024 ** 2})
        info.update({"engine": "sonicscribe_amd/gfx950", "replicas": len(self.__dict__.get("models", [])), "slots_per_replica": self.__dict__.get("slots", 1), "continuous": self.__dict__.get("continuous", False), "bulk": self.__dict__.get("bulk", False),
                     "weights_mb": self.model.weight_bytes() / 1024 ** 2 if hasattr(self, "model") else 0.0})
        info["scoring"] = bool(self.__dict__.get("scoring", False))
        info["grammar"] = bool(self.__dict__.get("grammar", False))
        info["draft_verify"] = bool(self.__dict__.get("draft_verify", False))
        info["best_of"] = int(self.__dict__.get("best_of", 1))
        info["timestamps"] = bool(self.__dict__.get("timestamps", False))
        g = self.__dict__.get("generation_guards")
        if g is not None:                            # the logits processors in force: the checkpoint's generation_config.json unless the constructor overrode it
            info.update(g.as_dict())
        return info

    def close(self):
        r = self.__dict__.pop("_retrier", None)
        if r is not None:
            r.close()
        for w in self.__dict__.pop("_fork_workers", []):      # (a posted run completes first: the worker leaves behind it)
            w.close()
        c = self.__dict__.pop("_dispatcher", None)
        if c is not None:
            c.close()
        err = None
        for g in self.__dict__.pop("_grammars", []):      # (behind the dispatcher: every request has completed, so no reference is left)
            try:
                g.close()
            except Exception as ex:                      # (the engines below still close, and free it; the error is raised afterwards)
                err = err or ex
        self.__dict__.pop("model", None)
        self.__dict__.pop("_slot_engines", None)
        self.__dict__.pop("_score_engines", None)
        self.__dict__.pop("_fork_engines", None)
        for m in self.__dict__.pop("models", []):
            m.close()                                # (an engine closes its slots first)
        if err is not None:
            raise err

    def __delattr__(self, name):   # main.py:84-86 does `del asr_model.model`
        if name == "model":
            self.close()
        else:
            super().__delattr__(name)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
