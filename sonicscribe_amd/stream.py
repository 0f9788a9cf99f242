"""A streaming session whose audio stays on the device: the ring that takes its wire chunks, and the decodes of chunk / sample ranges of it (ASRModel.open_stream)."""
from __future__ import annotations

import asyncio
import time
from concurrent.futures import Future
from typing import Dict, List, Optional

from . import frontend
from .reqvalues import CallKeywords


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
        return self._submit(CallKeywords(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed, grammar=grammar, draft=draft, top_k=top_k, top_p=top_p, min_p=min_p), first, n, max_new_tokens, hotwords, detailed, word_timestamps)

    def _submit(self, call: CallKeywords, first: int, n: int, max_new_tokens: int, hotwords, detailed: bool, word_timestamps: bool) -> "Future[str]":
        """submit_samples behind its keywords"""
        m = self.model
        if word_timestamps:
            raise ValueError("word_timestamps is not supported on submit() / transcribe_async() / stream decodes: align a finished transcript with ASRModel.align(), or use transcribe(..., word_timestamps=True)")
        m._check_detailed(detailed)
        values = m._request_values(call, hotwords, int(max_new_tokens), ladder_ok=False)      # (no best_of: a stream decode is one row)
        windows = [self.ring.slice(first + s, e - s) for s, e in frontend.split_windows(n, m.dims)]
        n_audio, _ = frontend.request_audio_tokens(n, m.dims)
        prompt = m.prompt.build(frontend.build_instruction(hotwords), n_audio)
        return m._dispatch(windows, prompt, int(max_new_tokens), detailed, values, replica=self.replica)

    def submit_chunks(self, start_chunk_id: int, end_chunk_id: int, max_new_tokens: int = 128, hotwords: Optional[List[str]] = None,
                      detailed: bool = False, sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None,
                      temperature: Optional[float] = None, seed: Optional[int] = None, word_timestamps: bool = False, grammar=None, draft=None, top_k=None, top_p=None, min_p=None) -> "Future[str]":
        """Transcribe chunks start..end inclusive (audio_manager.py:76-79 get_chunks_by_range + :115-123 concatenation)."""
        call = CallKeywords(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed, grammar=grammar, draft=draft, top_k=top_k, top_p=top_p, min_p=min_p)
        first, n = self.chunk_range_samples(start_chunk_id, end_chunk_id)
        return self._submit(call, first, n, max_new_tokens, hotwords, detailed, word_timestamps)

    async def transcribe_chunks(self, start_chunk_id: int, end_chunk_id: int, max_new_tokens: int = 128, hotwords: Optional[List[str]] = None) -> str:
        return await asyncio.wrap_future(self.submit_chunks(start_chunk_id, end_chunk_id, max_new_tokens, hotwords))

    def close(self):
        self.ring.close()
        self._chunks.clear()

