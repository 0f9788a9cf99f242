"""File mode: the body of the reference's POST /transcribe/file (backend/main.py:193-649) over device-resident audio.

The reference keeps the decoded file as a host float tensor, uploads all of it for the VAD call (main.py:308-314), slices, peak-normalises
and uploads every segment again, and keeps at most three `transcribe()` calls in flight behind a semaphore (main.py:429-445).  Here the
file's int16 PCM is appended ONCE to a device ring (engine.Ring, capacity = the file); the Silero network scores it in place
(VADProcessor.detect_voice_activity_ring -> sonic_vad_probs_rings); every segment is a range of that ring handed to the model's scheduler
at once, which forms the batches; a segment's int16 -> float -> peak-normalise -> PCM_16 steps run on the device (csrc/ingest.hip), bit
identical with `transcribe()` of the same samples.

  plan_segments        get_segments (main.py:274-363) + cut_long_segments (:527-567) + get_segments_summary (:569-583): pure host code
  transcribe_file      the generator of main.py:385-483's records (dicts; the endpoint serialises them as NDJSON lines)
  transcribe_files     several files, their VAD passes in one device call

Decoding a container format (ffmpeg / pydub in the reference) stays with the host application: input is mono 16-bit PCM.  At another
rate than 16 kHz (`sampling_rate=`) the file's ring is a rate ring: the one append resamples on the device (csrc/resample.hip, the
reference's set_frame_rate(16000), utils.py:18), the flush ends the stream, and everything from there on is the 16 kHz path unchanged.
"""
from __future__ import annotations

import itertools
import math
import time
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from . import frontend, reqvalues

SAMPLE_RATE = 16000                  # config.py:22 AUDIO_SAMPLE_RATE
DEFAULT_MAX_SEGMENT_S = 30.0         # config.py:41 MAX_SEGMENT_DURATION
NO_VAD_BELOW_S = 1.0                 # main.py:290
MIN_SEGMENT_S = 0.1                  # main.py:326, :553, :606
MIN_SPAN = 100                       # main.py:323: a timestamp pair spans at least 100 samples

_file_ids = itertools.count()


# ------------------------------------------------------------------------------------------------------------------ planning (host)
def plan_segments(total_samples: int, speech_timestamps: Optional[Sequence[Dict[str, int]]], vad_enabled: bool,
                  max_segment_duration: float, sample_rate: int = SAMPLE_RATE) -> Tuple[List[Dict[str, Any]], List[Dict[str, Any]]]:
    """(final segments, their summary records) of a file of `total_samples` samples.

    speech_timestamps: what detect_voice_activity returned ([{start, end}] in samples), or None / [] for no speech; ignored when the VAD
    is off or the file is shorter than 1 s.  Each final segment carries original_index, start_sample, end_sample, start_time, end_time,
    duration, is_long_segment, sub_segment_count, sub_segment_index, 1-based segment_index and - for pieces of a cut segment -
    original_duration.  Arithmetic is the reference's: Python floats, samples / sample_rate."""
    total_samples = int(total_samples)
    total_duration = total_samples / sample_rate

    def whole():
        return [{"original_index": 1, "start_sample": 0, "end_sample": total_samples, "start_time": 0.0, "end_time": total_duration,
                 "duration": total_duration, "is_long_segment": total_duration > max_segment_duration}]

    raw: List[Dict[str, Any]] = []
    if vad_enabled and total_duration >= NO_VAD_BELOW_S and speech_timestamps:
        for idx, ts in enumerate(speech_timestamps):
            start = max(0, min(int(ts["start"]), total_samples - 1))
            end = max(start + MIN_SPAN, min(int(ts["end"]), total_samples))
            duration = (end - start) / sample_rate
            if duration > MIN_SEGMENT_S:
                raw.append({"original_index": idx + 1, "start_sample": start, "end_sample": end, "start_time": start / sample_rate,
                            "end_time": end / sample_rate, "duration": duration, "is_long_segment": duration > max_segment_duration})
    if not raw:                        # VAD off, short file, no speech, or nothing survived: the whole file
        raw = whole()
    final: List[Dict[str, Any]] = []
    for seg in raw:
        duration, start, end = seg["duration"], seg["start_sample"], seg["end_sample"]
        if duration <= max_segment_duration:
            final.append({**seg, "is_long_segment": False, "sub_segment_count": 1, "sub_segment_index": 1})
            continue
        n_sub = int(math.ceil(duration / max_segment_duration))
        per_sub = int(max_segment_duration * sample_rate)
        for k in range(n_sub):
            a = start + k * per_sub
            b = min(start + (k + 1) * per_sub, end, total_samples)
            sub_duration = (b - a) / sample_rate
            if sub_duration > MIN_SEGMENT_S:
                final.append({**seg, "start_sample": a, "end_sample": b, "start_time": a / sample_rate, "end_time": b / sample_rate,
                              "duration": sub_duration, "is_long_segment": True, "sub_segment_count": n_sub, "sub_segment_index": k + 1,
                              "original_duration": duration})
    for i, seg in enumerate(final):
        seg["segment_index"] = i + 1
    return final, segments_summary(final)


def segments_summary(segments: Sequence[Dict[str, Any]]) -> List[Dict[str, Any]]:
    return [{"segment_index": s["segment_index"], "original_index": s["original_index"], "start_time": round(s["start_time"], 3),
             "end_time": round(s["end_time"], 3), "duration": round(s["duration"], 3), "is_long_segment": s["is_long_segment"],
             "sub_segment_count": s.get("sub_segment_count", 1), "sub_segment_index": s.get("sub_segment_index", 1)} for s in segments]


def as_pcm16(audio) -> np.ndarray:
    """Mono int16 PCM of `audio`: an int16 array ([N] or [1, N]) as it is, or the reference's float tensor of int16 / 32768 values
    (audiosegment_to_tensor of a 16-bit file).  Any other float content is refused: decoding files is not done here."""
    a = audio.detach().cpu().numpy() if hasattr(audio, "detach") else np.asarray(audio)
    if a.ndim == 2 and a.shape[0] == 1:
        a = a[0]
    if a.ndim != 1:
        raise ValueError(f"file mode takes mono audio ([N] or [1, N]), got shape {tuple(a.shape)}")
    if a.dtype == np.int16:
        return np.ascontiguousarray(a)
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"file mode takes int16 PCM or a float tensor of int16 / 32768 values, got dtype {a.dtype}")
    scaled = a.astype(np.float64) * 32768.0
    pcm = np.rint(scaled)
    if a.size and (not np.isfinite(scaled).all() or (pcm != scaled).any() or pcm.min() < -32768 or pcm.max() > 32767):
        raise ValueError("file mode: the float audio is not int16 / 32768 (16-bit mono PCM) - decode the file to 16-bit PCM first (ffmpeg "
                         "in the reference) and pass its rate as sampling_rate=; nothing is rounded or rescaled here")
    return pcm.astype(np.int16)


# ------------------------------------------------------------------------------------------------------------------ one file
class _FileJob:
    """One file on the device: its ring, its plan and its queued decodes."""

    def __init__(self, model, call: reqvalues.CallKeywords, audio, vad, vad_enabled: bool, hotwords, max_segment_duration, max_new_tokens: int, filename: str,
                 sampling_rate: int = SAMPLE_RATE, word_timestamps: bool = False):
        if not hasattr(model, "model"):
            raise RuntimeError("ASR model has been released")
        # word_timestamps (a model built with timestamps=True): every segment's tokens are aligned on the replica's scoring handle as its record is
        # made, from the same ring ranges; `words` in the record are on the file's clock (offset by the segment's start)
        self.word_timestamps = bool(word_timestamps)
        if self.word_timestamps:
            model._check_timestamps()
        # the file's temperature (a float) or fallback ladder (a sequence) and seed (a model built with sampling=True; ASRModel._request_sampling): every segment
        # of the file is decoded with them, each as its own request
        samp = model._request_sampling(call.temperature, call.seed, cut=(call.top_k, call.top_p, call.min_p)) if hasattr(model, "_request_sampling") else None
        # the file's sequence-bias table (a model built with request_bias=True; ASRModel._request_bias): every segment of the file carries it
        bias = model._request_bias(hotwords, call.sequence_bias, call.bad_words_ids, call.hotword_boost) if hasattr(model, "_request_bias") else None
        # the file's grammar (a model built with grammar=True; ASRModel.compile_grammar): every segment of the file is decoded under it, from its start node
        gram = model._request_grammar(call.grammar) if call.grammar is not None else None
        self.values = reqvalues.CallValues(bias, samp, gram)      # (resolved in file mode's own order: sampling ahead of the table; no draft, one sample)
        self.model, self.filename = model, filename
        self.vad_enabled, self.hotwords = bool(vad_enabled), list(hotwords) if hotwords else None
        self.max_seg = float(max_segment_duration or DEFAULT_MAX_SEGMENT_S)
        self.max_new = int(max_new_tokens)
        self.t0 = time.time()
        pcm = as_pcm16(audio)
        if pcm.size == 0:
            raise ValueError("file mode: empty audio")
        self.sr = model.target_sr
        self.in_rate = int(sampling_rate)
        # a file at another rate: its 16 kHz length is the resampler's trim, ceil(nf * N / of); every record counts the 16 kHz content
        self.total = int(pcm.size)
        if self.in_rate != self.sr:
            of, nf, _, _ = frontend.resample_geometry(self.in_rate, self.sr)
            self.total = -(-nf * int(pcm.size) // of)
        self.duration = self.total / self.sr
        self.replica = model._dispatcher.home(f"file:{next(_file_ids)}:{filename}")
        if self.wants_vad:
            # the VAD handle reads the ring in place, so the file lives on the handle's GPU (a ring elsewhere would be refused)
            dev = getattr(vad, "device_id", 0)
            if dev not in model.device_indices:
                raise ValueError(f"file mode: the VADProcessor is on device {dev}, the model on {model.device_indices}: build the VADProcessor "
                                 "with device_id= one of the model's GPUs")
            self.replica = model.device_indices.index(dev)
        eng = model.models[self.replica]
        self.ring = eng.ring_create(max(1024, self.total)) if self.in_rate == self.sr else eng.ring_create(max(1024, self.total), rate=self.in_rate)
        try:
            self.first = self.ring.append(pcm)      # the file's only copy on the device
            if self.in_rate != self.sr:
                self.ring.flush()
                if self.ring.head - self.first != self.total:
                    raise RuntimeError(f"file mode: the rate ring holds {self.ring.head - self.first} samples, expected {self.total}")
        except BaseException:
            self.release()
            raise
        if self.word_timestamps and samp is not None and samp.ladder:
            self.release()
            raise ValueError("word_timestamps is not supported with a fallback ladder of temperatures in file mode (the ladder's futures carry texts, not tokens): pass one temperature")
        self.futures: List[Any] = []
        self.requests: List[Any] = []          # word_timestamps: per segment (windows, prompt, samples), None for a segment that was refused
        self.segments: List[Dict[str, Any]] = []
        self.summary: List[Dict[str, Any]] = []

    @property
    def wants_vad(self) -> bool:
        return self.vad_enabled and self.duration >= NO_VAD_BELOW_S

    def plan(self, timestamps) -> None:
        self.segments, self.summary = plan_segments(self.total, timestamps, self.vad_enabled, self.max_seg, self.sr)

    def submit_all(self) -> None:
        """every segment at once: the scheduler forms the batches (no three-way semaphore)"""
        m = self.model
        instruction = frontend.build_instruction(self.hotwords)
        for seg in self.segments:
            a, n = seg["start_sample"], seg["end_sample"] - seg["start_sample"]
            if n < int(MIN_SEGMENT_S * self.sr):
                # the reference's segment_error for this case (main.py:606-607); its keys, this package's own wording of the text
                self.futures.append(ValueError(f"segment {seg['segment_index']} has too few samples: {n}"))
                self.requests.append(None)
                continue
            # > 30 s: one request of several windows sharing one peak, as transcribe() makes it (frontend.split_windows)
            windows = [self.ring.slice(self.first + a + s, e - s) for s, e in frontend.split_windows(n, m.dims)]
            n_audio, _ = frontend.request_audio_tokens(n, m.dims)
            self.requests.append((windows, m.prompt.build(instruction, n_audio), n))
            if self.values.samp is not None and not self.word_timestamps:      # (a future of the TEXT: the ladder judges texts; records() takes either)
                self.futures.append(m._dispatch(windows, m.prompt.build(instruction, n_audio), self.max_new, False, self.values, replica=self.replica))
                continue
            # the scheduler's own future carries the tokens (with word_timestamps: at the file's one temperature; a ladder was refused when the job was made)
            self.futures.append(m._dispatcher.submit(windows, m.prompt.build(instruction, n_audio), self.max_new, replica=self.replica,
                                                     **reqvalues.submit_keywords(self.values)))

    def records(self) -> Iterator[Dict[str, Any]]:
        total_segments = len(self.segments)
        hot = self.hotwords or []
        try:
            yield {"type": "initialization", "filename": self.filename, "file_size": self.total * 2, "total_duration": round(self.duration, 2),
                   "total_segments": total_segments,
                   "config": {"vad_enabled": self.vad_enabled, "hotwords": hot, "max_segment_duration": self.max_seg}, "timestamp": time.time()}
            yield {"type": "segments_summary", "segments": self.summary, "total_segments": total_segments, "timestamp": time.time()}
            ok = bad = 0
            for i_seg, (seg, fut) in enumerate(zip(self.segments, self.futures)):
                try:
                    if isinstance(fut, Exception):
                        raise fut
                    got = fut.result()
                    text = got if isinstance(got, str) else self.model.prompt.decode(got).strip()
                    words = None
                    if self.word_timestamps:
                        from . import scoring as scoring_
                        wins, prompt, n = self.requests[i_seg]
                        al = self.model._align_items([(wins, prompt, scoring_.with_eos([int(t) for t in got], self.model._eos_ids(), True), n)], replica=self.replica)[0]
                        words = [w.as_dict() for w in al.shifted(seg["start_time"]).words]
                    rec = {"type": "segment_result", "segment_index": seg["segment_index"], "original_index": seg["original_index"],
                           "start_time": round(seg["start_time"], 3), "end_time": round(seg["end_time"], 3), "duration": round(seg["duration"], 3),
                           "text": text, "processing_time": 0, "is_long_segment": seg["is_long_segment"], "hotwords_used": hot,
                           "timestamp": time.time()}
                    if words is not None:
                        rec["words"] = words
                    ok += 1
                except Exception as ex:
                    rec = {"type": "segment_error", "segment_index": seg["segment_index"], "original_index": seg["original_index"],
                           "error": str(ex), "is_long_segment": seg["is_long_segment"], "timestamp": time.time()}
                    bad += 1
                rec["progress"] = round((ok + bad) / total_segments * 100, 1)
                yield rec
            yield {"type": "final_summary", "total_segments": total_segments, "successful_segments": ok, "failed_segments": bad,
                   "total_duration": round(self.duration, 2), "processing_time": round(time.time() - self.t0, 2), "completed_at": time.time(),
                   "message": "转录完成", "hotwords_used": hot, "vad_enabled": self.vad_enabled}
        finally:
            self.release()

    def release(self) -> None:
        """queued decodes are cancelled, the ring goes back to the driver (a request that already stages from it finishes first:
        sonic_ring_destroy waits for the ring's lock)"""
        for f in getattr(self, "futures", []):
            if hasattr(f, "cancel"):
                f.cancel()
        ring, self.ring = getattr(self, "ring", None), None
        if ring is not None:
            ring.close()


class FileRecords:
    """Iterator of one file's records.  The file's device ring is destroyed when it is exhausted, closed or collected - also when it was
    never started (a plain generator would not run its `finally` then)."""

    def __init__(self, job: _FileJob):
        self._job, self._gen = job, job.records()

    def __iter__(self):
        return self

    def __next__(self) -> Dict[str, Any]:
        return next(self._gen)

    def close(self) -> None:
        self._gen.close()
        self._job.release()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _detect(vad, jobs: Sequence[_FileJob]) -> List[Any]:
    """speech timestamps of every job that wants the VAD, all files in ONE device call (the recurrence kernel runs a block per sequence).
    A failing VAD call raises: the reference's fall-back to the whole file (main.py:352-363) would hide a refused ring or a lost device."""
    from . import vad_net
    out: List[Any] = [None] * len(jobs)
    live = [i for i, j in enumerate(jobs) if j.wants_vad]
    thr = vad.threshold
    by_engine: Dict[int, List[int]] = {}
    for i in live:
        by_engine.setdefault(jobs[i].replica, []).append(i)
    for idx in by_engine.values():
        probs = vad.probs_rings(jobs[idx[0]].ring.engine, [[(jobs[i].ring, jobs[i].first, jobs[i].total)] for i in idx])
        for i, p in zip(idx, probs):
            out[i] = vad_net.speech_timestamps(p, jobs[i].total, thr, int(vad.min_speech_duration * 1000), float("inf"),
                                               int(vad.max_silence_duration * 1000))
    return out


def transcribe_file(model, call: reqvalues.CallKeywords, audio, vad, vad_enabled: bool = True, hotwords: Optional[List[str]] = None,
                    max_segment_duration: Optional[float] = None, max_new_tokens: int = 256, filename: str = "",
                    sampling_rate: int = SAMPLE_RATE, word_timestamps: bool = False) -> Iterator[Dict[str, Any]]:
    """Generator of the reference's file-mode records for one file (see ASRModel.transcribe_file, which builds `call` from its keywords)."""
    job = _FileJob(model, call, audio, vad, vad_enabled, hotwords, max_segment_duration, max_new_tokens, filename, sampling_rate, word_timestamps)
    try:
        ts = vad.detect_voice_activity_ring(job.ring, job.first, job.total)[0] if job.wants_vad else None
        job.plan(ts)
        job.submit_all()
    except BaseException:
        job.release()
        raise
    yield from job.records()


def transcribe_files(model, call: reqvalues.CallKeywords, audios: Sequence[Any], vad, vad_enabled: bool = True, hotwords: Optional[List[str]] = None,
                     max_segment_duration: Optional[float] = None, max_new_tokens: int = 256,
                     filenames: Optional[Sequence[str]] = None, sampling_rate: int = SAMPLE_RATE, word_timestamps: bool = False) -> List[FileRecords]:
    """One record iterator per file; the VAD of all files runs in one device call and every file's segments are queued before the call
    returns.  Each iterator must be exhausted or closed (its ring lives until then)."""
    names = list(filenames) if filenames is not None else [""] * len(audios)
    jobs: List[_FileJob] = []
    try:
        for a, name in zip(audios, names):
            jobs.append(_FileJob(model, call, a, vad, vad_enabled, hotwords, max_segment_duration, max_new_tokens, name, sampling_rate, word_timestamps))
        for job, ts in zip(jobs, _detect(vad, jobs)):
            job.plan(ts)
        for job in jobs:
            job.submit_all()
    except BaseException:
        for job in jobs:
            job.release()
        raise
    return [FileRecords(j) for j in jobs]
