"""VADProcessor: a drop-in for the reference's backend/vad.py class with the Silero network on the GPU (sonic_vad_* of
include/sonic_hip.h, csrc/vad.hip).  Construction, thresholds and both detection methods keep the reference's signatures and parameters;
what `get_speech_timestamps` does after its model loop is vad_net.speech_timestamps.  New: `is_voice_active_batch` scores the windows of
many sessions in one device call, and `scorer()` is the `vad` argument of sessions.GatedSessions.tick.  Audio that already lies in device
rings (engine.Ring) is scored in place: `probs_rings`, `detect_voice_activity_ring` (file mode, filemode.py) and `ring_scorer()` (the `vad`
argument of a GatedSessions built with device_vad=True).

Swap in the reference (models_manager.vad_model_init, models_manager.py:49): `_vad_processor = sonicscribe_amd.vad.VADProcessor()`.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from . import engine, frontend, vad_net


class VADProcessor:
    def __init__(self, threshold: float = 0.5, sampling_rate: int = 16000, weights: Union[None, str, Mapping[str, object]] = None,
                 device_id: int = 0, max_windows: int = 4096):
        """weights: a state dict of load_silero_vad() (keys `_model.*`; `_model_8k.*` ignored), a path to the silero TorchScript file, or
        None = silero_vad.load_silero_vad() when the package is importable.  Raises ValueError for a rate other than 8000 / 16000
        (vad.py:21-22) and RuntimeError when the HIP library or the GPU is missing (no CPU fallback)."""
        self.sampling_rate = sampling_rate
        self.device_id = int(device_id)
        self.threshold = threshold
        self.min_speech_duration = 0.3      # vad.py:16-17
        self.max_silence_duration = 1.0
        self.vad_iterator = None
        if self.sampling_rate not in [8000, 16000]:
            raise ValueError("sampling_rate must be 8000 or 16000 Hz")
        self.weights = vad_net.weights_from_state_dict(_state_dict(weights))
        self.lib = engine.load_library()
        h = C.c_void_p()
        rc = self.lib.sonic_vad_create(int(device_id), int(max_windows), C.byref(h))
        if rc != 0:
            raise RuntimeError(f"sonic_vad_create failed ({rc}): " + (self.lib.sonic_vad_last_error(None) or b"").decode())
        self.h = h
        self._lock = threading.Lock()       # close() against calls; the handle serialises calls itself
        for name, a in self.weights.items():
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._check(self.lib.sonic_vad_load_tensor(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim))

    # ---- device ---------------------------------------------------------------------------------------------------------------------
    def _check(self, rc: int) -> None:
        if rc != 0:
            raise RuntimeError(f"sonic_vad failed ({rc}): " + (self.lib.sonic_vad_last_error(self.h) or b"").decode())

    def probs(self, seqs: Sequence[np.ndarray]) -> List[np.ndarray]:
        """Per-window speech probabilities of each 16 kHz sequence, all in one device call.  The sequences must share a dtype: int16
        (scored as x / 32768) or float (divided by max|x| when that exceeds 1, vad.py:24-38)."""
        seqs = list(seqs)
        if not seqs:
            return []
        is_i16 = seqs[0].dtype == np.int16
        dt = np.int16 if is_i16 else np.float32
        if any((s.dtype == np.int16) != is_i16 for s in seqs):
            raise ValueError("VADProcessor.probs: int16 and float sequences in one call")
        lens = np.array([len(s) for s in seqs], np.int64)
        off = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        pcm = np.concatenate([np.asarray(s, dt).reshape(-1) for s in seqs]) if off[-1] else np.zeros(1, dt)
        nw = np.array([vad_net.n_windows(n) for n in lens], np.int64)
        out = np.zeros(max(1, int(nw.sum())), np.float32)
        p = pcm.ctypes.data_as(C.c_void_p)
        with self._lock:
            if self.h is None:
                raise RuntimeError("VADProcessor is closed")
            self._check(self.lib.sonic_vad_probs(self.h, p if is_i16 else None, None if is_i16 else p,
                                                 off.ctypes.data_as(C.c_void_p), len(seqs), out.ctypes.data_as(C.c_void_p)))
        return np.split(out[:int(nw.sum())], np.cumsum(nw)[:-1])

    def probs_rings(self, engine_or_model, sequences: Sequence[Sequence[Tuple[object, int, int]]]) -> List[np.ndarray]:
        """probs() of sequences that lie in device rings, read in place (sonic_vad_probs_rings): each sequence is a list of pieces
        `(ring, first_sample, n)` and is scored as the int16 concatenation of its pieces would be by probs(), bit for bit.
        engine_or_model: the Engine (or a slot of it, or the ASRModel) that owns the rings; None = the engine of the first ring."""
        sequences = [list(sq) for sq in sequences]
        if not sequences:
            return []
        pieces = [pc for sq in sequences for pc in sq]
        eng = engine_or_model
        if eng is None:
            if not pieces:
                return [np.zeros(0, np.float32) for _ in sequences]
            eng = pieces[0][0].engine
        elif hasattr(eng, "models"):                # an ASRModel: the replica that owns the rings
            owners = {id(pc[0].engine.root) for pc in pieces}
            eng = next((m for m in eng.models if id(m.root) in owners), eng.models[0])
        if self.sampling_rate != 16000:
            raise ValueError("VADProcessor.probs_rings: rings hold 16 kHz audio; this processor was built for another rate")
        seq_piece = np.zeros(len(sequences) + 1, np.int64)
        np.cumsum([len(sq) for sq in sequences], out=seq_piece[1:])
        P = len(pieces)
        rings = (C.c_void_p * max(1, P))(*[pc[0].h for pc in pieces])
        start = np.array([int(pc[1]) for pc in pieces] or [0], np.int64)
        n = np.array([int(pc[2]) for pc in pieces] or [0], np.int32)
        nw = np.array([vad_net.n_windows(sum(int(pc[2]) for pc in sq)) for sq in sequences], np.int64)
        out = np.zeros(max(1, int(nw.sum())), np.float32)
        with self._lock:
            if self.h is None:
                raise RuntimeError("VADProcessor is closed")
            if eng.h is None:
                raise RuntimeError("VADProcessor.probs_rings: the engine is closed")
            self._check(self.lib.sonic_vad_probs_rings(self.h, eng.h, rings, start.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p),
                                                       seq_piece.ctypes.data_as(C.c_void_p), len(sequences), out.ctypes.data_as(C.c_void_p)))
        return np.split(out[:int(nw.sum())], np.cumsum(nw)[:-1])

    def _to16k(self, audio) -> np.ndarray:
        """vad.py:24-38 and :60-67 / :104-111: float, peak-normalised only above 1, resampled to 16 kHz"""
        a = audio.detach().cpu().numpy() if hasattr(audio, "detach") else np.asarray(audio)
        a = np.asarray(a, np.float32).reshape(-1)
        if self.sampling_rate != 16000:
            if a.size and np.abs(a).max() > 1.0:
                a = a / np.abs(a).max()
            a = frontend.resample_sinc_hann(a, self.sampling_rate, 16000)
        return a

    # ---- the reference's interface --------------------------------------------------------------------------------------------------
    def detect_voice_activity(self, audio_tensor, threshold: Optional[float] = None) -> Tuple[List[Dict[str, int]], bool]:
        """vad.py:41-82: (speech timestamps in samples at 16 kHz, any speech) over the whole buffer."""
        if threshold is None:
            threshold = self.threshold
        a = self._to16k(audio_tensor)
        if a.size == 0:
            return [], False
        ts = vad_net.speech_timestamps(self.probs([a])[0], a.size, threshold, int(self.min_speech_duration * 1000), float("inf"),
                                       int(self.max_silence_duration * 1000))
        return ts, len(ts) > 0

    def detect_voice_activity_ring(self, ring, first: int, n: int, threshold: Optional[float] = None) -> Tuple[List[Dict[str, int]], bool]:
        """detect_voice_activity over samples [first, first + n) of a device ring (int16 wire PCM, scored as x / 32768 - what the
        reference's float file tensor holds): the same timestamps logic on probabilities computed where the audio already is."""
        if threshold is None:
            threshold = self.threshold
        n = int(n)
        if n == 0:
            return [], False
        ts = vad_net.speech_timestamps(self.probs_rings(ring.engine, [[(ring, int(first), n)]])[0], n, threshold,
                                       int(self.min_speech_duration * 1000), float("inf"), int(self.max_silence_duration * 1000))
        return ts, len(ts) > 0

    def is_voice_active(self, audio_chunk, threshold: Optional[float] = None) -> bool:
        """vad.py:84-126: does the chunk hold speech (get_speech_timestamps with 100 ms / 1 s / 100 ms)."""
        if not (isinstance(audio_chunk, np.ndarray) or hasattr(audio_chunk, "detach")):
            raise ValueError("audio chunk must be a numpy array or a torch tensor")
        if threshold is None:
            threshold = self.threshold
        return bool(self.is_voice_active_batch([self._to16k(audio_chunk)], [threshold])[0])

    def set_threshold(self, threshold: float) -> None:
        if not 0.0 <= threshold <= 1.0:
            raise ValueError("threshold must be between 0.0 and 1.0")
        self.threshold = threshold

    def get_threshold(self) -> float:
        return self.threshold

    def reset(self) -> None:
        self.vad_iterator = None

    # ---- batched ----------------------------------------------------------------------------------------------------------------------
    def is_voice_active_batch(self, pcm_list: Sequence[np.ndarray], thresholds) -> np.ndarray:
        """is_voice_active of every chunk (16 kHz; int16 as the gate's windows, or float) at its own threshold, all windows in one
        sonic_vad_probs call.  An empty chunk is no speech."""
        thr = np.broadcast_to(np.asarray(thresholds, np.float64), (len(pcm_list),))
        out = np.zeros(len(pcm_list), bool)
        live = [i for i, p in enumerate(pcm_list) if len(p)]
        if not live:
            return out
        seqs = [np.asarray(pcm_list[i]).reshape(-1) for i in live]
        if any(s.dtype != np.int16 for s in seqs):
            seqs = [s.astype(np.float32) / 32768.0 if s.dtype == np.int16 else s.astype(np.float32) for s in seqs]
        for i, s, p in zip(live, seqs, self.probs(seqs)):
            out[i] = len(vad_net.speech_timestamps(p, len(s), float(thr[i]), **vad_net.CHUNK_PARAMS)) > 0
        return out

    def scorer(self):
        """The `vad(rows, pcm, thresholds) -> bool[len(rows)]` callable of sessions.GatedSessions.tick: the windows of one tick in one
        device call (what vad_processor_manager.py:95-104 does per session: int16 / 32768 -> is_voice_active at the dynamic threshold)."""
        def vad(rows, pcm, thr):
            return self.is_voice_active_batch(pcm, thr)
        return vad

    def ring_scorer(self):
        """The `vad` callable of a sessions.GatedSessions built with device_vad=True: there the second argument carries, per row, the
        ring pieces `(ring, first_sample, n)` of the gate's window ids and no bytes; the windows of one tick are scored in place in
        one sonic_vad_probs_rings call per engine replica (the pieces name their rings themselves)."""
        def vad(rows, pieces, thr):
            thr = np.broadcast_to(np.asarray(thr, np.float64), (len(pieces),))
            out = np.zeros(len(pieces), bool)
            by_engine: Dict[int, List[int]] = {}
            for i, sq in enumerate(pieces):
                if sum(int(pc[2]) for pc in sq) > 0:
                    by_engine.setdefault(id(sq[0][0].engine.root), []).append(i)
            for live in by_engine.values():
                for i, p in zip(live, self.probs_rings(pieces[live[0]][0][0].engine, [pieces[i] for i in live])):
                    n = sum(int(pc[2]) for pc in pieces[i])
                    out[i] = len(vad_net.speech_timestamps(p, n, float(thr[i]), **vad_net.CHUNK_PARAMS)) > 0
            return out
        return vad

    def close(self) -> None:
        with self._lock:
            if getattr(self, "h", None) is not None:
                self.lib.sonic_vad_destroy(self.h)
                self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _state_dict(weights) -> Mapping[str, object]:
    if weights is None:
        try:
            from silero_vad import load_silero_vad
        except ImportError as e:
            raise RuntimeError("VADProcessor: the silero_vad package is not importable - pass weights= (a state dict of "
                               "silero_vad.load_silero_vad(), or the path of its silero_vad.jit file)") from e
        return load_silero_vad().state_dict()
    if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
        import torch
        return torch.jit.load(weights, map_location="cpu").state_dict()
    if all(not str(k).startswith(vad_net.PREFIX) for k in weights) and set(weights) == set(vad_net.LAYOUT):
        return {vad_net.PREFIX + k: v for k, v in weights.items()}      # already in LAYOUT names (vad_net.synthetic_weights)
    return weights
