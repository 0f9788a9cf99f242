"""The Silero VAD network (silero-vad 5.x / 6.x, `load_silero_vad()`, 16 kHz branch) as the reference runs it (backend/vad.py:84-126):
its weight layout, a synthetic weight set, and the post-processing of `get_speech_timestamps` on given probabilities.  Pure numpy.

The network (csrc/vad.hip runs it; tests/vad_torch_ref.py restates it with torch.nn layers):
    window     64 samples of context (the last 64 of the previous window's 576; zeros for a sequence's first window) + 512 new = 576
    STFT       reflection pad right by 64 -> 640; conv1d with stft.forward_basis_buffer [258, 1, 256], stride 128 -> [258, 4];
               magnitude sqrt(re^2 + im^2) of rows 0..128 / 129..257 -> [129, 4]
    encoder    4 x (conv1d k3 p1 + ReLU): 129 -> 128 (s1), -> 64 (s2), -> 64 (s2), -> 128 (s1); time 4 -> 4 -> 2 -> 1 -> 1
    LSTMCell   128 -> 128 (gates i, f, g, o), state carried across the windows of one sequence
    head       sigmoid(conv1d k1 (relu(h))) = the window's speech probability
A sequence of n samples is ceil(n / 512) windows, the last zero-padded (get_speech_timestamps).  The 8 kHz sub-model (`_model_8k.`) is
never run by the reference (it resamples to 16 kHz first, vad.py:60-67,104-111) and is not built.
"""
from __future__ import annotations

import math
from typing import Dict, List, Mapping, Tuple

import numpy as np

WINDOW = 512          # new samples per window at 16 kHz
CONTEXT = 64
PREFIX = "_model."
PREFIX_8K = "_model_8k."

# name (after `_model.`) -> shape; the order is the one csrc/vad.cpp keeps
LAYOUT: Dict[str, Tuple[int, ...]] = {
    "stft.forward_basis_buffer": (258, 1, 256),
    "encoder.0.reparam_conv.weight": (128, 129, 3), "encoder.0.reparam_conv.bias": (128,),
    "encoder.1.reparam_conv.weight": (64, 128, 3), "encoder.1.reparam_conv.bias": (64,),
    "encoder.2.reparam_conv.weight": (64, 64, 3), "encoder.2.reparam_conv.bias": (64,),
    "encoder.3.reparam_conv.weight": (128, 64, 3), "encoder.3.reparam_conv.bias": (128,),
    "decoder.rnn.weight_ih": (512, 128), "decoder.rnn.bias_ih": (512,),
    "decoder.rnn.bias_hh": (512,), "decoder.rnn.weight_hh": (512, 128),
    "decoder.decoder.2.weight": (1, 128, 1), "decoder.decoder.2.bias": (1,),
}


def n_windows(n_samples: int) -> int:
    return -(-int(n_samples) // WINDOW)


def weights_from_state_dict(sd: Mapping[str, object]) -> Dict[str, np.ndarray]:
    """load_silero_vad()'s state dict (TorchScript `state_dict()`; torch tensors or arrays) -> {LAYOUT name: fp32 array}.  `_model.` is
    stripped, `_model_8k.` ignored; any other key, a missing name or a wrong shape raises ValueError."""
    out: Dict[str, np.ndarray] = {}
    for k, v in sd.items():
        if k.startswith(PREFIX_8K):
            continue
        if not k.startswith(PREFIX) or k[len(PREFIX):] not in LAYOUT:
            raise ValueError(f"silero VAD state dict: unexpected tensor {k!r}")
        name = k[len(PREFIX):]
        a = np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v), dtype=np.float32)
        if a.shape != LAYOUT[name]:
            raise ValueError(f"silero VAD state dict: {k} has shape {a.shape}, expected {LAYOUT[name]}")
        out[name] = a
    missing = [PREFIX + n for n in LAYOUT if n not in out]
    if missing:
        raise ValueError(f"silero VAD state dict: missing {missing}")
    return out


# gains for synthetic_weights that make the untrained network's output move with the signal (tone / noise -> high, silence -> low) and
# cross the reference's thresholds; at the default initialisation every window scores about 0.48
RESPONSIVE = dict(scale_encoder=4.0, scale_rnn=2.0, scale_head=20.0)


def synthetic_weights(seed: int, scale_encoder: float = 1.0, scale_rnn: float = 1.0, scale_head: float = 1.0) -> Dict[str, np.ndarray]:
    """PyTorch-default-initialised tensors (Conv1d / LSTMCell: U(-1/sqrt(fan_in), 1/sqrt(fan_in)); LSTMCell fan_in = hidden size) and a
    Hann-windowed DFT basis (the layout of silero's STFT buffer); the encoder weights, the LSTM weight matrices and the head are
    multiplied by the given gains.  For tests and tools: not the trained model."""
    rng = np.random.default_rng(seed)
    w: Dict[str, np.ndarray] = {}
    k = np.arange(256)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * k / 256)
    f = np.arange(129)[:, None]
    w["stft.forward_basis_buffer"] = np.concatenate([hann * np.cos(2 * np.pi * f * k / 256), -hann * np.sin(2 * np.pi * f * k / 256)])[:, None, :]
    for name, shape in LAYOUT.items():
        if name.startswith("encoder") or name.startswith("decoder.decoder"):
            fan_in = int(np.prod(shape[1:])) if name.endswith("weight") else int(np.prod(LAYOUT[name.replace("bias", "weight")][1:]))
        elif name.startswith("decoder.rnn"):
            fan_in = 128
        else:
            continue
        bound = 1.0 / math.sqrt(fan_in)
        w[name] = rng.uniform(-bound, bound, size=shape)
        if name.startswith("encoder") and name.endswith("weight"):
            w[name] *= scale_encoder
        elif name.startswith("decoder.rnn.weight"):
            w[name] *= scale_rnn
        elif name.startswith("decoder.decoder"):
            w[name] *= scale_head
    return {n: np.ascontiguousarray(w[n], dtype=np.float32) for n in LAYOUT}


def speech_timestamps(probs, n_samples: int, threshold: float = 0.5, min_speech_ms: int = 250, max_speech_s: float = float("inf"),
                      min_silence_ms: int = 100, speech_pad_ms: int = 30, sampling_rate: int = 16000) -> List[Dict[str, int]]:
    """silero's `get_speech_timestamps` (utils_vad.py) after its model loop, on the per-window probabilities of one sequence of
    n_samples samples (16 kHz, 512-sample windows): neg_threshold = max(threshold - 0.15, 0.01), segment ends after min_silence of
    sub-neg_threshold windows, segments of at most min_speech dropped, an open segment closed at the end of the audio, speech_pad
    added / split between close segments.  The max-speech split is not restated: both reference callers make it unreachable
    (vad.py:73-77: inf; :117-121: 14 528 samples > a 10 240-sample window) - NotImplementedError if it could fire here."""
    probs = np.asarray(probs, np.float64)
    ws = WINDOW
    if probs.shape != (n_windows(n_samples),):
        raise ValueError(f"{probs.shape[0]} probabilities for {n_samples} samples (expected {n_windows(n_samples)})")
    min_speech_samples = sampling_rate * min_speech_ms / 1000
    speech_pad_samples = sampling_rate * speech_pad_ms / 1000
    max_speech_samples = sampling_rate * max_speech_s - ws - 2 * speech_pad_samples
    min_silence_samples = sampling_rate * min_silence_ms / 1000
    if ws * (len(probs) - 1) > max_speech_samples:
        raise NotImplementedError("get_speech_timestamps' max-speech split is not restated (neither reference caller reaches it)")
    neg_threshold = max(threshold - 0.15, 0.01)
    triggered, temp_end = False, 0
    speeches: List[Dict[str, int]] = []
    cur: Dict[str, int] = {}
    for i, p in enumerate(probs):
        if p >= threshold and temp_end:
            temp_end = 0
        if p >= threshold and not triggered:
            triggered = True
            cur["start"] = ws * i
            continue
        if p < neg_threshold and triggered:
            if not temp_end:
                temp_end = ws * i
            if ws * i - temp_end < min_silence_samples:
                continue
            cur["end"] = temp_end
            if cur["end"] - cur["start"] > min_speech_samples:
                speeches.append(cur)
            cur, temp_end, triggered = {}, 0, False
    if cur and n_samples - cur["start"] > min_speech_samples:
        cur["end"] = n_samples
        speeches.append(cur)
    for i, sp in enumerate(speeches):
        if i == 0:
            sp["start"] = int(max(0, sp["start"] - speech_pad_samples))
        if i != len(speeches) - 1:
            gap = speeches[i + 1]["start"] - sp["end"]
            if gap < 2 * speech_pad_samples:
                sp["end"] += int(gap // 2)
                speeches[i + 1]["start"] = int(max(0, speeches[i + 1]["start"] - gap // 2))
            else:
                sp["end"] = int(min(n_samples, sp["end"] + speech_pad_samples))
                speeches[i + 1]["start"] = int(max(0, speeches[i + 1]["start"] - speech_pad_samples))
        else:
            sp["end"] = int(min(n_samples, sp["end"] + speech_pad_samples))
    return speeches


# the reference's two parameter sets (backend/vad.py:69-77 and :113-121), as speech_timestamps keyword arguments
FILE_PARAMS = dict(min_speech_ms=300, max_speech_s=float("inf"), min_silence_ms=1000)
CHUNK_PARAMS = dict(min_speech_ms=100, max_speech_s=1.0, min_silence_ms=100)
