"""The Silero VAD network (sonicscribe_amd/vad_net.py's table) restated with torch.nn layers in float64: ReflectionPad1d, F.conv1d for the
STFT, nn.Conv1d encoder, nn.LSTMCell, and silero's model-loop bookkeeping (512-sample windows, the last zero-padded, 64 samples of
context carried from window to window, zeros for a sequence's first).  The CPU truth the GPU kernels are checked against: padding,
stride and gate order are torch's own, not the library's."""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

WINDOW, CONTEXT = 512, 64


def windows(x: np.ndarray) -> np.ndarray:
    """[ceil(n / 512)][576] model inputs of one sequence: context + zero-padded chunk (what silero's model(chunk, 16000) sees)."""
    x = np.asarray(x, np.float64).reshape(-1)
    nw = -(-x.size // WINDOW)
    padded = np.zeros(CONTEXT + nw * WINDOW)
    padded[CONTEXT:CONTEXT + x.size] = x
    idx = np.arange(nw)[:, None] * WINDOW + np.arange(CONTEXT + WINDOW)[None, :]
    return padded[idx]


def as_float(pcm: np.ndarray) -> np.ndarray:
    """int16 -> x / 32768; float -> / max|x| when that exceeds 1 (backend/vad.py:24-38)"""
    if pcm.dtype == np.int16:
        return pcm.astype(np.float64) / 32768.0
    x = pcm.astype(np.float32)
    peak = np.abs(x).max() if x.size else 0.0
    return (x / peak if peak > 1.0 else x).astype(np.float64)


class TorchVAD(nn.Module):
    def __init__(self, w: Dict[str, np.ndarray]):
        super().__init__()
        t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
        self.pad = nn.ReflectionPad1d((0, 64))
        self.register_buffer("basis", t(w["stft.forward_basis_buffer"]))
        self.enc = nn.ModuleList()
        for i, (ci, co, s) in enumerate([(129, 128, 1), (128, 64, 2), (64, 64, 2), (64, 128, 1)]):
            c = nn.Conv1d(ci, co, 3, stride=s, padding=1).double()
            c.weight.data, c.bias.data = t(w[f"encoder.{i}.reparam_conv.weight"]), t(w[f"encoder.{i}.reparam_conv.bias"])
            self.enc.append(c)
        self.cell = nn.LSTMCell(128, 128).double()
        for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            getattr(self.cell, n).data = t(w[f"decoder.rnn.{n}"])
        self.head = nn.Conv1d(128, 1, 1).double()
        self.head.weight.data, self.head.bias.data = t(w["decoder.decoder.2.weight"]), t(w["decoder.decoder.2.bias"])

    @torch.no_grad()
    def features(self, win: np.ndarray) -> torch.Tensor:
        """[N][576] model inputs -> [N][128] LSTM inputs (everything that does not depend on the recurrence)"""
        x = self.pad(torch.tensor(win, dtype=torch.float64)[:, None, :])           # [N][1][640]
        s = F.conv1d(x, self.basis, stride=128)                                     # [N][258][4]
        x = torch.sqrt(s[:, :129] ** 2 + s[:, 129:] ** 2)
        for c in self.enc:
            x = F.relu(c(x))
        return x[:, :, 0]

    @torch.no_grad()
    def probs_batch(self, seqs: Sequence[np.ndarray]) -> List[np.ndarray]:
        """per-window probabilities of each sequence (int16 or float PCM); the state is reset per sequence"""
        xs = [as_float(np.asarray(s).reshape(-1)) for s in seqs]
        wins = [windows(x) for x in xs]
        nw = [len(w) for w in wins]
        if sum(nw) == 0:
            return [np.zeros(0) for _ in seqs]
        feats = self.features(np.concatenate(wins)).split(nw)
        T = max(nw)
        h = torch.zeros(len(seqs), 128, dtype=torch.float64)
        c = torch.zeros_like(h)
        out = torch.zeros(len(seqs), T, dtype=torch.float64)
        inp = torch.zeros(T, len(seqs), 128, dtype=torch.float64)
        for b, f in enumerate(feats):
            inp[:len(f), b] = f
        for t in range(T):
            h, c = self.cell(inp[t], (h, c))
            out[:, t] = torch.sigmoid(self.head(F.relu(h)[:, :, None]))[:, 0, 0]
        return [out[b, :nw[b]].numpy() for b in range(len(seqs))]

    def probs(self, pcm: np.ndarray) -> np.ndarray:
        return self.probs_batch([pcm])[0]
