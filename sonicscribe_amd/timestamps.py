"""Host side of word timestamps (ASRModel.align / transcribe(word_timestamps=True)): what the engine's t_n - the index into a request's
audio-token run at which token n starts - becomes in seconds, how token times become start / end pairs, and how tokens are grouped into words.

One audio token is merge x 2 x hop = 1280 samples = 80 ms.  A request of several 30 s windows carries its windows' kept rows one after the other in ONE run of
placeholders, so index i of the run lies in window w at offset i - (rows of the windows before w): w * chunk_seconds + offset * 0.08 s.

Word grouping is a policy of this package (openai-whisper's split_tokens_on_unicode / split_tokens_on_spaces, restated); the kernels' contract ends at t_n.

This file is host logic only (no GPU, no library).
"""
from __future__ import annotations

import json
import math
import os
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

AUDIO_TOKEN_SECONDS = 0.08      # merge (4) x conv stride (2) x hop (160) samples at 16 kHz


def check_timestamps(timestamps: bool, scoring: bool, alignment_heads, dec_layers: Optional[int] = None, dec_heads: Optional[int] = None) -> Optional[List[Tuple[int, int]]]:
    """ASRModel's timestamps / alignment_heads arguments -> the head list (None: the default), or ValueError by name - before any device work."""
    if alignment_heads is not None and not timestamps:
        raise ValueError("alignment_heads needs timestamps=True (ASRModel(..., token_logprobs=True, scoring=True, timestamps=True))")
    if timestamps and not scoring:
        raise ValueError("timestamps=True needs scoring=True: the alignment rides on the scoring handle's parallel forced run "
                         "(ASRModel(..., token_logprobs=True, scoring=True, timestamps=True))")
    if alignment_heads is None:
        return None
    heads: List[Tuple[int, int]] = []
    for i, lh in enumerate(alignment_heads):
        try:
            l, h = (int(x) for x in lh)
        except (TypeError, ValueError):
            raise ValueError(f"alignment_heads[{i}] = {lh!r} is not a [layer, head] pair") from None
        if l < 0 or h < 0 or h > 255 or (dec_layers is not None and l >= dec_layers) or (dec_heads is not None and h >= dec_heads):
            raise ValueError(f"alignment_heads[{i}] = [{l}, {h}] is outside the decoder ({dec_layers} layers x {dec_heads} heads)")
        if (l, h) not in heads:
            heads.append((l, h))
    if not heads:
        raise ValueError("alignment_heads is empty (None selects the default: every head of the last half of the decoder layers)")
    if len(heads) > 256:
        raise ValueError(f"alignment_heads holds {len(heads)} heads, the engine takes 256")
    return heads


def load_alignment_heads(checkpoint_dir: str):
    """the `alignment_heads` entry of the checkpoint's generation_config.json (Whisper's format: a list of [layer, head]), or None"""
    path = os.path.join(str(checkpoint_dir), "generation_config.json")
    if not os.path.isfile(path):
        return None
    with open(path, "r", encoding="utf-8") as f:
        return json.load(f).get("alignment_heads")


def audio_index_seconds(idx, per_window_rows: Sequence[int], n_placeholders: int, chunk_seconds: float = 30.0, step: float = AUDIO_TOKEN_SECONDS) -> np.ndarray:
    """Index into a request's audio-token run -> seconds from the start of its audio.  per_window_rows: frontend.request_audio_tokens' per-window counts;
    n_placeholders: the run's length.  Where the two agree (every request the engine accepts: it refuses a prompt whose placeholder count differs from the rows it
    keeps), index i of window w maps to w * chunk_seconds + (i - rows before w) * step.  Where they differ - a processor that counts placeholders from the summed
    frames - there is no per-window offset to trust, and the rule is the run's own: i * step."""
    idx = np.asarray(idx, np.int64)
    rows = [int(r) for r in per_window_rows]
    if sum(rows) != int(n_placeholders):
        return idx.astype(np.float64) * step
    first = np.concatenate([[0], np.cumsum(rows)])                       # first run index of every window
    w = np.clip(np.searchsorted(first, idx, side="right") - 1, 0, max(0, len(rows) - 1))
    return w.astype(np.float64) * float(chunk_seconds) + (idx - first[w]).astype(np.float64) * step


def token_spans(starts: Sequence[float], duration: float) -> Tuple[np.ndarray, np.ndarray]:
    """start times of consecutive tokens -> (start, end): end_n = start_{n+1}, the last token ends with the audio.  Starts are clipped to [0, duration]."""
    s = np.clip(np.asarray(starts, np.float64), 0.0, float(duration))
    e = np.concatenate([s[1:], [float(duration)]]) if s.size else s.copy()
    return s, e


_WORD_SCRIPTS = ((0x0E00, 0x0E7F),                                     # Thai
                 (0x1100, 0x11FF), (0x3130, 0x318F), (0xAC00, 0xD7AF),  # hangul
                 (0x3040, 0x30FF), (0x31F0, 0x31FF),                    # kana
                 (0x2E80, 0x2FDF), (0x3400, 0x4DBF), (0x4E00, 0x9FFF), (0xF900, 0xFAFF), (0x20000, 0x2FA1F))   # CJK


def is_unspaced_script(text: str) -> bool:
    """does the piece hold a CJK, kana, hangul or Thai character (scripts written without spaces: every such piece is a word of its own)"""
    return any(lo <= ord(c) <= hi for c in text for lo, hi in _WORD_SCRIPTS)


def split_pieces(token_ids: Sequence[int], decode: Callable[[List[int]], str]) -> List[Tuple[str, List[int]]]:
    """Whisper's split_tokens_on_unicode: tokens -> (text, token positions) pieces; tokens whose bytes do not yet decode to valid text (the decoder's U+FFFD)
    merge forward into the piece that completes them.  A trailing incomplete rest is one last piece."""
    out: List[Tuple[str, List[int]]] = []
    cur: List[int] = []
    for i, t in enumerate(token_ids):
        cur.append(i)
        text = decode([int(token_ids[j]) for j in cur])
        if "\ufffd" not in text:
            out.append((text, cur))
            cur = []
    if cur:
        out.append((decode([int(token_ids[j]) for j in cur]), cur))
    return out


def group_words(pieces: Sequence[Tuple[str, Sequence[int]]]) -> List[Tuple[str, List[int]]]:
    """Whisper's split_tokens_on_spaces over pieces: a word starts at a piece that begins with whitespace (and at the first piece); a piece holding a CJK, kana,
    hangul or Thai character is a word of its own, and so is what follows it.  Returns (word text, token positions) in order; the words partition the tokens."""
    words: List[Tuple[str, List[int]]] = []
    alone = False                   # the last word is an unspaced-script piece: nothing joins it
    for text, pos in pieces:
        own = is_unspaced_script(text)
        if not words or own or alone or text[:1].isspace():
            words.append((text, list(pos)))
        else:
            words[-1] = (words[-1][0] + text, words[-1][1] + list(pos))
        alone = own
    return words


class Word:
    """One word of an Alignment: its text (stripped), start / end in seconds, `probability` = exp(mean log-probability of its tokens), its token positions."""
    __slots__ = ("word", "start", "end", "probability", "tokens")

    def __init__(self, word: str, start: float, end: float, probability: float, tokens: Sequence[int]):
        self.word, self.start, self.end, self.probability, self.tokens = word, float(start), float(end), float(probability), [int(t) for t in tokens]

    def as_dict(self) -> dict:
        return {"word": self.word, "start": self.start, "end": self.end, "probability": self.probability}

    def __repr__(self):
        return f"Word({self.word!r}, {self.start:.2f}-{self.end:.2f}, p={self.probability:.3f})"


class Alignment:
    """When a transcript's tokens were spoken: `token_ids` (EOS dropped), `token_start` / `token_end` [n] float64 seconds from the start of the audio,
    `token_logprobs` [n] float32 and `words` (Word).  `audio_index` [n]: the engine's t_n."""
    __slots__ = ("token_ids", "token_start", "token_end", "token_logprobs", "audio_index", "words")

    def __init__(self, token_ids, token_start, token_end, token_logprobs, audio_index, words: List[Word]):
        self.token_ids = np.asarray(token_ids, np.int32)
        self.token_start, self.token_end = np.asarray(token_start, np.float64), np.asarray(token_end, np.float64)
        self.token_logprobs, self.audio_index, self.words = np.asarray(token_logprobs, np.float32), np.asarray(audio_index, np.int32), list(words)

    def shifted(self, offset: float) -> "Alignment":
        """the same alignment on a clock that starts `offset` seconds earlier (a file segment's start)"""
        o = float(offset)
        return Alignment(self.token_ids, self.token_start + o, self.token_end + o, self.token_logprobs, self.audio_index,
                         [Word(w.word, w.start + o, w.end + o, w.probability, w.tokens) for w in self.words])

    def __repr__(self):
        return f"Alignment(tokens={self.token_ids.size}, words={len(self.words)})"


def build_alignment(token_ids, token_logprobs, audio_index, eos_ids: Sequence[int], per_window_rows: Sequence[int], n_placeholders: int, duration: float,
                    pieces_of: Callable[[Sequence[int]], List[Tuple[str, List[int]]]], chunk_seconds: float = 30.0) -> Alignment:
    """One scored sequence -> its Alignment.  The EOS token is dropped from the output (its row took part in the normalisation over tokens, as in Whisper)."""
    ids = [int(t) for t in np.asarray(token_ids).reshape(-1)]
    eos = set(int(e) for e in eos_ids)
    n = len(ids) - 1 if ids and ids[-1] in eos else len(ids)
    ids = ids[:n]
    lp = np.asarray(token_logprobs, np.float32).reshape(-1)[:n]
    idx = np.asarray(audio_index, np.int32).reshape(-1)[:n]
    start, end = token_spans(audio_index_seconds(idx, per_window_rows, n_placeholders, chunk_seconds), duration)
    words = []
    for text, pos in group_words(pieces_of(ids)):
        mean = float(np.mean(lp[pos], dtype=np.float64)) if len(pos) else float("nan")
        words.append(Word(text.strip(), start[pos[0]], end[pos[-1]], math.exp(mean) if mean == mean else float("nan"), pos))
    return Alignment(ids, start, end, lp, idx, words)
