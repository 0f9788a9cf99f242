"""Per-request sequence bias: HF's SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor (generation/logits_process.py) on a table that belongs to one
request - the reference's per-connection / per-upload `hotwords` (backend/asr.py:303-333) as shallow biasing of the scores, beside the sentence in the prompt.

The contract (include/sonic_hip.h at sonic_set_request_bias).  A table is a list of entries, each a token sequence of 1 .. 8 ids and an fp32
bias, de-duplicated as HF's list-to-dict conversion does (the last bias of equal sequences wins, at the first position).  With input_ids = the prompt ids
(audio placeholders included) followed by every emitted id, a per-token fp32 sum starts at +0.0, takes the length-1 entry of that token, then - in list order -
every longer entry that ends on the token, has L <= len(input_ids) (HF skips L == len + 1 although its prefix would fit) and whose first L - 1 ids are the last
L - 1 ids of input_ids.  score = score + sum, once, in fp32, ahead of GenerationGuards (HF's _get_logits_processor order: the penalty sees the biased score).

bad_words_ids are the same entries with bias -inf, minus every sequence equal to [eos] (NoBadWords' own filter).  HF applies them behind the n-gram guard; folded
into the one table they give the same bits, because sequence_bias values must be finite: (s + b) -> penalty -> -inf and s + (b + -inf) -> penalty are both -inf
for p > 0, and -inf stays -inf under every later processor.

`RequestBias.apply` restates the arithmetic in numpy, bit for bit (tests/test_request_bias_host.py holds it against HF's own classes); the full chain of one row is
`guards.apply(bias.apply(scores, history), history)`.  It is the reference of the GPU tests.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .frontend import clean_hotwords

MAX_ENTRIES = 256       # the library's caps (sonic_set_request_bias): entries per request, ids per entry.  Nothing is ever truncated
MAX_LEN = 8


def _entries_of(sequence_bias) -> List[Tuple[Tuple[int, ...], float]]:
    """HF's two accepted forms, {tuple of ids: bias} and [[ids, bias], ...], as a list in iteration order"""
    if sequence_bias is None:
        return []
    if isinstance(sequence_bias, dict):
        items = list(sequence_bias.items())
    else:
        items = []
        for ent in sequence_bias:
            if not isinstance(ent, (list, tuple)) or len(ent) != 2:
                raise ValueError(f"sequence_bias: every element is [ids, bias], got {ent!r}")
            items.append((ent[0], ent[1]))
    out = []
    for ids, b in items:
        if isinstance(ids, (str, bytes)) or not isinstance(ids, (list, tuple, np.ndarray)):
            raise ValueError(f"sequence_bias: a token sequence is a list or tuple of ids, got {ids!r}")
        out.append((_ids_of(ids, "sequence_bias"), b))
    return out


def _ids_of(ids, what: str) -> Tuple[int, ...]:
    seq = list(ids)
    if not seq:
        raise ValueError(f"{what}: an empty token sequence")
    for t in seq:
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or int(t) < 0:
            raise ValueError(f"{what}: token ids are non-negative integers, got {t!r}")
    return tuple(int(t) for t in seq)


class RequestBias:
    """One request's table: `sequence_bias` entries (finite biases) in their order, then `bad_words_ids` (bias -inf; sequences equal to [eos] for one of
    `eos_ids` dropped), de-duplicated as one dict.  ValueError for a non-finite sequence_bias value, more than 256 entries, more than 8 ids in an entry,
    and - where `vocab` is known - an id outside the vocabulary."""
    __slots__ = ("entries",)

    def __init__(self, sequence_bias=None, bad_words_ids=None, eos_ids: Iterable[int] = (), *, vocab: Optional[int] = None):
        table: Dict[Tuple[int, ...], np.float32] = {}
        for ids, b in _entries_of(sequence_bias):
            with np.errstate(over="ignore"):
                b32 = np.float32(b) if isinstance(b, (int, float, np.floating, np.integer)) and not isinstance(b, bool) else None
            if b32 is None or not math.isfinite(float(b)) or not math.isfinite(float(b32)):
                raise ValueError(f"sequence_bias: the bias of {list(ids)} must be a finite fp32 value, got {b!r} (a forbidden sequence belongs in bad_words_ids)")
            table[ids] = b32                             # dict semantics: the last value wins, the first position stays
        eos = [int(t) for t in eos_ids]
        if bad_words_ids is not None:
            if isinstance(bad_words_ids, (str, bytes)) or not isinstance(bad_words_ids, (list, tuple)):
                raise ValueError(f"bad_words_ids is a list of token sequences, got {bad_words_ids!r}")
            for seq in bad_words_ids:
                if isinstance(seq, (str, bytes)) or not isinstance(seq, (list, tuple, np.ndarray)):
                    raise ValueError(f"bad_words_ids is a list of token sequences, got {seq!r}")
                ids = _ids_of(seq, "bad_words_ids")
                if len(ids) == 1 and ids[0] in eos:      # NoBadWordsLogitsProcessor: a bad word equal to [eos] is dropped
                    continue
                table[ids] = np.float32(-np.inf)
        for ids in table:
            if len(ids) > MAX_LEN:
                raise ValueError(f"request bias: the sequence {list(ids)} has {len(ids)} ids, at most {MAX_LEN} (entries are never truncated)")
        if len(table) > MAX_ENTRIES:
            raise ValueError(f"request bias: {len(table)} entries, at most {MAX_ENTRIES} per request (entries are never truncated)")
        self.entries: List[Tuple[Tuple[int, ...], np.float32]] = list(table.items())
        if vocab is not None:
            self.check_vocab(vocab)

    def check_vocab(self, vocab: int) -> None:
        for ids, _ in self.entries:
            for t in ids:
                if t >= int(vocab):
                    raise ValueError(f"request bias: token id {t} is outside the vocabulary ({int(vocab)})")

    def __len__(self) -> int:
        return len(self.entries)

    def __bool__(self) -> bool:
        return bool(self.entries)

    def __eq__(self, other):
        return isinstance(other, RequestBias) and [(i, np.float32(b).tobytes()) for i, b in self.entries] == [(i, np.float32(b).tobytes()) for i, b in other.entries]

    def __repr__(self):
        return f"RequestBias({[[list(i), float(b)] for i, b in self.entries]!r})"

    def table(self):
        """(seq_ids int32 [sum L], seq_off int32 [n + 1], bias fp32 [n]): the packed arrays the library takes, in list order (the library groups them)"""
        ids = np.asarray([t for seq, _ in self.entries for t in seq], dtype=np.int32)
        off = np.zeros(len(self.entries) + 1, np.int32)
        if self.entries:
            off[1:] = np.cumsum([len(seq) for seq, _ in self.entries])
        return ids, off, np.asarray([b for _, b in self.entries], dtype=np.float32)

    def bias_vector(self, vocab: int, history: Sequence[int]) -> np.ndarray:
        """the fp32 sum per token [V] for this history, accumulated in the contract's order"""
        self.check_vocab(vocab)
        h = [int(t) for t in history]
        acc = np.zeros(int(vocab), np.float32)
        for ids, b in self.entries:                      # the length-1 values first (unique per token after the de-duplication)
            if len(ids) == 1:
                acc[ids[0]] = np.float32(0.0) + b
        with np.errstate(invalid="ignore"):
            for ids, b in self.entries:                  # then every longer entry, in list order
                L = len(ids)
                if L == 1 or L > len(h):
                    continue
                if h[len(h) - (L - 1):] == list(ids[:-1]):
                    acc[ids[-1]] = acc[ids[-1]] + b
        return acc

    def apply(self, scores_f32, history: Sequence[int]) -> np.ndarray:
        """One row: raw fp32 scores [V] and the row's input_ids -> scores + bias, one fp32 addition per token (HF adds the whole vector, +0.0 included)"""
        s = np.array(scores_f32, dtype=np.float32, copy=True)
        assert s.ndim == 1
        with np.errstate(invalid="ignore"):
            return (s + self.bias_vector(s.shape[0], history)).astype(np.float32)


def combine(*tables: Optional["RequestBias"]) -> "RequestBias":
    """tables concatenated as lists in the given order, then de-duplicated as one dict (ASRModel: constructor sequence_bias, constructor bad words, the call's
    values, the hotword entries)"""
    out = RequestBias()
    merged: Dict[Tuple[int, ...], np.float32] = {}
    for t in tables:
        if t is None:
            continue
        for ids, b in t.entries:
            merged[ids] = b
    if len(merged) > MAX_ENTRIES:
        raise ValueError(f"request bias: {len(merged)} entries after combining, at most {MAX_ENTRIES} per request (entries are never truncated)")
    out.entries = list(merged.items())
    return out


def hotword_entries(hotwords: Optional[Sequence[str]], boost: float, encode) -> List[List[Any]]:
    """The hotword policy (README; the kernel contract does not depend on it): the hotwords are cleaned exactly as the prompt sentence cleans them
    (frontend.clean_hotwords); each is tokenised as it stands and with one leading space, duplicates dropped; every prefix of length 1 .. min(n, 8) of either
    tokenisation gets bias `boost` - HF's own advice for greedy runs ("apply the bias to their prefixes").  `encode(text) -> ids` adds no special tokens.
    Returns [[ids, boost], ...] in that order; [] for boost == 0 or no hotwords."""
    b = float(boost)
    if not math.isfinite(b) or b < 0:
        raise ValueError(f"hotword_boost must be a finite value >= 0, got {boost!r}")
    if b == 0.0:
        return []
    seen, out = set(), []
    for hw in clean_hotwords(hotwords):
        toks = []
        for text in (hw, " " + hw):
            ids = tuple(int(t) for t in encode(text))
            if ids and ids not in toks:
                toks.append(ids)
        for ids in toks:
            for n in range(1, min(len(ids), MAX_LEN) + 1):
                if ids[:n] not in seen:
                    seen.add(ids[:n])
                    out.append([list(ids[:n]), b])
    return out
