"""The part of a checkpoint's generation_config.json that changes what greedy decoding emits.

The reference decodes with `model.generate(**inputs, max_new_tokens=..., do_sample=False)`: generate() merges the checkpoint's generation_config.json
into the call and builds a LogitsProcessorList from it (GenerationMixin._get_logits_processor).  Three of those processors run inside the engine's
greedy kernel (sonic_set_generation): repetition_penalty, no_repeat_ngram_size, suppress_tokens.  Every other field that would change
the tokens of a do_sample=False run is refused by name - a silently different transcript is what this module exists to prevent - and the fields
that only matter when sampling are ignored, as do_sample=False ignores them.

`GenerationGuards.apply` restates the three processors in numpy, bit for bit (tests/test_generation_guards_host.py holds it against HF's own classes);
it is the reference of the GPU tests.
"""
from __future__ import annotations

import json
import math
import os
from typing import Any, Dict, Iterable, List, Optional, Sequence

import numpy as np

MAX_SUPPRESS = 256      # the library's cap (sonic_set_generation)
MAX_NGRAM = 64

# field -> does this value switch something on that the engine does not implement
_REFUSED = {
    "num_beams": lambda v: v is not None and int(v) > 1,
    "num_beam_groups": lambda v: v is not None and int(v) > 1,
    "bad_words_ids": lambda v: bool(v),
    "min_new_tokens": lambda v: v is not None and int(v) > 0,
    "min_length": lambda v: v is not None and int(v) > 0,
    "begin_suppress_tokens": lambda v: bool(v),
    "sequence_bias": lambda v: bool(v),
    "forced_bos_token_id": lambda v: v is not None,
    "forced_eos_token_id": lambda v: v is not None,
    "forced_decoder_ids": lambda v: bool(v),
    "encoder_repetition_penalty": lambda v: v is not None and float(v) != 1.0,
    "encoder_no_repeat_ngram_size": lambda v: v is not None and int(v) > 0,
    "penalty_alpha": lambda v: v is not None and float(v) != 0.0,
    "exponential_decay_length_penalty": lambda v: bool(v),
    "guidance_scale": lambda v: v is not None and float(v) != 1.0,
    "stop_strings": lambda v: bool(v),                 # ends a greedy run earlier than EOS / max_new_tokens would
    "watermarking_config": lambda v: bool(v),          # biases the scores ahead of the argmax
    # constrained generation: a config cannot carry a callable or an automaton; the engine's own form is a grammar per request (_HINTS)
    "prefix_allowed_tokens_fn": lambda v: v is not None,
    "force_words_ids": lambda v: bool(v),
    "constraints": lambda v: bool(v),
}
_HINTS = {name: " (to restrict transcripts to a closed set, build the model with grammar=True and pass ASRModel.compile_grammar(...) as grammar= of the call)"
          for name in ("prefix_allowed_tokens_fn", "force_words_ids", "constraints")}
# Known and let through, because a greedy run emits the same ids with and without them: renormalize_logits (log_softmax keeps the argmax; it would only
# shift the scores HF reports) and remove_invalid_values (it rewrites nan / +-inf scores, which finite weights do not produce).  INTEGRATION.md says so.


class GenerationGuards:
    """repetition_penalty p (1.0: none), no_repeat_ngram_size n (0: none), suppress_tokens (empty: none)"""
    __slots__ = ("repetition_penalty", "no_repeat_ngram_size", "suppress_tokens")

    def __init__(self, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None, suppress_tokens: Optional[Iterable[int]] = None):
        p = 1.0 if repetition_penalty is None else float(repetition_penalty)
        n = 0 if no_repeat_ngram_size is None else int(no_repeat_ngram_size)
        sup = [] if suppress_tokens is None else [int(t) for t in suppress_tokens]
        if not (p > 0 and math.isfinite(p)):
            raise ValueError(f"repetition_penalty must be a finite value > 0, got {repetition_penalty!r}")
        if not 0 <= n <= MAX_NGRAM:
            raise ValueError(f"no_repeat_ngram_size must be within 0 .. {MAX_NGRAM}, got {no_repeat_ngram_size!r}")
        if len(sup) > MAX_SUPPRESS or any(t < 0 for t in sup):
            raise ValueError(f"suppress_tokens: at most {MAX_SUPPRESS} non-negative ids, got {len(sup)}")
        self.repetition_penalty, self.no_repeat_ngram_size, self.suppress_tokens = p, n, sup

    @property
    def active(self) -> bool:
        return float(np.float32(self.repetition_penalty)) != 1.0 or self.no_repeat_ngram_size > 0 or bool(self.suppress_tokens)

    def as_dict(self) -> Dict[str, Any]:
        return {"repetition_penalty": self.repetition_penalty, "no_repeat_ngram_size": self.no_repeat_ngram_size, "suppress_tokens": list(self.suppress_tokens)}

    def override(self, repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                 suppress_tokens: Optional[Iterable[int]] = None) -> "GenerationGuards":
        """a value given here replaces this object's; None keeps it"""
        return GenerationGuards(self.repetition_penalty if repetition_penalty is None else repetition_penalty,
                                self.no_repeat_ngram_size if no_repeat_ngram_size is None else no_repeat_ngram_size,
                                self.suppress_tokens if suppress_tokens is None else suppress_tokens)

    def __repr__(self):
        return f"GenerationGuards(repetition_penalty={self.repetition_penalty}, no_repeat_ngram_size={self.no_repeat_ngram_size}, suppress_tokens={self.suppress_tokens})"

    def __eq__(self, other):
        return isinstance(other, GenerationGuards) and self.as_dict() == other.as_dict()

    def banned_ngram_tokens(self, history: Sequence[int]) -> List[int]:
        """ids that followed an earlier occurrence of the history's last n - 1 ids (HF _calc_banned_ngram_tokens); nothing while len + 1 < n"""
        n, h = self.no_repeat_ngram_size, [int(t) for t in history]
        if n <= 0 or len(h) + 1 < n:
            return []
        last = h[len(h) - (n - 1):] if n > 1 else []
        return [h[j + n - 1] for j in range(len(h) - n + 1) if h[j:j + n - 1] == last]

    def apply(self, scores_f32, history: Sequence[int]) -> np.ndarray:
        """One row: the processed fp32 scores [V] of raw fp32 scores and the row's input_ids (prompt ids, then every emitted id).  The penalty is
        rounded to fp32 once; s * p and s / p are fp32 operations (numpy's float32 divide is correctly rounded); then the bans, -inf."""
        s = np.array(scores_f32, dtype=np.float32, copy=True)
        assert s.ndim == 1
        h = np.asarray(list(history), dtype=np.int64)
        p = np.float32(self.repetition_penalty)
        if p != np.float32(1.0) and h.size:
            ids = np.unique(h)
            v = s[ids]
            with np.errstate(over="ignore", invalid="ignore"):
                s[ids] = np.where(v < 0, v * p, v / p)
        banned = self.banned_ngram_tokens(h.tolist()) + list(self.suppress_tokens)
        if banned:
            s[np.asarray(banned, dtype=np.int64)] = -np.inf
        return s


def from_dict(cfg: Dict[str, Any]) -> GenerationGuards:
    """the guards of a generation config given as a dict; ValueError naming the first field the engine would have to ignore"""
    for name, on in _REFUSED.items():
        if name in cfg and on(cfg[name]):
            raise ValueError(f"generation_config.json sets {name}={cfg[name]!r}: generate(do_sample=False) would honour it, this engine does not implement it" + _HINTS.get(name, ""))
    return GenerationGuards(cfg.get("repetition_penalty"), cfg.get("no_repeat_ngram_size"), cfg.get("suppress_tokens"))


def load(checkpoint_dir: str) -> GenerationGuards:
    """generation_config.json of a checkpoint directory; a missing file means no guards"""
    path = os.path.join(str(checkpoint_dir), "generation_config.json")
    if not os.path.isfile(path):
        return GenerationGuards()
    with open(path, "r", encoding="utf-8") as f:
        cfg = json.load(f)
    if not isinstance(cfg, dict):
        raise ValueError(f"{path} does not hold a JSON object")
    return from_dict(cfg)
