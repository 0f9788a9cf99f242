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
import json
import math
import os
import threading
import time
from concurrent.futures import Future
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np

from . import fallback, frontend, genconfig, grammar as grammar_, ngram as ngram_, reqbias, reqvalues, sampling as sampling_, scoring as scoring_, timestamps as timestamps_, weights
from .dispatch import Dispatcher
from .engine import Engine, MODE_INT8, MODE_NATIVE, SonicError, TokenScores, device_count, device_info
from .prompts import HFPrompt, SyntheticPrompt
from .reqvalues import CallKeywords, CallValues
from .sampling import NO_CUT, CallSampling
from .scoring import Score
from .spec import FULL, ModelDims
from .stream import AudioStream
from .transcription import Transcription, _only_text, _text_future, cut_draft, draft_matched, stamp, then


# Batches in flight per replica on ONE weight copy (engine slots, include/sonic_hip.h sonic_slot_create).  The reference's file mode keeps up to
# three decodes in flight on its one model object (backend/main.py:429-445); here they overlap on the device instead of serialising.
DEFAULT_SLOTS = 2
# Row-level scheduling (dispatch._ContinuousReplica): the replica's engine decodes forever over its rows, the slot prefills; requests join and
# leave row by row.  False: batch by batch (dispatch._Replica), every slot runs whole batches.
DEFAULT_CONTINUOUS = True


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


# The constructor's refusals of a feature without what it needs: (feature, does the model `m` break the rule, the text).  ASRModel.__init__ walks them feature by
# feature, top to bottom, each feature behind the check of its own values - so, for a call that breaks two rules, in this order: mode, top_logprobs
# (check_top_logprobs: range, token_logprobs, bulk), the values of temperature / seed / thresholds, "temperature", the values of top_k / top_p / min_p, "truncation",
# "sampling", best_of (check_best_of: range, sampling, bulk), "grammar", "draft_verify", "scoring", score_share_prompt (check_share_prompt), timestamps (timestamps.check_timestamps), the device - all ahead
# of any engine.  "request_bias" alone comes behind the loading: the defaults that switch it on are checked against the checkpoint's vocabulary.
_NEEDS_SAMPLING = " need a model built with sampling=True (ASRModel(..., token_logprobs=True, sampling=True))"
# (the two models whose scoring handles cannot share a prompt, DESIGN.md 6.14: the constructor and score(..., share_prompt=True) say the same)
_SHARE_INT8 = "share_prompt is not supported with mode='int8': its prefill finds outlier columns per sequence, and a shared prompt belongs to several"
_SHARE_ALIGN = "share_prompt is not supported on a model built with timestamps=True: its scoring handles align, and the alignment reads a sequence's audio keys from its own rows"
_REFUSALS = (
    ("temperature", lambda m: not m.sampling and (any(t != 0.0 for t in sampling_.temperatures(m._default_temperature)[0]) or m._default_seed != 0), "temperature / seed" + _NEEDS_SAMPLING),
    ("truncation", lambda m: not m.sampling and m._default_cut != NO_CUT, "top_k / top_p / min_p" + _NEEDS_SAMPLING),
    ("sampling", lambda m: m.sampling and not m.token_logprobs, "sampling=True needs token_logprobs=True: the sampling kernels are log-probability kernels, and the fallback ladder reads avg_logprob"),
    ("sampling", lambda m: m.sampling and m.bulk, "sampling is not supported with bulk=True: the bulk pipeline carries no per-request values"),
    ("grammar", lambda m: m.grammar and not m.token_logprobs, "grammar=True needs token_logprobs=True: the grammar kernels are log-probability kernels (ASRModel(..., token_logprobs=True, grammar=True))"),
    ("grammar", lambda m: m.grammar and m.bulk, "grammar is not supported with bulk=True: the bulk pipeline carries no per-request grammar state"),
    ("draft_verify", lambda m: m.draft_verify and m.mode == "int8", "draft_verify is not supported with mode='int8': its prefill quantises per request group, so a draft would change the prompt's own values"),
    ("draft_verify", lambda m: m.draft_verify and m.bulk, "draft_verify is not supported with bulk=True: the bulk pipeline verifies no drafts"),
    ("scoring", lambda m: m.scoring and not m.token_logprobs, "scoring=True needs token_logprobs=True: a score is the candidates' token log-probabilities (ASRModel(..., token_logprobs=True, scoring=True))"),
    ("request_bias", lambda m: m.request_bias and m.bulk, "request_bias is not supported with bulk=True: the bulk pipeline carries no per-request tables"),
)


def check_lm(lm, lm_weight, token_logprobs: bool, bulk: bool, grammar: bool, draft_verify: bool, best_of: int) -> float:
    """ASRModel's lm / lm_weight arguments -> the fp32 weight, or ValueError by name: a weight that is not finite and >= 0; lm= without token_logprobs=True, or beside
    bulk=True, grammar=True, draft_verify=True or best_of > 1 (the library's own refusals, DESIGN.md 6.15, ahead of any engine)"""
    w = ngram_.check_weight(lm_weight)
    if lm is None:
        return w
    if not isinstance(lm, (ngram_.NGramLM, str, os.PathLike)):
        raise ValueError("lm= takes an ngram.NGramLM or the path of an ARPA file")
    if not token_logprobs:
        raise ValueError("lm= needs token_logprobs=True: the language model's kernels are log-probability kernels (ASRModel(..., token_logprobs=True, lm=...))")
    if bulk:
        raise ValueError("lm is not supported with bulk=True: the bulk pipeline carries no language-model state")
    if grammar:
        raise ValueError("lm is not supported with grammar=True: a grammar decides and a language model weighs - the kernels hold one of the two")
    if draft_verify:
        raise ValueError("lm is not supported with draft_verify=True: the verify pass knows no language model")
    if int(best_of) > 1:
        raise ValueError("lm is not supported with best_of > 1: a row fork copies no language-model state")
    return w


def check_share_prompt(share, scoring: bool, mode: str, timestamps: bool) -> bool:
    """score_share_prompt as ASRModel takes it: ValueError without scoring=True, with mode="int8" and with timestamps=True"""
    if not share:
        return False
    if not scoring:
        raise ValueError("score_share_prompt=True needs scoring=True: it is the scoring handle's prefill that shares the prompt (ASRModel(..., token_logprobs=True, scoring=True, score_share_prompt=True))")
    if mode == "int8" or timestamps:
        raise ValueError(_SHARE_INT8 if mode == "int8" else _SHARE_ALIGN)
    return True


def check_fp8_checkpoint(checkpoint_dir) -> None:
    """mode="fp8" snaps the checkpoint's OWN bfloat16 values (W' is exact in bfloat16), so the mode asks of its checkpoint, ahead of any device,
    what the other modes find out while loading: ValueError by name when the directory has no config.json, or when that file states a torch_dtype other than
    bfloat16 (a float16 / float32 checkpoint would be rounded to bfloat16 first, and the snapped model would not be the one the caller quantised in their head)"""
    path = os.path.join(str(checkpoint_dir), "config.json")
    if not os.path.isfile(path):
        raise ValueError(f"mode='fp8' needs a bfloat16 checkpoint to snap: {path} not found")
    with open(path, "r", encoding="utf-8") as f:
        cfg = json.load(f)
    stated = [c.get("torch_dtype", c.get("dtype")) for c in (cfg, cfg.get("text_config") or {}) if isinstance(c, dict)]
    wrong = [str(t) for t in stated if t is not None and str(t).replace("torch.", "") != "bfloat16"]
    if wrong:
        raise ValueError(f"mode='fp8' needs a bfloat16 checkpoint to snap: {path} states torch_dtype {wrong[0]}")


def _flatten(windows_per_request):
    """windows per request -> (all windows in a row, req_win: request i owns windows req_win[i] .. req_win[i + 1] - 1), as Engine.transcribe_batch / score_batch take them"""
    segs, req_win = [], [0]
    for w in windows_per_request:
        segs.extend(w)
        req_win.append(len(segs))
    return segs, req_win


# --------------------------------------------------------------------------------------- façade
class ASRModel:
    # the feature flags' "off" values: what a model reads that was never built (the host tests make one with ASRModel.__new__ and set what they need)
    sampling = grammar = draft_verify = request_bias = scoring = score_share_prompt = timestamps = bulk = token_logprobs = continuous = False
    mode = "native"
    top_logprobs, best_of, slots = 0, 1, 1
    lm, lm_weight = None, 0.0

    def __init__(self, checkpoint_dir: str, device: str = "cuda", mode: str = "native",
                 cpu_threads: Optional[int] = None, cpu_interop_threads: Optional[int] = None,
                 *, max_batch: int = 32, max_ctx: int = 1024, slots: int = DEFAULT_SLOTS, continuous: bool = DEFAULT_CONTINUOUS, decoders: int = 1, bulk: bool = False, native_dispatch: Optional[bool] = None, token_logprobs: bool = False, top_logprobs: int = 0,
                 repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None, suppress_tokens: Optional[Sequence[int]] = None,
                 request_bias: bool = False, sequence_bias=None, bad_words_ids=None, hotword_boost: float = 0.0,
                 sampling: bool = False, temperature=0.0, seed: int = 0, top_k: int = 0, top_p: float = 1.0, min_p: float = 0.0, compression_ratio_threshold: Optional[float] = 2.4, logprob_threshold: Optional[float] = -1.0, best_of: int = 1,
                 scoring: bool = False, score_share_prompt: bool = False, timestamps: bool = False, alignment_heads=None, grammar: bool = False, draft_verify: bool = False, lm=None, lm_weight: float = 0.3,
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
        brings, in one prefill pass per run on a handle of their own per replica; off, no such handle exists.  `score_share_prompt` (needs scoring=True; not with
        mode="int8", not with timestamps=True): the candidates of one audio also share ONE prefill of their prompt - the default of the `share_prompt=` of score() / score_batch().  `timestamps` (needs scoring=True): align() and
        word_timestamps=True give the time at which every token and word was spoken, from the decoder's attention onto the audio on that scoring handle;
        `grammar` (needs token_logprobs=True; not with bulk=True): requests may be
        restricted to the transcripts of a grammar - compile_grammar() of a phrase list or of a grammar.Grammar, passed as `grammar=` of the transcribe calls; the mask and
        the state run inside the greedy kernel.  `draft_verify` (not with mode="int8", not with bulk=True): requests may bring a draft of their transcript
        as `draft=` of the transcribe calls - a previous partial, a first-pass model's output, an edited transcript; the prefill accepts the prefix the model itself would
        have emitted and decoding starts behind it, so a right draft costs one prefill instead of its tokens' steps and a wrong one only its prefill rows.  `lm` (needs
        token_logprobs=True; not with bulk=True, grammar=True, draft_verify=True or best_of > 1): shallow fusion - an ngram.NGramLM over the model's own tokens, or the
        path of an ARPA file (ngram.NGramLM.from_arpa over the tokenizer's pieces, or decimal ids), whose log-probabilities times `lm_weight` are added to every step's
        scores inside the decode loops of every entry point; token_logprobs, avg_logprob and the ladder's logprob_threshold are then over the fused scores.  `alignment_heads`: the [layer, head] pairs to read (None: the `alignment_heads` entry of the checkpoint's generation_config.json, else every head of the last half of the layers).  The arguments with a leading underscore are not part of the
        supported surface: they exist for the test-suite and the benchmark and may change without notice.  `_engine_mode` in particular (an engine.MODE_*
        value in place of the one `mode` selects) is unsupported outside the tests: MODE_F32 has no slots, so it needs slots=1, continuous=False."""
        # -- 1. the arguments, in _REFUSALS' order; no device is touched
        if mode not in ["native", "int8", "fp8"]:
            raise ValueError("mode must be either 'native' or 'int8'")            # asr.py:46-47 ("fp8" is this library's third: weight-only e4m3)
        if mode == "fp8" and _engine_mode is not None:
            raise ValueError("mode='fp8' is not supported with _engine_mode: it is a bf16 model (engine.MODE_NATIVE) whose decoder weights are snapped to e4m3")
        if mode == "fp8" and not int((_options or {}).get("fp8_weights", 1)):
            raise ValueError("mode='fp8' is not supported with _options fp8_weights=0: the mode is that option (fp8_chain=0 runs the snapped model on the default chains)")
        if mode == "fp8" and _synthetic_seed is None:
            check_fp8_checkpoint(checkpoint_dir)
        self.mode, self.bulk, self.token_logprobs = mode, bool(bulk), bool(token_logprobs)
        self.sampling, self.grammar, self.draft_verify, self.scoring, self.timestamps = bool(sampling), bool(grammar), bool(draft_verify), bool(scoring), bool(timestamps)
        self.top_logprobs = check_top_logprobs(top_logprobs, token_logprobs, bulk)
        self._default_temperature, self._default_seed = temperature, sampling_.check_seed(seed)
        fallback.FallbackPolicy(sampling_.temperatures(temperature)[0], compression_ratio_threshold, logprob_threshold)      # (validates the values)
        self.compression_ratio_threshold, self.logprob_threshold = compression_ratio_threshold, logprob_threshold
        self._refuse("temperature")
        self._default_cut = sampling_.check_truncation(top_k, top_p, min_p)      # every sampled decode's tail cut: each rung of a ladder above 0, every fork of best_of
        self._refuse("truncation", "sampling")
        self.best_of = check_best_of(best_of, max_batch, self.sampling, bulk)
        self._max_batch = int(max_batch)
        self._refuse("grammar", "draft_verify", "scoring")
        self.lm_weight = check_lm(lm, lm_weight, self.token_logprobs, self.bulk, self.grammar, self.draft_verify, self.best_of)
        self.score_share_prompt = check_share_prompt(score_share_prompt, self.scoring, mode, self.timestamps)
        self._grammars: List[Any] = []      # what compile_grammar() made, closed with the model
        self.alignment_heads = timestamps_.check_timestamps(self.timestamps, self.scoring, alignment_heads, *((_dims.dec_layers, _dims.dec_heads) if _dims is not None else ()))
        dev = str(device)
        if dev.startswith("cpu"):
            raise RuntimeError("sonicscribe_amd runs on MI355X only: DEVICE=cpu has no HIP path (no CPU fallback by design)")
        # -- 2. the engines: one replica per device, the checkpoint's generation values and its prompt
        n_dev = device_count()
        # "cuda" / "cuda:1" = one replica (the reference's surface); "cuda:*" = every visible GPU; "cuda:0,2,3" = those
        spec_ = dev.split(":", 1)[1] if ":" in dev else "0"
        self.device_indices = list(range(n_dev)) if spec_ in ("*", "all") else [int(x) for x in spec_.split(",") if x != ""]
        if not self.device_indices or max(self.device_indices) >= n_dev:
            raise RuntimeError(f"HIP device {spec_} not available ({n_dev} visible)")
        self.device_index = self.device_indices[0]
        self.device = f"cuda:{self.device_index}" if len(self.device_indices) == 1 else "cuda:" + ",".join(map(str, self.device_indices))
        self.model_dtype = "bfloat16" if mode in ("native", "fp8") else "float16"            # asr.py:61
        emode = MODE_NATIVE if mode in ("native", "fp8") else MODE_INT8      # fp8: a bf16 engine whose option fp8_weights is set first, below
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
        file_guards = genconfig.GenerationGuards() if _synthetic_seed is not None else genconfig.load(str(checkpoint_dir))
        self.generation_guards = file_guards.override(repetition_penalty, no_repeat_ngram_size, suppress_tokens)
        self.dims = (_dims or FULL) if _synthetic_seed is not None else weights.load_dims(str(self.checkpoint_dir))
        for di in self.device_indices:
            eng = Engine(self.dims, di, emode, max_batch, max_ctx)
            if _synthetic_seed is not None:
                eng.load_synthetic(_synthetic_seed)
            else:
                weights.load_checkpoint(eng, str(self.checkpoint_dir))
            self.models.append(eng)
        if _synthetic_seed is not None:
            self.prompt = SyntheticPrompt(self.dims)
        else:
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
        # -- 3. the engine options, on every replica before any slot exists (the slots copy them)
        # request_bias: every request may carry a sequence-bias table of its own.  The three value arguments are defaults for every request and switch
        # the option on.  Combined per call as lists - these sequence_bias entries, these bad words, the call's own, then the hotword entries - and de-duplicated as
        # HF de-duplicates one list (reqbias.combine)
        self.hotword_boost = float(hotword_boost or 0.0)
        self._default_bias = reqbias.RequestBias(sequence_bias, bad_words_ids, self._eos_ids(), vocab=self.dims.vocab)
        reqbias.hotword_entries([], self.hotword_boost, None)         # (validates the value)
        self.request_bias = bool(request_bias) or bool(self._default_bias) or self.hotword_boost > 0
        self._refuse("request_bias")
        # In the library's order: the experiment knobs (sonic_set_option); token_logprobs (every greedy step also returns the emitted token's log-probability) and, behind
        # it, top_logprobs; the generation guards; request_bias; sampling with truncation (top_k / top_p / min_p ride on the sampling values; rows that state
        # none take the kernel's branch around the select); grammar; draft_verify.  Only what is on is set: off, nothing changes
        g = self.generation_guards
        options = [(k, int(v)) for k, v in (_options or {}).items()]
        if mode == "fp8":        # first among the options, on every replica before any slot exists: the weights are snapped once, the slots share them
            options = [("fp8_weights", 1)] + [kv for kv in options if kv[0] != "fp8_weights"]
        options.sort(key=lambda kv: kv[0] != "fp8_weights")      # (stable: a caller's fp8_weights goes ahead of its fp8_chain whatever order they came in)
        options += [(k, v) for k, v in (("token_logprobs", int(self.token_logprobs)), ("top_logprobs", self.top_logprobs),
                                        ("generation", (g.repetition_penalty, g.no_repeat_ngram_size, g.suppress_tokens) if g.active else None),
                                        ("request_bias", int(self.request_bias)), ("sampling", int(self.sampling)), ("truncation", int(self.sampling)),
                                        ("grammar", int(self.grammar)), ("draft_verify", int(self.draft_verify))) if v]
        for eng in self.models:
            for k, v in options:
                if k == "generation":
                    eng.set_generation(*v)
                else:
                    eng.set_option(k, v)
        # lm: the automaton onto every replica, the options lm_weight / lm on its owner - every slot made below copies them (a scoring slot ignores them)
        if lm is not None:
            tok = self.prompt.processor.tokenizer if isinstance(self.prompt, HFPrompt) else None
            self.lm = ngram_.load(lm, self.dims.vocab, eos_ids=self._eos_ids(), token_id=None if tok is None else (lambda s, _v=tok.get_vocab(): _v.get(s)))
            for eng in self.models:
                eng.set_lm(eng.lm_create(self.lm), self.lm_weight)
        # -- 4. the handles and the dispatcher
        self._retrier = fallback.Retrier()
        self.model = self.models[0]                  # main.py:84-86 checks and deletes `.model`
        # continuous: `decoders` handles per replica run a greedy loop over max_batch rows each, the other handles prefill (>= 1).  Streaming:
        # decoders=1, slots=2.  Bulk transcription of many segments: max_batch=64, decoders=3, slots=4 (the bench's pipeline shape since round 5; decoders=2, slots=3 before).
        # bulk=True (file mode: deep queues of whole segments): the same handles behind the library's native pipeline (dispatch._BulkReplica ->
        # csrc/pipeline.cpp); implies continuous decode loops.  max_batch=64, decoders=3, slots=4 is the bench's shape.
        self.continuous = bool(continuous) or self.bulk
        self.decoders = max(1, int(decoders)) if self.continuous else 0
        self.slots = max(self.decoders + 1 if self.continuous else 1, int(slots))
        # scoring: one further slot per replica with option forced_parallel on, used for nothing else - score() runs on it from the caller's thread, beside the
        # dispatcher's loops, on the slot's own stream (as a prefill slot does); a lock per replica serialises the calls.  Made before the dispatcher takes the others
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

    def _refuse(self, *features: str) -> None:
        """ValueError with the text of the first row of _REFUSALS, among these features' rows, whose rule the model breaks"""
        for feature, broken, text in _REFUSALS:
            if feature in features and broken(self):
                raise ValueError(text)

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

    def _prepare_all(self, audios, sampling_rate: int, hotwords):
        """per audio: its windows (_prepare), its prompt under the call's one instruction, and its sample count"""
        instruction = frontend.build_instruction(hotwords)
        prepared = [self._prepare(a, sampling_rate) for a in audios]
        return [wins for _, wins, _ in prepared], [self.prompt.build(instruction, n_audio) for _, _, n_audio in prepared], [len(pcm) for pcm, _, _ in prepared]

    def _eos_ids(self) -> List[int]:
        return [int(t) for t in self.dims.eos_ids]       # (NoBadWordsLogitsProcessor drops a bad word equal to [eos])

    def _request_bias(self, hotwords, sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None):
        """One call's table: the constructor's defaults, the call's sequence_bias / bad_words_ids, then - for a boost > 0 (None: the constructor's) - the call's
        hotwords as entries (reqbias.hotword_entries: each hotword as it stands and with one leading space, every prefix of 1 .. 8 tokens).  None when nothing
        applies.  ValueError naming request_bias when the call gives a value and the model was built without the option."""
        explicit = sequence_bias is not None or bad_words_ids is not None or (hotword_boost is not None and float(hotword_boost) != 0.0)
        if explicit and not self.request_bias:
            raise ValueError("sequence_bias / bad_words_ids / hotword_boost need a model built with request_bias=True (ASRModel(..., request_bias=True))")
        if not self.request_bias:
            return None
        if self.bulk:
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
        """One call's sampling: None (a model without the option, nothing asked), or the sampling.CallSampling - temperatures, is it a ladder, seed, (top_k, top_p,
        min_p) - from the call's values over the constructor's defaults; with all three of the cut off such a request states pairs, as it always did
        (CallSampling.attempt).  `cut` in: the call's three values, None for one it does not state.  ValueError naming sampling when the call gives a value and the
        model was built without the option."""
        cut = (None, None, None) if cut is None else tuple(cut)
        if not self.sampling:
            if temperature is not None or seed is not None:
                raise ValueError("temperature / seed" + _NEEDS_SAMPLING)
            if any(v is not None for v in cut):
                raise ValueError("top_k / top_p / min_p" + _NEEDS_SAMPLING)
            return None
        if self.bulk:
            raise ValueError("a temperature is not supported with bulk=True")
        ts, ladder = sampling_.temperatures(self._default_temperature if temperature is None else temperature)
        if ladder and not ladder_ok:
            raise ValueError("stream decodes take one temperature (a float), not a fallback ladder")
        c = sampling_.check_truncation(*[d if v is None else v for v, d in zip(cut, getattr(self, "_default_cut", NO_CUT))])
        return CallSampling(ts, ladder, sampling_.check_seed(self._default_seed if seed is None else seed), c)

    def compile_grammar(self, phrases_or_grammar, repeat: bool = False):
        """A grammar for `grammar=` of the transcribe calls: a grammar.Grammar, or a list of phrases (grammar.Grammar.from_phrases: each phrase, cleaned as hotwords
        are, as it stands and with one leading space, ending in EOS; repeat=True: any number of phrases in a row; needs the checkpoint's tokenizer).  Returns a
        grammar.CompiledGrammar that lives on every replica and serves any number of requests; it is closed with the model, or earlier by its close() (refused while
        a request still refers to it).  Needs a model built with grammar=True."""
        self._check_live()
        if not self.grammar:
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
        if not self.grammar:
            raise ValueError("grammar= needs a model built with grammar=True (ASRModel(..., token_logprobs=True, grammar=True))")
        if self.bulk:
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
        if not self.draft_verify:
            raise ValueError("draft= needs a model built with draft_verify=True (ASRModel(..., draft_verify=True))")
        if bias:
            raise ValueError("draft= cannot be combined with bias values (sequence_bias / bad_words_ids / hotword_boost): the verify pass applies the model's own processors only")
        if samp is not None and (samp.ladder or any(t > 0 for t in samp.temperatures)):
            raise ValueError("draft= cannot be combined with a temperature ladder or a temperature > 0: an accepted draft token is the model's argmax, not a sample")
        if gram is not None:
            raise ValueError("draft= cannot be combined with a grammar: the verify pass applies the model's own processors only")
        ids = cut_draft(self._candidate_ids(draft), self._eos_ids(), max_new)
        return ids or None

    def _request_values(self, call: CallKeywords, hotwords, max_new: int, ladder_ok: bool = True, best_of: int = 1) -> CallValues:
        """One call's own values, checked in this order: bias, samp, gram, draft as _request_bias, _request_sampling, _request_grammar and _request_draft give
        them - what _dispatch takes behind `detailed`, and reqvalues.submit_keywords turns into Dispatcher.submit's keywords.  This is the one place that reads the
        call's keywords.  best_of: what _request_best_of gave for call.best_of, which the entries that take one resolve ahead of everything else."""
        bias = self._request_bias(hotwords, call.sequence_bias, call.bad_words_ids, call.hotword_boost)
        samp = self._request_sampling(call.temperature, call.seed, ladder_ok=ladder_ok, cut=(call.top_k, call.top_p, call.min_p))
        gram = self._request_grammar(call.grammar)
        return CallValues(bias, samp, gram, self._request_draft(call.draft, max_new, bias, samp, gram), best_of)

    def _request_best_of(self, best_of=None) -> int:
        """One call's best_of: the constructor's N when the call states none.  ValueError naming best_of for a value on a model built without best_of > 1, and for
        one outside 1 .. max_batch."""
        N = int(self.best_of)
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

    def _forked_run(self, replica: int, windows_per_audio, prompts, budgets, biases, grams, samp: CallSampling, temperature: float, n: int) -> List[Transcription]:
        """ONE forked run on the replica's fork handle (the caller is that replica's worker thread): every audio becomes n rows that share its encoder pass and
        prefill; fork j decodes at `temperature` (above 0) with seed sampling.fork_seed(samp.seed, j), under the call's cut and the audio's own bias table, grammar and
        budget.  Per audio the Transcription fallback.pick_best selects, with best_of, fork_index and fork_avg_logprobs filled in."""
        eng = self._fork_engines[replica]
        forks = [n] * len(prompts)
        rows = Engine.fork_rows(forks)
        told, bias_rows, gram_rows = [None] * (n * len(prompts)), [None] * (n * len(prompts)), [None] * (n * len(prompts))
        for a, rr in enumerate(rows):
            for j, r in enumerate(rr):
                told[r] = samp.attempt(temperature, sampling_.fork_seed(samp.seed, j))      # (every fork under the same cut)
                bias_rows[r] = biases[a] if biases[a] else None
                gram_rows[r] = None if grams[a] is None else grams[a].on(eng)
        kw = {k: vals for k, vals in (("request_bias", bias_rows), ("request_grammar", gram_rows)) if any(v is not None for v in vals)}
        segs, req_win = _flatten(windows_per_audio)
        ids, _, lps = eng.transcribe_batch(segs, prompts, budgets, req_win=req_win, want_logprobs=True, request_sampling=told, forks=forks, **kw)
        out = []
        for a, rr in enumerate(rows):
            trs = [Transcription(self.prompt.decode(ids[r]).strip(), ids[r], lps[r], temperature) for r in rr]
            avgs = [t.avg_logprob for t in trs]
            j = fallback.pick_best(avgs)
            win = trs[j]
            win.best_of, win.fork_index, win.fork_avg_logprobs = n, j, np.asarray(avgs, np.float64)
            out.append(stamp(win, temperature, samp.cut, grams[a]))
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

    def _forked_attempt(self, windows, prompt, max_new: int, values: CallValues, temperature: float, route) -> "Future":
        """one request's sampled attempt as a forked run of values.best_of rows -> a future of the winning Transcription"""
        runs = self._forked_post(self._fork_replica(route), [windows], [prompt], [max_new], [values.bias], [values.gram], values.samp, float(temperature), values.best_of)
        return then(runs, lambda winners: winners[0])

    def _dispatch(self, windows, prompt, max_new: int, detailed: bool, values: CallValues, **route) -> "Future":
        """One request on the scheduler -> a future of its text (detailed: its Transcription).  values.samp (from _request_sampling): None, one attempt at a temperature,
        or the fallback ladder - each attempt a new request for the same windows, prompt, table and seed; the future resolves after the last one.  Retries
        are submitted by the model's worker thread, never by a completion callback and never by the caller (fallback.py).  values.best_of = n > 1 (from
        _request_best_of): an attempt at a temperature above 0 is ONE forked run of n samples on the replica's fork handle, whose winner stands for the attempt
        (_forked_run); an attempt at temperature 0 is the one greedy decode it always was."""
        samp, gram = values.samp, values.gram
        kw = dict(route, **reqvalues.submit_keywords(values))

        def attempt(temperature, want: bool, draft=None, **stated):
            """one decode at one temperature -> a future of its Transcription (want) or its text.  stated: a ladder's `sampling=` of this attempt (one temperature
            states its own in kw).  (top_k, top_p, min_p): every rung of a ladder above 0 and every fork repeat them"""
            if values.best_of > 1 and temperature > 0:
                fut = self._forked_attempt(windows, prompt, max_new, values, temperature, route)
                return fut if want else _only_text(fut)
            return _text_future(self._dispatcher.submit(windows, prompt, max_new, want_logprobs=want, **stated, **kw), self.prompt.decode, want, temperature,
                                grammar=gram, draft=draft, cut=() if samp is None else samp.cut)
        if samp is None or not samp.ladder:
            return attempt(0.0 if samp is None else samp.temperatures[0], detailed, values.draft)
        policy = fallback.FallbackPolicy(samp.temperatures, self.compression_ratio_threshold, self.logprob_threshold)
        fut = fallback.decode_with_fallback(lambda temperature, seed: attempt(temperature, True, sampling=samp.attempt(temperature, seed)), policy, samp.seed, retrier=self._retrier)
        return fut if detailed else _only_text(fut)

    def _check_live(self):
        if not hasattr(self, "model"):
            raise RuntimeError("ASR model has been released")

    def _check_detailed(self, detailed: bool):
        if detailed and not self.token_logprobs:
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
        call = CallKeywords(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed, grammar=grammar, draft=draft, best_of=best_of, top_k=top_k, top_p=top_p, min_p=min_p)
        return self._submit(call, audio_tensor, sampling_rate, max_new_tokens, hotwords, session, detailed, word_timestamps)

    def _submit(self, call: CallKeywords, audio_tensor, sampling_rate: int, max_new_tokens: int, hotwords, session=None, detailed: bool = False, word_timestamps: bool = False) -> "Future[str]":
        """submit() behind its keywords: what transcribe_async, transcribe and transcribe_batch(word_timestamps=True) call with their own"""
        self._check_live()
        if word_timestamps:
            raise ValueError("word_timestamps is not supported on submit() / transcribe_async() / stream decodes: align a finished transcript with ASRModel.align(), or use transcribe(..., word_timestamps=True)")
        self._check_detailed(detailed)
        n_best = self._request_best_of(call.best_of)
        values = self._request_values(call, hotwords, int(max_new_tokens), best_of=n_best)
        pcm, windows, n_audio = self._prepare(audio_tensor, sampling_rate)
        prompt = self.prompt.build(frontend.build_instruction(hotwords), n_audio)
        return self._dispatch(windows, prompt, int(max_new_tokens), detailed, values, session=session)

    def open_stream(self, session: str, buffer_seconds: float = 30.0, margin_seconds: float = 10.0, sampling_rate: int = 16000) -> AudioStream:
        """A streaming session whose audio stays on the device (config.py:25 MAX_AUDIO_BUFFER_SECONDS = 30): chunks are appended to a
        ring on the session's GPU, partial / final decodes name chunk ranges (AudioStream).  The ring holds `margin_seconds` more than
        the buffer, so a max-length final that waits in the queue is not overwritten by the chunks that keep arriving."""
        self._check_live()
        if sampling_rate == self.target_sr:
            return AudioStream(self, session, self._dispatcher.home(session), buffer_seconds, margin_seconds)
        return AudioStream(self, session, self._dispatcher.home(session), buffer_seconds, margin_seconds, sampling_rate=sampling_rate)

    async def transcribe_async(self, audio_tensor, sampling_rate: int = 16000, max_new_tokens: int = 128,
                               hotwords: Optional[List[str]] = None, session: Optional[str] = None, detailed: bool = False,
                               sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None, temperature=None, seed: Optional[int] = None,
                               word_timestamps: bool = False, grammar=None, draft=None, best_of: Optional[int] = None, top_k=None, top_p=None, min_p=None) -> str:
        """Awaitable transcribe() for the asyncio callers (connection_manager.py:127-245): the event loop is not blocked while the
        device works, so all sessions' partial and final decodes can be in flight (and batched) together."""
        call = CallKeywords(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed, grammar=grammar, draft=draft, best_of=best_of, top_k=top_k, top_p=top_p, min_p=min_p)
        return await asyncio.wrap_future(self._submit(call, audio_tensor, sampling_rate, max_new_tokens, hotwords, session, detailed, word_timestamps))

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
        call = CallKeywords(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed, grammar=grammar, draft=draft, best_of=best_of, top_k=top_k, top_p=top_p, min_p=min_p)
        self._check_live()
        if word_timestamps:
            self._check_timestamps()
        t0 = time.time()
        try:
            want = bool((return_debug_info or word_timestamps) and self.token_logprobs)
            res = self._submit(call, audio_tensor, sampling_rate, max_new_tokens, hotwords, detailed=want).result()
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
                    if self.top_logprobs:             # a top_logprobs model: the K best ids of every step and their log-probabilities
                        info.update({"top_token_ids": det.top_token_ids, "top_logprobs": det.top_logprobs})
                    if self.sampling:             # a sampling model: what the transcript was decoded at, and the ladder's other measure
                        info.update({"temperature": det.temperature, "compression_ratio": det.compression_ratio, "top_k": det.top_k, "top_p": det.top_p, "min_p": det.min_p})
                    if self.best_of > 1:              # a best_of model: how many samples the returned attempt drew, and which of them this is
                        info.update({"best_of": det.best_of, "fork_index": det.fork_index})
                    if self.lm is not None:           # an lm model: the weight, and what the language model alone says of the returned ids
                        info.update({"lm_weight": self.lm_weight, "lm_logprob": self.lm.walk(det.token_ids)[1]})
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
        call = CallKeywords(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed, best_of=best_of, top_k=top_k, top_p=top_p, min_p=min_p)      # (the grammars and drafts: per audio)
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
            futs_ = [self._submit(call._replace(grammar=grams[i], draft=None if drafts is None else drafts[i]), a, sampling_rate, mn_[i], hotwords, detailed=True) for i, a in enumerate(audios)]
            dets = [f.result() for f in futs_]
            self._attach_alignment(list(audios), dets, sampling_rate, hotwords)
            return dets
        shared = self._request_values(call, hotwords, 0, best_of=n_best)
        mn = [int(max_new_tokens)] * len(audios) if isinstance(max_new_tokens, int) else [int(x) for x in max_new_tokens]
        samp = shared.samp
        values = [shared._replace(gram=g, draft=None if drafts is None else self._request_draft(drafts[i], mn[i], shared.bias, samp, g)) for i, g in enumerate(grams)]
        wins_of, prompts, _ = self._prepare_all(audios, sampling_rate, hotwords)
        if samp is not None and samp.ladder:
            futs = [self._dispatch(wins_of[i], prompts[i], mn[i], False, values[i]) for i in range(len(audios))]
            return [f.result() for f in futs]
        if samp is not None and n_best > 1 and samp.temperatures[0] > 0:
            # one temperature above 0: floor(max_batch / best_of) audios per forked run, the runs spread over the replicas' fork handles in turn
            per = max(1, self._max_batch // n_best)
            runs = [self._forked_post(self._fork_replica({}), [wins_of[i] for i in g], [prompts[i] for i in g], [mn[i] for i in g],
                                      [shared.bias] * len(g), [grams[i] for i in g], samp, samp.temperatures[0], n_best)
                    for g in (range(g0, min(g0 + per, len(audios))) for g0 in range(0, len(audios), per))]
            return [t.text for r in runs for t in r.result()]
        subs = [reqvalues.submit_keywords(v) for v in values]
        if len(self.models) == 1 and not self.continuous:
            # one engine call: a value that some audio brings becomes its keyword's list, None for the audios without it
            kw = {v.keyword: [v.on(s.get(v.attr), self.model) for s in subs] for v in reqvalues.VALUES if any(v.attr in s for s in subs)}
            segs, req_win = _flatten(wins_of)
            ids, _ = self.model.transcribe_batch(segs, prompts, mn, req_win=req_win, **kw)
        else:            # independent segments: spread over the replicas (least-loaded placement), results in input order
            futs = [self._dispatcher.submit(wins_of[i], prompts[i], mn[i], **subs[i]) for i in range(len(audios))]
            ids = [f.result() for f in futs]
        return [self.prompt.decode(i).strip() for i in ids]

    # -- scoring: how probable is THIS transcript, given THIS audio
    def _candidate_ids(self, cand) -> List[int]:
        if isinstance(cand, str):
            if not isinstance(self.prompt, HFPrompt):
                raise ValueError("a text candidate needs a tokenizer (a checkpoint with its processor): the synthetic prompt has none - pass token ids")
            return [int(t) for t in self.prompt.processor.tokenizer.encode(cand, add_special_tokens=False)]
        return [int(t) for t in np.asarray(cand).reshape(-1)]

    def lm_score(self, text_or_ids) -> float:
        """The sum of the language model's log-probabilities (natural log, unweighted) over a transcript - a string, tokenised with the checkpoint's tokenizer, or
        token ids - walked from the model's start node (ngram.NGramLM.walk).  Needs a model built with lm=."""
        if self.lm is None:
            raise ValueError("lm_score needs a model built with lm= (ASRModel(..., token_logprobs=True, lm=...))")
        return float(self.lm.walk(self._candidate_ids(text_or_ids))[1])

    def share_prompt_refusal(self) -> Optional[str]:
        """why this model's scoring handles cannot share a prompt, or None: the library refuses the same by the option's name"""
        return _SHARE_INT8 if self.mode == "int8" else _SHARE_ALIGN if self.timestamps else None

    def score(self, audio, candidates, sampling_rate: int = 16000, hotwords: Optional[List[str]] = None, append_eos: bool = True,
              share_prompt: Optional[bool] = None) -> List["Score"]:
        """The log-probability of each candidate transcript given the audio: n-best / hotword-list rescoring, keyword verification, comparing an edited
        transcript with the greedy one.  A candidate is a string (tokenised with the checkpoint's tokenizer) or a sequence of token ids.  The prompt is the one
        transcribe() builds (same hotword sentence, same audio-token count); all candidates share one encoder pass.  append_eos: the first EOS id is appended as a
        last target, so that hypotheses of different length compare as HF's sequence scores do.  The scores are those of the raw model distribution at temperature
        1: no logits processor (repetition penalty, bias, ...) is applied, whatever the model carries.  Needs a model built with scoring=True.  share_prompt (None: the
        model's score_share_prompt): the candidates also share one prefill of the prompt, so a long list costs its candidates' own tokens and fits fewer runs
        (DESIGN.md 6.14); the scores agree with the unshared ones to the attention's rounding, not bit for bit."""
        return self.score_batch([audio], [candidates], sampling_rate, hotwords, append_eos, share_prompt)[0]

    def score_batch(self, audios: Sequence[Any], candidates_per_audio: Sequence[Sequence[Any]], sampling_rate: int = 16000,
                    hotwords: Optional[List[str]] = None, append_eos: bool = True, share_prompt: Optional[bool] = None) -> List[List["Score"]]:
        """score() for several audios, each with its own candidates: as few runs as hold them (scoring.plan_runs), the same bits as one call per audio."""
        self._check_live()
        if not self.scoring or not self._score_engines:
            raise ValueError("score() needs a model built with scoring=True (ASRModel(..., token_logprobs=True, scoring=True))")
        if len(audios) != len(candidates_per_audio):
            raise ValueError(f"{len(audios)} audios but {len(candidates_per_audio)} candidate lists")
        share = self.score_share_prompt if share_prompt is None else bool(share_prompt)
        if share and self.share_prompt_refusal():
            raise ValueError(self.share_prompt_refusal())
        eos = self._eos_ids()
        wins_of, prompts, _ = self._prepare_all(audios, sampling_rate, hotwords)
        targets = [[scoring_.with_eos(self._candidate_ids(c), eos, append_eos) for c in cands] for cands in candidates_per_audio]
        i = self._score_next % len(self._score_engines)
        self._score_next += 1
        eng = self._score_engines[i]
        runs = scoring_.plan_runs([len(p) for p in prompts], [[len(t) for t in ts] for ts in targets], eng.max_batch, eng.tok_cap, eng.max_ctx, share_prompt=share)
        dummy = next(t for t in range(self.dims.vocab) if t != self.dims.audio_token_id and t not in eos)
        out: List[List[Optional[scoring_.Score]]] = [[None] * len(ts) for ts in targets]
        with self._score_locks[i]:
            for run in runs:
                segs, req_win = _flatten(wins_of[a] for a, _ in run.groups)
                run_prompts = [prompts[a] for a, part in run.groups for _ in part]
                ids, _, lps = eng.score_batch(segs, run_prompts, scoring_.run_targets(run, targets, dummy), req_win=req_win, fanout=run.fanout, share_prompt=share)
                r = 0
                for a, part in run.groups:
                    for c in part:
                        if c is not None:        # (a dummy's result is cut again)
                            out[a][c] = scoring_.Score(self.prompt.decode(ids[r]).strip(), ids[r], lps[r])
                        r += 1
        return out      # type: ignore[return-value]

    # -- word timestamps: WHEN was this transcript spoken
    def _check_timestamps(self):
        if not self.timestamps or not getattr(self, "_score_engines", None):
            raise ValueError("word timestamps need a model built with timestamps=True (ASRModel(..., token_logprobs=True, scoring=True, timestamps=True))")

    def _pieces_of(self, ids: Sequence[int]):
        """the tokens' text pieces for word grouping (timestamps.split_pieces): the tokenizer's, or - the synthetic prompt has none - one word per token"""
        if isinstance(self.prompt, HFPrompt):
            tok = self.prompt.processor.tokenizer
            return timestamps_.split_pieces(ids, lambda t: tok.decode(t, skip_special_tokens=False))
        return [(" " + str(int(t)), [i]) for i, t in enumerate(ids)]

    def _align_items(self, items, replica: Optional[int] = None):
        """items: (windows, prompt ids, target ids with their EOS, samples of the audio) each -> one timestamps.Alignment each, in as few parallel forced runs on
        a scoring handle as hold them (scoring.plan_runs, one candidate per audio).  replica: the handle of that replica (ring slices live on one GPU)."""
        self._check_timestamps()
        if replica is None:
            replica = self._score_next % len(self._score_engines)
            self._score_next += 1
        eng = self._score_engines[replica]
        runs = scoring_.plan_runs([len(it[1]) for it in items], [[len(it[2])] for it in items], eng.max_batch, eng.tok_cap, eng.max_ctx)
        out: List[Any] = [None] * len(items)
        with self._score_locks[replica]:
            for run in runs:
                who = [a for a, part in run.groups for c in part if c is not None]
                segs, req_win = _flatten(items[a][0] for a in who)
                ids, _, sc = eng.score_batch(segs, [items[a][1] for a in who], [items[a][2] for a in who], req_win=req_win, fanout=1, align=True)
                for r, a in enumerate(who):
                    n_samples = int(items[a][3])
                    total, per_win = frontend.request_audio_tokens(n_samples, self.dims)
                    out[a] = timestamps_.build_alignment(ids[r], sc[r].lp, sc[r].times, self._eos_ids(), per_win, total, n_samples / self.target_sr, self._pieces_of,
                                                         self.dims.chunk_seconds)
        return out

    def _align_audios(self, audios, ids_per_audio, sampling_rate: int, hotwords):
        """one timestamps.Alignment per audio for its token ids, under the prompt transcribe() builds; the first EOS id is appended as a last target"""
        eos = self._eos_ids()
        wins_of, prompts, samples = self._prepare_all(audios, sampling_rate, hotwords)
        return self._align_items([(w, p, scoring_.with_eos(ids, eos, True), n) for w, p, ids, n in zip(wins_of, prompts, ids_per_audio, samples)])

    def _attach_alignment(self, audios, dets, sampling_rate: int, hotwords):
        """align the decoded tokens of each Transcription and hang words / token times on it"""
        for det, al in zip(dets, self._align_audios(audios, [[int(t) for t in det.token_ids] for det in dets], sampling_rate, hotwords)):
            det.words, det.token_start, det.token_end = al.words, al.token_start, al.token_end

    def align(self, audio, transcript, sampling_rate: int = 16000, hotwords: Optional[List[str]] = None):
        """When every token and word of `transcript` (a string, tokenised with the checkpoint's tokenizer, or a sequence of token ids) was spoken in `audio`: a
        timestamps.Alignment.  The prompt is the one transcribe() builds; the first EOS id is appended as a last target (its row takes part in the normalisation
        over tokens and is dropped from the result).  Needs a model built with timestamps=True."""
        return self.align_batch([audio], [transcript], sampling_rate, hotwords)[0]

    def align_batch(self, audios: Sequence[Any], transcripts: Sequence[Any], sampling_rate: int = 16000, hotwords: Optional[List[str]] = None):
        """align() for several audios, each with its transcript: as few runs as hold them, the same bits as one call per audio."""
        self._check_live()
        self._check_timestamps()
        if len(audios) != len(transcripts):
            raise ValueError(f"{len(audios)} audios but {len(transcripts)} transcripts")
        return self._align_audios(audios, [self._candidate_ids(t) for t in transcripts], sampling_rate, hotwords)

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
        call = CallKeywords(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed, grammar=grammar, top_k=top_k, top_p=top_p, min_p=min_p)
        return filemode.transcribe_file(self, call, audio, vad, vad_enabled, hotwords, max_segment_duration, max_new_tokens, filename, sampling_rate, word_timestamps)

    def transcribe_files(self, audios: Sequence[Any], vad, vad_enabled: bool = True, hotwords: Optional[List[str]] = None,
                         max_segment_duration: Optional[float] = None, max_new_tokens: int = 256, filenames: Optional[Sequence[str]] = None,
                         sampling_rate: int = 16000, sequence_bias=None, bad_words_ids=None, hotword_boost: Optional[float] = None, temperature=None,
                         seed: Optional[int] = None, word_timestamps: bool = False, grammar=None, top_k=None, top_p=None, min_p=None):
        """transcribe_file for several files: all VAD passes in one device call, one record iterator per file (filemode.transcribe_files)."""
        from . import filemode
        call = CallKeywords(sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, hotword_boost=hotword_boost, temperature=temperature, seed=seed, grammar=grammar, top_k=top_k, top_p=top_p, min_p=min_p)
        return filemode.transcribe_files(self, call, audios, vad, vad_enabled, hotwords, max_segment_duration, max_new_tokens, filenames, sampling_rate, word_timestamps)

    def get_model_info(self) -> Dict[str, Any]:
        """asr.py:490-513: the reference's keys for a GPU device (`cuda_version` carries the HIP runtime version: torch.version.cuda is
        the toolkit the reference's torch was built with), plus `engine`, `replicas`, `weights_mb`."""
        info = {"mode": self.mode, "device": str(self.device), "model_dtype": "torch." + self.model_dtype, "target_sampling_rate": self.target_sr,
                "checkpoint_dir": str(self.checkpoint_dir), "is_glm_asr": self.is_glm_asr}
        di = device_info(self.device_index)
        v = di["hip_runtime_version"]
        info.update({"cuda_version": f"HIP {v // 10000000}.{(v // 100000) % 100}.{v % 100000}", "gpu_name": di["name"],
                     "gpu_memory_total_mb": di["total_bytes"] / 1024 ** 2})
        info.update({"engine": "sonicscribe_amd/gfx950", "replicas": len(self.__dict__.get("models", [])), "slots_per_replica": self.slots, "continuous": self.continuous, "bulk": self.bulk,
                     "weights_mb": self.model.weight_bytes() / 1024 ** 2 if hasattr(self, "model") else 0.0})
        info.update({"scoring": self.scoring, "grammar": self.grammar, "draft_verify": self.draft_verify, "best_of": self.best_of, "timestamps": self.timestamps,
                     "lm": self.lm is not None, "lm_weight": self.lm_weight if self.lm is not None else 0.0})
        if self.mode == "fp8" and hasattr(self, "model"):      # mode fp8: what the e4m3 copies add to weights_mb, and the token steps the dispatcher's handles built in the fp8 form
            handles = list(self.models) + [s for ss in self.__dict__.get("_slot_engines", []) for s in ss]
            info.update({"fp8_weights_mb": self.model.fp8_info()["extra_weight_bytes"] / 1024 ** 2, "fp8_step_builds": sum(h.fp8_info()["step_builds"] for h in handles)})
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
