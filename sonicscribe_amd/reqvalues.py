"""The values a request may bring of its own, listed once: what dispatch.py and engine.py need to know about each to carry it from a dispatch.Request to an engine
handle.  A further value is one entry here plus its packing code (Engine.set_request_<x>, the keyword of Engine.transcribe_batch / prefill, and
_NativeContinuousReplica.put's way to the library).  This module imports neither dispatch nor engine: both import it."""
from __future__ import annotations

from collections import namedtuple

# attr:    the attribute of dispatch.Request (and the keyword of Dispatcher.submit)
# option:  the engine option that admits the value, mirrored as an attribute of the handle (engine.MIRRORED_OPTIONS)
# keyword: the keyword of Engine.transcribe_batch / Engine.prefill that takes one value or None per request
# setter:  the method of a handle that arms the values of its next prefill
# off:     the refusal of a request that brings the value to handles without the option
# on:      (the request's value, a handle) -> the value as that handle takes it
# lead:    what the native dispatcher's refusals of the value start with, ahead of a colon (csrc/dispatch.cpp sonic_dispatch_submit)
ReqValue = namedtuple("ReqValue", "attr option keyword setter off on lead")

# in the order every site arms them and states their keywords
VALUES = (
    ReqValue("bias", "request_bias", "request_bias", "set_request_bias",
             "a sequence bias needs the engine option request_bias on every handle (ASRModel(request_bias=True))", lambda table, engine: table, "request_bias"),
    ReqValue("sampling", "sampling", "request_sampling", "set_request_sampling",
             "a temperature needs the engine option sampling on every handle (ASRModel(sampling=True))", lambda pair, engine: pair, "sampling"),      # ((t, seed), or (t, seed, top_k, top_p, min_p): passed through unchanged; the cut's refusals start with "truncation")
    # (a grammar.CompiledGrammar holds a device handle per weight owner: the one that serves `engine`; None: a free request)
    ReqValue("grammar", "grammar", "request_grammar", "set_request_grammar",
             "a grammar needs the engine option grammar on every handle (ASRModel(token_logprobs=True, grammar=True))", lambda g, engine: None if g is None else g.on(engine), "grammar"),
    ReqValue("draft", "draft_verify", "request_draft", "set_request_draft",
             "a draft needs the engine option draft_verify on every handle (ASRModel(draft_verify=True))", lambda ids, engine: ids, "draft"),
)
DRAFT = VALUES[3]


def _stated(engine, reqs):
    """(entry, the requests' values as `engine` takes them - None for a request without one) for every value that the engine's option admits or that some request
    brings.  A handle with the option on is ALWAYS told its batch's values, so a batch never depends on what an earlier, failed one left behind; a duck-typed engine
    without the option hears of a value only when somebody brought one.  Lazy: a value's list is built when the caller reaches it."""
    for v in VALUES:
        if getattr(engine, v.option, False) or any(getattr(r, v.attr) for r in reqs):
            yield v, [v.on(getattr(r, v.attr), engine) for r in reqs]


def keywords(engine, reqs) -> dict:
    """the per-request keywords of engine.transcribe_batch(...) for the batch `reqs`"""
    return {v.keyword: values for v, values in _stated(engine, reqs)}


def arm(engine, reqs) -> None:
    """the set_request_* calls ahead of engine.prefill(...) for the batch `reqs`: row i of that prefill is reqs[i]; the prefill consumes them"""
    for v, values in _stated(engine, reqs):
        getattr(engine, v.setter)(values)


def supported(engines) -> tuple:
    """per entry of VALUES: does every handle have the option on, so that a request may bring the value"""
    return tuple(all(getattr(e, v.option, False) for e in engines) for v in VALUES)


def refuse_unsupported(req, flags) -> None:
    """ValueError by name for a bias table, a temperature or a grammar that the handles do not admit (flags: supported(engines)), in that order.  A draft is
    check_draft's to refuse: it has a second rule, and the callers differ in what they check ahead of it."""
    for v, ok in zip(VALUES, flags):
        if v is not DRAFT and getattr(req, v.attr) and not ok:
            raise ValueError(v.off)


def check_draft(req, engines) -> None:
    """ValueError by name unless every handle verifies drafts, and for a draft beside a bias table, a temperature > 0 or a grammar (the library refuses those too)"""
    if not req.draft:
        return
    if not all(getattr(e, DRAFT.option, False) for e in engines):
        raise ValueError(DRAFT.off)
    if req.bias or req.grammar or (req.sampling and req.sampling[0] > 0):
        raise ValueError("a draft cannot be combined with a bias table, a temperature > 0 or a grammar (the verify pass applies the engine's own processors only)")


# Above the scheduler.  The generation keywords of one call as its public entry received them, None for one the caller did not state or the entry does not take (file mode has no draft
# or best_of, streams no best_of).  Every entry of ASRModel and AudioStream builds it once; from there on only the record travels.  A further keyword is one field
# here, the entries' signatures and constructions, and its line in ASRModel._request_values.
CallKeywords = namedtuple("CallKeywords", "sequence_bias bad_words_ids hotword_boost temperature seed grammar draft best_of top_k top_p min_p", defaults=(None,) * 11)
# One call's own values as ASRModel._request_values resolves them: `bias` a reqbias.RequestBias or None, `samp` a sampling.CallSampling or None (a model without the
# option), `gram` a grammar.CompiledGrammar or None, `draft` its token ids or None, `best_of` the samples of an attempt at a temperature above 0.
CallValues = namedtuple("CallValues", "bias samp gram draft best_of", defaults=(None, None, None, None, 1))


def submit_keywords(values: CallValues) -> dict:
    """One call's own values as the keywords of Dispatcher.submit.  Each only when the request brings it - stub dispatchers need not know the others: `bias` a
    non-empty table, `sampling` for one temperature (a fallback ladder states it attempt by attempt: ASRModel._dispatch; (top_k, top_p, min_p) behind the pair when the
    call cuts the tail), `grammar`, `draft` a non-empty one."""
    kw = {}
    if values.bias:
        kw["bias"] = values.bias
    if values.samp is not None and not values.samp.ladder:
        kw["sampling"] = values.samp.attempt(values.samp.temperatures[0])
    if values.gram is not None:
        kw["grammar"] = values.gram
    if values.draft:
        kw["draft"] = values.draft
    return kw
