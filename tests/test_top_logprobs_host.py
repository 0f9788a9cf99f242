"""Host side of option top_logprobs, on CPU: the one function that unpacks the wide log-probability records, ASRModel's three refusals, the
result object's new arrays, the header's words on the option and the record layout, and the ABI staying what the pinning tests say it is - the feature adds no
entry point.  The GPU halves are tests/test_gpu_top_logprobs_kernel.py and tests/test_gpu_top_logprobs.py."""
import os
import re

import numpy as np
import pytest

from sonicscribe_amd import asr, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = np.float32("-inf")


def test_unpack_wide_records():
    K, W = 3, 7
    rec = np.array([[-0.5, -0.5, -1.25, -3.0, 11, 7, 59263],                       # a greedy step: alternative 0 is the token
                    [-2.0, -0.25, -2.0, NEG, 5, 9, -1],                            # a forced / sampled step with two finite scores: (-1, -inf) fills the rest
                    [-9.0, NEG, NEG, NEG, -1, -1, -1]], np.float32)                # every score banned
    buf = np.full(5 * W, np.nan, np.float32)                                       # room for five tokens, three written
    buf[:3 * W] = rec.reshape(-1)
    got = engine.unpack_logprobs(buf, 3, K)
    assert isinstance(got, engine.TokenScores) and got.lp.dtype == np.float32 and got.top_logprobs.dtype == np.float32 and got.top_ids.dtype == np.int32
    assert got.lp.tolist() == [-0.5, -2.0, -9.0] and got.top_logprobs.shape == got.top_ids.shape == (3, K)
    assert got.top_ids.tolist() == [[11, 7, 59263], [5, 9, -1], [-1, -1, -1]]
    assert np.array_equal(got.top_logprobs, rec[:, 1:4]) and np.isneginf(got.top_logprobs[1, 2]) and np.all(np.isneginf(got.top_logprobs[2]))
    got.lp[0] = 1.0
    assert buf[0] == np.float32(-0.5), "the result owns its memory"
    # ids are exact as fp32 up to 2^24: the largest one survives the round trip
    big = engine.unpack_logprobs(np.array([0.0, -1.0, float(2 ** 24 - 1)], np.float32), 1, 1)
    assert big.top_ids.tolist() == [[2 ** 24 - 1]]
    # K = 0: the array the wrappers returned before the option existed; no tokens: empty arrays of the right shape
    narrow = engine.unpack_logprobs(np.array([-1.0, -2.0, np.nan], np.float32), 2, 0)
    assert isinstance(narrow, np.ndarray) and narrow.dtype == np.float32 and narrow.tolist() == [-1.0, -2.0]
    none = engine.unpack_logprobs(buf, 0, K)
    assert none.lp.shape == (0,) and none.top_logprobs.shape == (0, K) and none.top_ids.shape == (0, K)


def test_asrmodel_refusals_by_name():
    """raised before any engine is built: no device is needed"""
    with pytest.raises(ValueError, match="top_logprobs needs token_logprobs"):
        asr.ASRModel("<none>", top_logprobs=3)
    with pytest.raises(ValueError, match="top_logprobs is not supported with bulk=True"):
        asr.ASRModel("<none>", token_logprobs=True, top_logprobs=3, bulk=True)
    for bad in (-1, 9, 2.5, True, "3"):
        with pytest.raises(ValueError, match=r"top_logprobs must be an integer in 0 \.\. 8"):
            asr.ASRModel("<none>", token_logprobs=True, top_logprobs=bad)
    assert asr.check_top_logprobs(0, False, True) == 0 and asr.check_top_logprobs(8, True, False) == 8 and asr.check_top_logprobs(np.int64(2), True, False) == 2


def test_transcription_carries_the_alternatives():
    sc = engine.TokenScores(np.array([-0.5, -1.5], np.float32), np.array([[-0.5, -2.0], [-1.5, NEG]], np.float32), np.array([[7, 3], [8, -1]], np.int32))
    t = asr.Transcription("7 8", [7, 8], sc)
    assert t.token_logprobs.tolist() == [-0.5, -1.5] and t.avg_logprob == pytest.approx(-1.0)
    assert t.top_token_ids.dtype == np.int32 and t.top_token_ids.tolist() == [[7, 3], [8, -1]] and t.top_logprobs.dtype == np.float32 and t.top_logprobs.shape == (2, 2)
    plain = asr.Transcription("7 8", [7, 8, 990], [-0.5, -1.5, -4.0])              # a model without the option: [n, 0]
    assert plain.top_token_ids.shape == (3, 0) and plain.top_token_ids.dtype == np.int32 and plain.top_logprobs.shape == (3, 0) and plain.top_logprobs.dtype == np.float32
    empty = asr.Transcription("", [], [])
    assert empty.top_token_ids.shape == (0, 0) and empty.top_logprobs.shape == (0, 0)
    # through the future every entry point shares
    from concurrent.futures import Future
    inner = Future()
    out = asr._text_future(inner, lambda ids: " ".join(str(int(i)) for i in ids), True)
    inner.set_result((np.array([7, 8], np.int32), sc))
    r = out.result(timeout=1)
    assert r.text == "7 8" and np.array_equal(r.top_token_ids, sc.top_ids) and np.array_equal(r.top_logprobs, sc.top_logprobs)


def test_header_documents_option_and_layout():
    hdr = open(os.path.join(ROOT, "include", "sonic_hip.h")).read()
    assert '"top_logprobs"' in hdr and "W = 1 + 2K" in hdr and "0 .. 8" in hdr
    for form in ("sonic_fetch_logprobs", "sonic_fetch_rows_lp", "sonic_dispatch_next_lp", "sonic_pipeline_submit_lp", "sonic_splice_rows"):
        assert re.search(r"\* +" + form + r"\b.*(out_ld|out_cap|narrow|one float|refuses|K differ)", hdr), form
    assert "out_lp + i * out_ld * W" in hdr and "out_cap * W floats" in hdr and "id -1 and -inf" in hdr
    assert "ids as fp32" in hdr and "2^24" in hdr
    # no entry point of its own: the option key and the widened records are the whole interface
    assert not re.search(r"sonic_[a-z_]*top[a-z_]*\s*\(", hdr)
    src = open(os.path.join(ROOT, "sonicscribe_amd", "csrc", "engine_options.cpp")).read()
    assert '{"top_logprobs", APPLY(opt_top_logprobs)}' in src
    k = open(os.path.join(ROOT, "sonicscribe_amd", "csrc", "kernels.h")).read()
    assert re.search(r"const unsigned\* samp;\s*(//[^\n]*\n\s*)*int topk;\s*\};", k), "GreedyArgs: the new field is the last one"


def test_abi_pins_still_hold():
    """tests/test_binding_signatures.py and tests/test_host_logic.py pin header, binding table and the library's export table to each other: their checks, called
    as they stand, pass with this feature in - the entry points of today (tests/abi_pins.py), none of them this feature's"""
    import abi_pins
    import test_binding_signatures
    import test_host_logic
    abi_pins.check_surface()
    test_binding_signatures.test_every_declaration_matches_its_binding()
    test_host_logic.test_header_declares_what_library_exports()
