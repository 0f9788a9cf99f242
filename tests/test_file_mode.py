"""File-mode segment planning (sonicscribe_amd/filemode.py::plan_segments) against tests/golden/file_mode.npz, which
tools/gen_file_mode_fixtures.py recorded from the reference's own endpoint and helper functions (backend/main.py:274-363, 527-583):
the sample ranges the endpoint handed to its model, its segment_result records, and cut_long_segments / get_segments_summary called
directly.  Plus the input forms transcribe_file accepts and refuses.  No GPU."""
import json
import os

import numpy as np
import pytest

from sonicscribe_amd import filemode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "file_mode.npz")
CASES = json.loads(str(np.load(GOLDEN)["cases"]))

REQUIRED = ["vad_off_short", "vad_off_long", "below_one_second", "no_speech", "touching_ends", "pair_closer_than_100", "exactly_max_30",
            "exactly_max_15", "last_sub_dropped_30", "last_sub_dropped_15", "mixed_30", "mixed_15"]


def plan(case):
    cfg = case["config"]
    return filemode.plan_segments(case["total_samples"], case["timestamps"], cfg.get("vad_enabled", True), case["max_segment_duration"])


def test_fixture_holds_the_cases():
    assert set(REQUIRED) <= set(CASES)
    assert {c["max_segment_duration"] for c in CASES.values()} >= {15.0, 30.0}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_equals_reference(name):
    case = CASES[name]
    final, summary = plan(case)
    sr = filemode.SAMPLE_RATE
    # what the endpoint decoded: every planned segment of at least 0.1 s, as the sample range its model was handed
    decodable = [s for s in final if s["end_sample"] - s["start_sample"] >= int(0.1 * sr)]
    assert [[s["start_sample"], s["end_sample"]] for s in decodable] == [list(r) for r in case["decoded_ranges"]]
    assert case["n_results"] == len(decodable)
    by_index = {s["segment_index"]: s for s in summary}
    for rec in case["segment_results"]:
        got = by_index[rec["segment_index"]]
        for k in ("original_index", "start_time", "end_time", "duration", "is_long_segment"):
            assert got[k] == rec[k], (name, rec["segment_index"], k)
    assert [s["segment_index"] for s in final] == list(range(1, len(final) + 1))
    # the two helper functions called directly on the closure's raw segments: field for field, floats exactly
    if case["direct"] is not None:
        assert final == case["direct"]["final"]
        assert summary == case["direct"]["summary"]
    # VAD off or a file below 1 s: the reference never called its VAD, and timestamps change nothing here
    if case["vad_calls"] == 0:
        again, _ = filemode.plan_segments(case["total_samples"], [{"start": 10, "end": 5000}], case["config"].get("vad_enabled", True),
                                          case["max_segment_duration"])
        assert again == final


def test_properties_named_by_the_cases():
    f, _ = plan(CASES["last_sub_dropped_30"])
    assert [s["sub_segment_index"] for s in f[:2]] == [1, 2] and f[0]["sub_segment_count"] == 3 and f[2]["sub_segment_count"] == 1
    assert all("original_duration" in s for s in f[:2]) and "original_duration" not in f[2]
    f, _ = plan(CASES["last_sub_kept_30"])
    assert len(f) == 3 and f[2]["end_sample"] - f[2]["start_sample"] == 1601
    f, _ = plan(CASES["exactly_max_30"])
    assert not f[0]["is_long_segment"] and f[0]["sub_segment_count"] == 1          # exactly 30 s is not cut
    assert f[1]["is_long_segment"] and f[1]["sub_segment_count"] == 2 and len(f) == 2   # 30 s + 1 sample: the second piece is dropped
    f, _ = plan(CASES["pair_closer_than_100"])
    assert len(f) == 1 and f[0]["original_index"] == 2
    f, _ = plan(CASES["tiny_file"])
    assert len(f) == 1 and f[0]["end_sample"] == 1000                               # planned; the decode refuses it (segment_error)
    f, _ = plan(CASES["no_speech"])
    assert [(s["start_sample"], s["end_sample"]) for s in f] == [(0, 20 * 16000)]


def test_input_forms():
    pcm = (np.arange(-5, 5) * 3000).astype(np.int16)
    assert np.array_equal(filemode.as_pcm16(pcm), pcm) and np.array_equal(filemode.as_pcm16(pcm[None, :]), pcm)
    f32 = pcm.astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(filemode.as_pcm16(f32[None, :]), pcm)
    import torch
    assert np.array_equal(filemode.as_pcm16(torch.from_numpy(f32).unsqueeze(0)), pcm)
    edge = np.array([-1.0, 32767 / 32768], np.float32)
    assert filemode.as_pcm16(edge).tolist() == [-32768, 32767]
    for bad in (np.array([0.3], np.float32), np.array([1.0], np.float32), np.array([np.nan], np.float32), np.zeros((2, 8), np.float32),
                np.zeros(4, np.int32)):
        with pytest.raises(ValueError):
            filemode.as_pcm16(bad)
