"""The launch sequence of every form of the token step and of the prefill, for comparing two builds kernel by kernel.

Run (one build):   rocprofv3 --kernel-trace -d DIR -o kt --output-format csv -- python3 tools/step_trace.py
    rocprofv3 alone: no counters, no other tracing.  Eager token steps (option no_graph), so every launch of a step is a row of the trace.  Cases, in this order:
    the eight (rows, option) cases of tests/test_gpu_step_forms.py on the full-width two-layer decoder and again on TINY, one fp32-kind run, one int8 run, and one
    prefill of three ragged requests on its own (stage_pcm + prefill).
Compare (no GPU):  python3 tools/step_trace.py --compare DIR_A DIR_B
    The ordered lists of (kernel name, grid, workgroup, LDS bytes) of the two traces must be the same list.  One list covers all cases: they run in a fixed order on
    one stream, so the lists are equal exactly if every case's is.  Prints the count, the first difference if there is one, and exits 1 on a difference."""
import torch  # noqa: F401  (first, so that a run under rocprofv3 uses torch's bundled HIP runtime: tools/rocprof_runtime_repro.py)
import csv
import glob
import os
import sys
from dataclasses import replace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [(1, None), (2, None), (2, "no_pre_norm"), (3, None), (3, "decode_gemv"), (33, None), (33, "gu64_split_norm"), (5, "no_fused_gu")]
N_NEW = 3


def requests(d, R):
    from sonicscribe_amd import spec, synth
    lens = [16000 * (1 + (i % 2)) + 37 * i for i in range(R)]
    segs = [synth.synth_pcm(400 + i, n) for i, n in enumerate(lens)]
    prompts = [[1, 17, 23, 5] + [d.audio_token_id] * spec.audio_token_count(spec.valid_frames(n)) + [7, 301, 302, 303, 9, 11][: 3 + i % 4] for i, n in enumerate(lens)]
    return segs, prompts


def run(e, d, R, option=None):
    segs, prompts = requests(d, R)
    if option:
        e.set_option(option, 1)
    try:
        e.transcribe_batch(segs, prompts, [N_NEW] * R)
        return e.timings()["decode_launches_per_layer"]
    finally:
        if option:
            e.set_option(option, 0)


def drive():
    from sonicscribe_amd import spec
    from sonicscribe_amd.engine import Engine, MODE_F32, MODE_INT8
    full = replace(spec.FULL, enc_layers=1, dec_layers=2, vocab=1024, audio_token_id=1000, eos_ids=())
    tiny = replace(spec.TINY, eos_ids=())
    for name, d in (("fullwidth", full), ("tiny", tiny)):
        e = Engine(d, 0, max_batch=64, max_ctx=384)
        e.load_synthetic(11)
        e.set_option("no_graph", 1)
        for R, option in CASES:
            print(name, R, option, "launches per layer", run(e, d, R, option), flush=True)
        if name == "fullwidth":
            segs, prompts = requests(d, 3)
            e.stage_pcm(segs); e.prefill(prompts, [N_NEW] * 3)
            print(name, "prefill of 3 ragged requests", flush=True)
        e.close()
    for name, mode in (("fp32", MODE_F32), ("int8", MODE_INT8)):
        e = Engine(tiny, 0, mode, max_batch=8, max_ctx=512)
        e.load_synthetic(20260128)
        e.set_option("no_graph", 1)
        print(name, 2, None, "launches per layer", run(e, tiny, 2), flush=True)
        e.close()


def launches(path):
    rows = []
    for f in glob.glob(path + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ"), int(r["LDS_Block_Size"])) for r in rows]


def compare(a, b):
    la, lb = launches(a), launches(b)
    print(f"{a}: {len(la)} launches, {len(set(x[0] for x in la))} kernels; {b}: {len(lb)} launches, {len(set(x[0] for x in lb))} kernels")
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            print(f"first difference at launch {i}:\n  {x}\n  {y}")
            return 1
    if len(la) != len(lb) or not la:
        print("one list is a prefix of the other" if la else "empty trace")
        return 1
    print("identical")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    drive()
