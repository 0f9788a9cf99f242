"""The native dispatcher's packers (sonicscribe_amd/csrc/dispatch_pack.h: pure host code) against engine.pack_request_bias and engine.pack_request_draft, the two
packers of one format, word for word; and its check of a submit's window offsets.  A stand-alone C++ program with its own main is built with the address and undefined-behaviour sanitizers and run as a child
process: it reads batches from stdin and prints the packed arrays.  Nothing is loaded into this process."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from sonicscribe_amd import engine
from sonicscribe_amd.reqbias import RequestBias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include <iostream>
#include <string>
#include "dispatch_pack.h"

template <class T> static void line(const char* name, const std::vector<T>& v) {
    printf("%s", name);
    for (const T& x : v) printf(" %lld", (long long)x);
    printf("\n");
}

int main() {
    std::string kind;
    while (std::cin >> kind) {
        int R = 0;
        std::cin >> R;
        if (kind == "bias") {                                   // per request: n, and for n > 0: m, m ids, n + 1 offsets into them, n biases as their bit patterns
            std::vector<dispatch_pack::BiasTable> own(R);
            for (auto& t : own) {
                int n = 0, m = 0;
                std::cin >> n;
                if (n == 0) continue;
                std::cin >> m;
                std::vector<int32_t> ids(m), off(n + 1); std::vector<float> val(n);
                for (auto& x : ids) std::cin >> x;
                for (auto& x : off) std::cin >> x;
                for (auto& x : val) { uint32_t bits = 0; std::cin >> bits; memcpy(&x, &bits, 4); }
                t = dispatch_pack::bias_table(ids.data(), off.data(), val.data(), n);      // what a submit keeps
            }
            std::vector<const dispatch_pack::BiasTable*> ts;
            for (auto& t : own) ts.push_back(&t);
            const dispatch_pack::BiasBatch b = dispatch_pack::pack_bias(ts);               // what a prefill is told
            std::vector<uint32_t> bits(b.bias.size());
            if (!bits.empty()) memcpy(bits.data(), b.bias.data(), bits.size() * 4);
            line("seq_ids", b.seq_ids); line("seq_off", b.seq_off); line("bias", bits); line("req_off", b.req_off);
        } else if (kind == "draft") {                           // per request: n, n ids
            std::vector<std::vector<int32_t>> own(R);
            for (auto& d : own) { int n = 0; std::cin >> n; d.resize(n); for (auto& x : d) std::cin >> x; }
            std::vector<const std::vector<int32_t>*> ds;
            for (auto& d : own) ds.push_back(&d);
            line("words", dispatch_pack::pack_drafts(ds));
        } else if (kind == "offsets") {                         // R = W windows: W + 1 offsets, exactly that many allocated (a read past them is the sanitizer's to report)
            std::vector<int64_t> off(R + 1);
            for (auto& x : off) std::cin >> x;
            printf("ok %d\n", dispatch_pack::offsets_ok(off.data(), R) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
"""

# a request's table as its submit states it: (RequestBias or None, ids ahead of the table's own in seq_ids - the offsets then do not start at 0)
BIAS_BATCHES = {
    "three requests, the middle one without a table": [(RequestBias([[[5, 6], 1.5], [[7], -2.0]]), 0), (None, 0), (RequestBias(None, [[9, 10, 11]]), 0)],
    "offsets that do not start at 0": [(RequestBias([[[3], 0.25], [[4, 5, 6], 2.0]]), 3), (RequestBias([[[8, 9], -1.0]]), 1)],
    "two sequences of different length": [(RequestBias([[[1, 2, 3, 4, 5, 6, 7, 8], 3.0], [[2], 1e-3]]), 0)],
    "one request": [(RequestBias([[[12], 4.0]]), 0)],
}
DRAFT_BATCHES = {
    "three requests, the first and the last empty": [[], [5, 6, 7], []],
    "one request": [[41, 42]],
    "one request without a draft": [[]],
}


# a submit's host_off -> does the submit take it: 0 == off[0] <= off[1] <= ... <= off[W]
OFFSETS = {
    "monotone": ([0, 16000, 16000, 48000], True),
    "not starting at 0": ([1, 16000, 32000], False),
    "one decreasing step in the middle": ([0, 32000, 16000, 48000], False),
    "last entry below an earlier one": ([0, 16000, 32000, 8000], False),
    "one window": ([0, 16000], True),
    "one window, decreasing": ([0, -1], False),
    "one empty window (a ring slice)": ([0, 0], True),
}


def _words(v):
    return " ".join(str(int(x)) for x in v)


def _bias_input(batch):
    out = [f"bias {len(batch)}"]
    for table, ahead in batch:
        if table is None:
            out.append("0")
            continue
        ids, off, val = table.table()
        junk = np.arange(1000, 1000 + ahead, dtype=np.int32)
        out.append(f"{len(val)} {len(ids) + ahead} {_words(np.concatenate([junk, ids]))} {_words(off + ahead)} {_words(val.view(np.uint32))}")
    return "\n".join(out) + "\n"


def _bias_expected(batch):
    seq_ids, seq_off, bias, req_off = engine.pack_request_bias([t for t, _ in batch])
    assert seq_ids.dtype == seq_off.dtype == req_off.dtype == np.int32 and bias.dtype == np.float32
    return [f"seq_ids {_words(seq_ids)}".rstrip(), f"seq_off {_words(seq_off)}", f"bias {_words(bias.view(np.uint32))}".rstrip(), f"req_off {_words(req_off)}"]


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("dispatch_pack")
    src, exe = d / "pack_main.cpp", d / "pack_main"
    src.write_text(PROGRAM)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # (clang links the sanitizers' runtimes statically by itself)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                        "-I", os.path.join(ROOT, "sonicscribe_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(text):
        p = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-3000:])      # the sanitizers report nothing
        return [ln.rstrip() for ln in p.stdout.splitlines()]
    return run


@pytest.mark.parametrize("name", list(BIAS_BATCHES))
def test_bias_tables_word_for_word(packer, name):
    batch = BIAS_BATCHES[name]
    assert packer(_bias_input(batch)) == _bias_expected(batch)


@pytest.mark.parametrize("name", list(DRAFT_BATCHES))
def test_drafts_word_for_word(packer, name):
    batch = DRAFT_BATCHES[name]
    text = f"draft {len(batch)}\n" + "".join(f"{len(d)} {_words(d)}\n" for d in batch)
    assert packer(text) == [f"words {_words(engine.pack_request_draft(batch))}"]


def test_every_batch_in_one_run(packer):
    """the program's state does not leak from one batch into the next"""
    text = "".join(_bias_input(b) for b in BIAS_BATCHES.values())
    assert packer(text) == [ln for b in BIAS_BATCHES.values() for ln in _bias_expected(b)]


@pytest.mark.parametrize("name", list(OFFSETS))
def test_window_offsets(packer, name):
    off, ok = OFFSETS[name]
    assert packer(f"offsets {len(off) - 1}\n{_words(off)}\n") == [f"ok {int(ok)}"]
