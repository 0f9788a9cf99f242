"""sonic_dispatch_request (include/sonic_hip.h), the one record a dispatcher submit takes, against engine.DispatchRequest: a stand-alone C program with its own main,
compiled against the header alone, prints the struct's size and every field's offset and size; the ctypes class must say the same, field by field and in order.  And
the surface: one submit entry point, the record's value fields in the header, none of the names the record replaced.  Needs no library and no device."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import abi_pins
from sonicscribe_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("size", "host_pcm", "host_off", "rings", "ring_start", "ring_n", "W", "prompt_ids", "prompt_len", "max_new", "seq_ids", "seq_off", "bias", "n_seq",
          "sampled", "temperature", "seed", "cut", "top_k", "top_p", "min_p", "grammar_id", "draft_ids", "n_draft")

PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "sonic_hip.h"
#define FIELD(f) printf(#f " %zu %zu\n", offsetof(sonic_dispatch_request, f), sizeof(((sonic_dispatch_request*)0)->f))
int main(void) {
    printf("sizeof %zu\n", sizeof(sonic_dispatch_request));
""" + "".join(f"    FIELD({f});\n" for f in FIELDS) + r"""    return 0;
}
"""


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or ("/opt/rocm/llvm/bin/clang" if os.path.exists("/opt/rocm/llvm/bin/clang") else None)
    if cc is None:
        pytest.skip("no host C compiler")
    d = tmp_path_factory.mktemp("dispatch_request")
    src, exe = d / "layout_main.c", d / "layout_main"
    src.write_text(PROGRAM)
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]
    return [ln.split() for ln in p.stdout.splitlines()]


def test_the_binding_has_the_header_layout(layout):
    R = engine.DispatchRequest
    assert layout[0] == ["sizeof", str(C.sizeof(R))]
    assert [f for f, _ in R._fields_] == list(FIELDS)                                   # ... every field, in the header's order
    assert layout[1:] == [[f, str(getattr(R, f).offset), str(getattr(R, f).size)] for f in FIELDS]
    assert {f for f, t in R._fields_ if t is C.c_float} == {"temperature", "top_k", "top_p", "min_p"}      # (an offset and a size do not tell a float from an int32)


def test_a_fresh_record_is_none_but_its_size():
    r = engine.DispatchRequest()
    assert r.size == C.sizeof(engine.DispatchRequest)
    r.size = 0
    assert bytes(r) == bytes(C.sizeof(r))                                                # all-zero: no table, greedy, no cut, no grammar, no draft
    assert engine.DispatchRequest(W=2, max_new=7).W == 2


def test_one_entry_point_and_none_of_the_names_it_replaced():
    abi_pins.check_surface(names=("sonic_dispatch_submit",),
                           header_strings=("typedef struct sonic_dispatch_request {", "} sonic_dispatch_request;", "int64_t size;",
                                           "const int32_t* seq_ids; const int32_t* seq_off; const float* bias; int32_t n_seq;",
                                           "int32_t sampled; float temperature; uint64_t seed;", "int32_t cut; float top_k, top_p, min_p;", "int32_t grammar_id;",
                                           "const int32_t* draft_ids; int32_t n_draft;",
                                           "SONIC_API int sonic_dispatch_submit(sonic_dispatch* d, const sonic_dispatch_request* r, int64_t* ticket_out);"))
    hdr = abi_pins.header()
    for gone in [v + ".dispatch" for v in ("grammar", "draft", "truncation")] + ["sonic_dispatch_submit_" + tail for tail in ("bias", "sampled")]:
        assert gone not in hdr and not any(gone in n for n in engine.EXPORTS), gone
    assert [n for n in engine.EXPORTS if n.startswith("sonic_dispatch_submit")] == ["sonic_dispatch_submit"]
