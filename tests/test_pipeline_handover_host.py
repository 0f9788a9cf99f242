"""The bulk pipeline's hand-over order on the CPU, both drivers over stub engines that count calls (as the stubs of tests/test_dispatch.py do):
csrc/pipeline.cpp's native threads - compiled here with the host compiler against a stub of the engine calls it makes - and pipeline.py's
ContinuousPipeline.  A finished block's rows are in the handle's pinned mirror, so the decoder fetches them at once: between the service_step whose
check reports a block finished and that block's fetch there is no further service_step.  With option fetch_stream = 1 (the fetch is copy commands and a
wait, about a chunk's time) one more chunk goes out first whenever another block keeps running - exactly one.  Every ticket completes either way."""
import ctypes as C
import os
import shutil
import subprocess
import threading
import time

import numpy as np
import pytest

from sonicscribe_amd.pipeline import ContinuousPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sonicscribe_amd", "csrc")
BUDGETS = [21, 9, 13, 17, 11, 15, 7]                        # one per batch: blocks end in different chunks

# The engine calls csrc/pipeline.cpp makes (include/sonic_hip.h, csrc/sched_engine.h), on handles that only count: a decoding handle's rows gain two tokens
# per chunk; the log holds "S <handle> <seq>" per service_step, "R <handle> <row> <occupied blocks> <blocks this step reports finished>" the first time a
# step's check reports a row finished (behind its splice), "F <handle> <row>" per fetched row
STUB = r"""
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "sched_engine.h"
struct sonic_engine { int id = 0, fetch_stream = 0, block = 2; bool on = false; long long seq = 0; int budget[64] = {0}, have[64] = {0}; long long spliced[64] = {0};
                      bool occ[64] = {false}, reported[64] = {false}; std::vector<int> staged; std::mutex mu; };
static std::mutex g_mu; static std::string g_log; static int g_weights;
static void say(const char* f, long long a, long long b, long long c = 0, long long d = 0) { char s[96]; snprintf(s, sizeof s, f, a, b, c, d); std::lock_guard<std::mutex> l(g_mu); g_log += s; }
extern "C" {
SONIC_API sonic_engine* stub_new(int id, int fetch_stream, int block) { auto* e = new sonic_engine(); e->id = id; e->fetch_stream = fetch_stream; e->block = block; return e; }
SONIC_API void stub_free(sonic_engine* e) { delete e; }
SONIC_API int stub_log(char* out, int cap) { std::lock_guard<std::mutex> l(g_mu); snprintf(out, cap, "%s", g_log.c_str()); const int n = (int)g_log.size(); g_log.clear(); return n; }
int sonic_engine_info(sonic_engine* e, int32_t* mb, int32_t* mc, int32_t* mode, int32_t* dev, const void** wid) {
    if (mb) *mb = 64; if (mc) *mc = 512; if (mode) *mode = 0; if (dev) *dev = 0; if (wid) *wid = &g_weights; return e ? SONIC_OK : SONIC_ERR_INVALID; }
int engine_token_logprobs_on(sonic_engine*) { return 0; }
int engine_top_logprobs(sonic_engine*) { return 0; }
int engine_forced_parallel_on(sonic_engine*) { return 0; }
int engine_lm_on(sonic_engine*) { return 0; }
int engine_draft_verify_on(sonic_engine*) { return 0; }
int engine_fetch_stream_on(sonic_engine* e) { return e->fetch_stream; }
int engine_fail(sonic_engine*, int code, const char*) { return code; }
const char* sonic_last_error(sonic_engine*) { return "stub"; }
int sonic_service_begin(sonic_engine* e) { e->on = true; return SONIC_OK; }
int sonic_service_end(sonic_engine* e) { e->on = false; return SONIC_OK; }
int sonic_stage_pcm(sonic_engine*, const int16_t*, const int64_t*, int) { return SONIC_OK; }
int sonic_stage_mixed(sonic_engine*, const int16_t*, const int64_t*, sonic_ring* const*, const int64_t*, const int32_t*, int, const int32_t*, int) { return SONIC_OK; }
int sonic_prefill_enqueue(sonic_engine* e, const int32_t*, int R, const int32_t*, const int64_t*, const int32_t* max_new) {
    std::lock_guard<std::mutex> l(e->mu); e->staged.assign(max_new, max_new + R); return SONIC_OK; }
int sonic_splice_rows(sonic_engine* d, sonic_engine* p, int n, const int32_t* src, const int32_t* dst, int64_t* seq_out) {
    std::lock_guard<std::mutex> l(d->mu); std::lock_guard<std::mutex> l2(p->mu);
    for (int i = 0; i < n; ++i) { const int r = dst[i]; if (d->occ[r]) return SONIC_ERR_INVALID; d->occ[r] = true; d->reported[r] = false; d->budget[r] = p->staged[src[i]]; d->have[r] = 1; d->spliced[r] = d->seq; }
    if (seq_out) *seq_out = d->seq; return SONIC_OK; }
int sonic_service_step(sonic_engine* e, int n_chunks, int rows, int32_t* fin, int32_t* nn, int64_t* seq_out, int32_t* nact) {
    std::this_thread::sleep_for(std::chrono::microseconds(300));
    std::lock_guard<std::mutex> l(e->mu);
    e->seq += n_chunks; say("S %lld %lld\n", e->id, e->seq);
    int act = 0, nocc = 0, ndone = 0;
    for (int r = 0; r < 64; ++r) {
        if (e->occ[r]) { if (r >= rows && rows > 0) return SONIC_ERR_INVALID; e->have[r] = e->have[r] + 2 * n_chunks < e->budget[r] ? e->have[r] + 2 * n_chunks : e->budget[r]; }
        fin[r] = !e->occ[r] || e->have[r] >= e->budget[r]; nn[r] = e->occ[r] ? e->have[r] : 0; act += !fin[r];
    }
    for (int b = 0; b < 64 / e->block; ++b) { const int r = b * e->block; if (e->occ[r]) { ++nocc; if (fin[r] && !e->reported[r] && e->seq > e->spliced[r]) ++ndone; } }
    for (int r = 0; r < 64; ++r) if (e->occ[r] && fin[r] && !e->reported[r] && e->seq > e->spliced[r]) { e->reported[r] = true; say("R %lld %lld %lld %lld\n", e->id, r, nocc, ndone); }
    if (seq_out) *seq_out = e->seq; if (nact) *nact = act; return SONIC_OK; }
int sonic_fetch_rows(sonic_engine* e, int n, const int32_t* rows, const int32_t* counts, int32_t* out, int ld) {
    std::lock_guard<std::mutex> l(e->mu);
    for (int i = 0; i < n; ++i) { const int r = rows[i]; if (!e->occ[r] || e->have[r] < e->budget[r] || counts[i] != e->budget[r]) return SONIC_ERR_INVALID;
                                  for (int j = 0; j < counts[i]; ++j) out[(size_t)i * ld + j] = e->budget[r] * 100 + j; e->occ[r] = false; say("F %lld %lld\n", e->id, r); }
    return SONIC_OK; }
int sonic_fetch_rows_lp(sonic_engine* e, int n, const int32_t* rows, const int32_t* counts, int32_t* out, int ld, float*) { return sonic_fetch_rows(e, n, rows, counts, out, ld); }
}
"""


def extra_steps(log, fetch_stream):
    """the log -> for every fetched row, the service_steps of its handle between the step that reported it finished and its fetch, checked against what the
    order promises; returns how many rows left while another block kept running"""
    steps_since, beside, ahead = {}, 0, {}
    for line in log.strip().splitlines():
        w = line.split()
        h = int(w[1])
        if w[0] == "S":
            ahead[h] = any(k[0] == h for k in steps_since)      # a step with a finished block unfetched: the chunk fetch_stream = 1 queues ahead of the fetch
            assert fetch_stream or not ahead[h], line
            for k in steps_since:
                if k[0] == h:
                    steps_since[k][0] += 1
        elif w[0] == "R":
            steps_since[(h, int(w[2]))] = [0, int(w[3]), int(w[4]), ahead[h]]
        else:
            n, nocc, ndone, late = steps_since.pop((h, int(w[2])))
            if late:        # reported by the chunk that went out ahead of another block's fetch: the decoder looks at the next step's check, and the rule starts there
                assert fetch_stream and n in (1, 2), (line, n)
                continue
            assert n == (1 if fetch_stream and ndone < nocc else 0), (line, n, nocc, ndone)
            beside += ndone < nocc
    assert not steps_since
    return beside


# ------------------------------------------------------------------------------------------ csrc/pipeline.cpp
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    d = tmp_path_factory.mktemp("pipe_stub")
    src, so = os.path.join(d, "stub_engine.cpp"), os.path.join(d, "libpipe_stub.so")
    with open(src, "w") as f:
        f.write(STUB)
    subprocess.run([cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-I", CSRC, "-x", "c++", os.path.join(CSRC, "pipeline.cpp"), src, "-o", so],
                   check=True, capture_output=True, text=True, timeout=300)
    lib = C.CDLL(so)
    lib.stub_new.restype = C.c_void_p
    lib.stub_new.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.stub_free.argtypes = [C.c_void_p]
    lib.sonic_pipeline_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.sonic_pipeline_submit.argtypes = [C.c_void_p] + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    lib.sonic_pipeline_wait.argtypes = [C.c_void_p, C.c_int64]
    lib.sonic_pipeline_destroy.argtypes = [C.c_void_p]
    return lib


@pytest.mark.parametrize("fetch_stream", [0, 1])
def test_native_decode_thread_fetches_before_the_next_chunk(native, fetch_stream):
    lib, block = native, 2
    dec, pre = lib.stub_new(1, fetch_stream, block), lib.stub_new(2, fetch_stream, block)
    pipe = C.c_void_p()
    assert lib.sonic_pipeline_create((C.c_void_p * 1)(dec), 1, (C.c_void_p * 1)(pre), 1, block, 2 * block, C.byref(pipe)) == 0      # one decoder, two blocks
    keep, tickets = [], []
    for b in BUDGETS:
        ids, off, mn = np.array([1, 2, 3, 4], np.int32), np.array([0, 2, 4], np.int64), np.array([b] * block, np.int32)
        out, out_len, t = np.zeros((block, b), np.int32), np.zeros(block, np.int32), C.c_int64(0)
        assert lib.sonic_pipeline_submit(pipe, None, None, 0, None, block, ids.ctypes.data, off.ctypes.data, mn.ctypes.data, out.ctypes.data, b, out_len.ctypes.data, C.byref(t)) == 0
        keep.append((ids, off, mn, out, out_len)); tickets.append(t.value)
    for t, b, k in zip(tickets, BUDGETS, keep):                  # every ticket completes, every row with its own tokens
        assert lib.sonic_pipeline_wait(pipe, t) == 0
        assert list(k[4]) == [b] * block and np.array_equal(k[3], np.tile(b * 100 + np.arange(b, dtype=np.int32), (block, 1)))
    lib.sonic_pipeline_destroy(pipe)
    buf = C.create_string_buffer(1 << 20)
    lib.stub_log(buf, len(buf))
    log = buf.value.decode()
    assert log.count("F ") == block * len(BUDGETS)
    assert extra_steps(log, fetch_stream) >= block               # ... and some of them beside a block that kept running
    lib.stub_free(dec); lib.stub_free(pre)


# ------------------------------------------------------------------------------------------ pipeline.py ContinuousPipeline
class Handle:
    def __init__(self, hid, log, block=2):
        self.hid, self.log, self.block, self.max_batch = hid, log, block, 2 * block
        self.rows, self.seq, self.staged, self.on = {}, 0, None, False

    def service_begin(self):
        self.on = True

    def service_end(self):
        self.on = False

    def prefill(self, budgets):
        self.staged = list(budgets)

    def splice_rows(self, src, src_rows, dst_rows):
        for s, d in zip(src_rows, dst_rows):
            assert d not in self.rows
            self.rows[d] = [src.staged[s], 1, self.seq, False]      # budget, tokens, spliced at, reported
        return self.seq

    def service_step(self, n_chunks=1, rows=0):
        time.sleep(0.0005)                                          # (a chunk takes the device a while: the prefiller's next hand-over is there by the next one)
        self.seq += n_chunks
        fin, nn = np.ones(64, np.int32), np.zeros(64, np.int32)
        with self.log[0]:
            self.log[1].append(f"S {self.hid} {self.seq}")
            for r, st in self.rows.items():
                assert r < rows
                st[1] = min(st[0], st[1] + 2 * n_chunks)
                fin[r], nn[r] = st[1] >= st[0], st[1]
            new = [r for r, st in self.rows.items() if fin[r] and not st[3] and self.seq > st[2]]
            nocc, ndone = len({r // self.block for r in self.rows}), len({r // self.block for r in new})
            for r in new:
                self.rows[r][3] = True
                self.log[1].append(f"R {self.hid} {r} {nocc} {ndone}")
        return fin, nn, self.seq, int((fin == 0).sum())

    def fetch_rows(self, rows, counts):
        out = []
        with self.log[0]:
            for r, n in zip(rows, counts):
                budget = self.rows.pop(r)[0]
                assert n == budget
                out.append(budget * 100 + np.arange(n, dtype=np.int32))
                self.log[1].append(f"F {self.hid} {r}")
        return out


@pytest.mark.parametrize("fetch_stream", [False, True])
def test_python_decoder_fetches_before_the_next_chunk(fetch_stream):
    log = (threading.Lock(), [])
    dec, pre = Handle(1, log), Handle(2, log)
    pipe = ContinuousPipeline([dec], [pre], block=2, fetch_stream=fetch_stream)
    todo, lock = list(BUDGETS), threading.Lock()

    def prefill(p):
        with lock:
            b = todo.pop(0)
        p.prefill([b, b])
        return b

    res = pipe.run(len(BUDGETS), prefill, lambda i, ids, b: np.array_equal(ids, b * 100 + np.arange(b)))
    pipe.close()
    assert res["batches"] == len(BUDGETS) and res["wrong_rows"] == 0 and not dec.rows and not dec.on
    assert extra_steps("\n".join(log[1]), fetch_stream) >= 2
