// sonic_dispatch_*: the request-level scheduler for live traffic as native threads.
//
// What it replaces: sonicscribe_amd/dispatch.py _ContinuousReplica - Python threads over ctypes that prefill whatever is queued, splice the rows into
// a continuously decoding handle, step it chunk by chunk and fetch rows as they finish.  The arithmetic was never in Python, but every decode chunk
// of every loop went through the interpreter (a numpy record, list comprehensions, a condition variable under the GIL) beside the sessions' own
// Python work.  The call sites this serves in the reference: one `await transcribe()` per partial / final of every WebSocket session on the event
// loop (backend/connection_manager.py:127-245, backend/transcription_manager.py:19-65) and three executor threads in file mode
// (backend/main.py:429-445, 616-624) - all serialised on one model object there.
//
// Same schedule as the Python class (whose CPU tests keep describing it, tests/test_dispatch.py):
//   * submit() queues a request (W windows: host PCM or slices of device rings, a prompt, a budget) and returns a ticket;
//   * one thread per PREFILL handle: takes the oldest requests that fit - as many as the emptiest decoder has free rows and the handle has windows,
//     step classes mix - stages them (sonic_stage_mixed), runs log-mel + encoder + prompt forward + first token (sonic_prefill, waited for: a splice
//     queued behind a running prefill would hold the decoder's stream) and hands the batch over; a request that fails validation fails alone
//     (the batch is retried one request at a time);
//   * one thread per DECODING handle: splices handed-over rows into its lowest free rows between two chunks, queues chunks over the occupied
//     rows (sonic_service_step), fetches every row the moment the pipelined check shows it finished (sonic_fetch_rows) and completes its ticket;
//   * completions are collected by sonic_dispatch_next (blocking, from any thread): the host side keeps one thread that turns them into futures.
// No thread polls: condition variables here, blocking HIP events inside the engine.  Only the C ABI of include/sonic_hip.h is used, plus what sched_engine.h
// lists of the library's own (is an option on for a handle, a request's values checked and taken at its submit).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "dispatch_pack.h"
#include "sched_engine.h"

namespace {

// What a request may bring of its own, in the order of VALUES below
struct ReqValues {
    dispatch_pack::BiasTable bias;                                 // its sequence-bias table (the record's seq_ids .. n_seq; empty: none)
    bool sampled = false; float temperature = 0.f; uint64_t seed = 0;   // its (temperature, seed); unsampled requests of a batch are greedy
    bool cut = false; float trunc[3] = {0.f, 1.f, 0.f};            // ... and its (top_k, top_p, min_p) (option truncation): they ride on the sampling values
    sonic_grammar* gram = nullptr;                                 // its grammar (grammar_id): a reference held from the submit until the request completes
    std::vector<int32_t> draft;                                    // its draft (option draft_verify): the prefill verifies it
};

struct Req {
    int64_t ticket = 0;
    int W = 0;
    std::vector<int16_t> pcm; std::vector<int64_t> off;            // host windows (ring windows: empty ranges)
    std::vector<sonic_ring*> rings; std::vector<int64_t> ring_start; std::vector<int32_t> ring_n; bool any_ring = false;
    std::vector<int32_t> prompt; int max_new = 0;
    int status = -1; std::string err; std::vector<int32_t> ids;    // result
    std::vector<float> lp;                                         // ... and, with option token_logprobs on the handles, every token's log-probability
    ReqValues own;                                                 // what it brings of its own
    bool cancelled = false;
};
typedef std::shared_ptr<Req> ReqP;
struct Handover { std::vector<ReqP> reqs; sonic_engine* src = nullptr; bool taken = false; };

}   // namespace

struct sonic_dispatch {
    std::vector<sonic_engine*> dec, pre;
    int n_rows = 0, pre_cap = 0;
    bool adaptive_tiles = true;
    bool lp = false;                                               // every handle has option token_logprobs on
    int lp_w = 1;                                                  // ... and their records hold this many floats per token (1 + 2K, option top_logprobs: equal on all)
    bool bias = false;                                             // every handle has option request_bias on
    bool samp = false;                                             // every handle has option sampling on
    bool trunc = false;                                            // every handle has option truncation on
    bool gram = false;                                             // every handle has option grammar on
    bool draft = false; int tok_cap = 0;                           // every handle has option draft_verify on; then a batch's prompts and drafts are counted against tok_cap
    std::mutex mu;
    std::condition_variable cv;                                    // queue, hand-overs, free rows, state
    std::condition_variable cv_done;                               // completions
    std::deque<ReqP> q;
    std::vector<int> free_rows;                                    // per decoder: rows neither occupied nor reserved by a prefill in flight
    std::vector<std::deque<std::shared_ptr<Handover>>> hand;
    std::deque<ReqP> done;
    int64_t next_ticket = 1, batches = 0, chunks = 0, outstanding = 0;   // outstanding: submitted and not yet collected by sonic_dispatch_next
    int queued_windows = 0;
    bool stop = false;
    int failed = 0; std::string fail_msg;
    std::vector<std::thread> threads;
};

namespace {

void finish(sonic_dispatch* d, const ReqP& r, int status, const std::string& err) {   // d->mu held
    if (r->status != -1) return;
    if (r->own.gram) { engine_grammar_unref(r->own.gram); r->own.gram = nullptr; }      // (its row was fetched - and let go of its own reference - or it never reached one)
    r->status = status; r->err = err;
    d->done.push_back(r);
    d->cv_done.notify_all();
}

// The per-request values, in the order every site arms them: bias, sampling, grammar, draft.  sonicscribe_amd/reqvalues.py (VALUES) is this list's Python twin; a
// further value is one entry here, its fields in ReqValues and its way into a submit.  brings: does this request bring the value; arm: the batch's values (row i
// is batch[i]; a request without one: an empty table, greedy, NULL, an empty draft) in the form handle h takes them for its next prefill.  prefill_batch arms a value
// only when some request of the batch brings it, where the Python replica (reqvalues.arm) states every value whose option is on ahead of every prefill: a
// difference kept as it is (a consuming call of the engine drops what was staged on every way out, so an unarmed batch starts without values).
struct Value {
    bool (*brings)(const ReqValues&);
    int (*arm)(sonic_engine* h, const std::vector<ReqP>& batch);
};
const Value VALUES[] = {
    {[](const ReqValues& v) { return !v.bias.val.empty(); },
     [](sonic_engine* h, const std::vector<ReqP>& batch) {
         std::vector<const dispatch_pack::BiasTable*> ts;
         for (auto& r : batch) ts.push_back(&r->own.bias);
         const dispatch_pack::BiasBatch b = dispatch_pack::pack_bias(ts);
         return sonic_set_request_bias(h, b.seq_ids.data(), b.seq_off.data(), b.bias.data(), b.req_off.data(), (int)batch.size());
     }},
    {[](const ReqValues& v) { return v.sampled; },
     [](sonic_engine* h, const std::vector<ReqP>& batch) {
         std::vector<float> t; std::vector<uint64_t> sd;
         for (auto& r : batch) { t.push_back(r->own.sampled ? r->own.temperature : 0.f); sd.push_back(r->own.sampled ? r->own.seed : 0); }
         const int rc = sonic_set_request_sampling(h, t.data(), sd.data(), (int)batch.size());
         bool any = false;
         for (auto& r : batch) any = any || r->own.cut;
         if (rc != SONIC_OK || !any) return rc;
         std::vector<float> rows;                                   // a batch in which some request cuts its tail: every row's three values, off for the others
         for (auto& r : batch) { const float off[3] = {0.f, 1.f, 0.f}; const float* v = r->own.cut ? r->own.trunc : off; rows.insert(rows.end(), v, v + 3); }
         const int64_t shape[2] = {(int64_t)batch.size(), 3};
         return sonic_load_tensor(h, "request_truncation", rows.data(), SONIC_DTYPE_F32, shape, 2);
     }},
    {[](const ReqValues& v) { return v.gram != nullptr; },
     [](sonic_engine* h, const std::vector<ReqP>& batch) {
         std::vector<sonic_grammar*> gs;
         for (auto& r : batch) gs.push_back(r->own.gram);
         return engine_set_request_grammar(h, gs.data(), (int)batch.size());
     }},
    {[](const ReqValues& v) { return !v.draft.empty(); },
     [](sonic_engine* h, const std::vector<ReqP>& batch) {
         std::vector<const std::vector<int32_t>*> ds;
         for (auto& r : batch) ds.push_back(&r->own.draft);
         const std::vector<int32_t> w = dispatch_pack::pack_drafts(ds);
         const int64_t n = (int64_t)w.size();
         return sonic_load_tensor(h, "request_draft", w.data(), SONIC_DTYPE_I32, &n, 1);
     }},
};

// stage + prefill `batch` on handle h; SONIC_OK or the failing status (message in *err)
int prefill_batch(sonic_dispatch* d, sonic_engine* h, const std::vector<ReqP>& batch, bool busy, std::string* err) {
    std::vector<int16_t> pcm; std::vector<int64_t> off{0}; std::vector<sonic_ring*> rings; std::vector<int64_t> rstart; std::vector<int32_t> rn;
    std::vector<int32_t> req_win{0}, ids, mn; std::vector<int64_t> poff{0};
    bool any_ring = false;
    for (auto& r : batch) {
        for (int w = 0; w < r->W; ++w) {
            const int64_t a = r->off[w], b = r->off[w + 1];
            pcm.insert(pcm.end(), r->pcm.begin() + a, r->pcm.begin() + b);
            off.push_back((int64_t)pcm.size());
            rings.push_back(r->any_ring ? r->rings[w] : nullptr); rstart.push_back(r->any_ring ? r->ring_start[w] : 0); rn.push_back(r->any_ring ? r->ring_n[w] : 0);
            any_ring = any_ring || (r->any_ring && r->rings[w]);
        }
        req_win.push_back((int32_t)(off.size() - 1));
        ids.insert(ids.end(), r->prompt.begin(), r->prompt.end());
        poff.push_back((int64_t)ids.size());
        mn.push_back(r->max_new);
    }
    if (pcm.empty()) pcm.push_back(0);
    const int W = (int)off.size() - 1, R = (int)batch.size();
    // A prefill beside RUNNING rows keeps the big GEMM tiles even where they under-fill the chip: the idle CUs are where the decode loops' kernels
    // run meanwhile (profiles/round4_streaming_ab.txt).  The tile choice never changes a result's bits.
    if (d->adaptive_tiles) (void)sonic_set_option(h, "gemm_small_eff", busy ? 0 : 75);
    int rc = any_ring ? sonic_stage_mixed(h, pcm.data(), off.data(), rings.data(), rstart.data(), rn.data(), W, req_win.data(), R)
                      : sonic_stage_pcm(h, pcm.data(), off.data(), W);
    for (const Value& v : VALUES) {                                // the requests' own values; the prefill below consumes them
        if (rc != SONIC_OK) break;
        if (std::any_of(batch.begin(), batch.end(), [&](const ReqP& r) { return v.brings(r->own); })) rc = v.arm(h, batch);
    }
    if (rc == SONIC_OK) rc = sonic_prefill(h, req_win.data(), R, ids.data(), poff.data(), mn.data(), 0);
    if (rc != SONIC_OK && err) *err = sonic_last_error(h);
    return rc;
}

void release_rows(sonic_dispatch* d, int k, int n) {             // d->mu held
    d->free_rows[k] += n;
    d->cv.notify_all();
}

// hands a prefilled batch to decoder k and waits until its rows have been spliced (they are the splice's source until then)
void hand_over(sonic_dispatch* d, sonic_engine* h, std::vector<ReqP> batch, int k, std::unique_lock<std::mutex>& lk) {
    auto ho = std::make_shared<Handover>(); ho->reqs = std::move(batch); ho->src = h;
    d->hand[k].push_back(ho);
    d->cv.notify_all();
    d->cv.wait(lk, [&] { return ho->taken || d->failed; });
    if (!ho->taken) {                                              // the decode side died with this batch in hand: fail it here, exactly once
        auto& v = d->hand[k];
        auto it = std::find(v.begin(), v.end(), ho);
        if (it != v.end()) {
            v.erase(it);
            for (auto& r : ho->reqs) finish(d, r, d->failed, d->fail_msg);
            release_rows(d, k, (int)ho->reqs.size());
        }
    }
}

void prefill_thread(sonic_dispatch* d, sonic_engine* h) {
    const int nd = (int)d->dec.size();
    for (;;) {
        std::vector<ReqP> batch; int k = 0; bool busy = false;
        {
            std::unique_lock<std::mutex> lk(d->mu);
            d->cv.wait(lk, [&] { return d->stop || d->failed || (!d->q.empty() && *std::max_element(d->free_rows.begin(), d->free_rows.end()) > 0); });
            if (d->stop || d->failed) return;                      // closing / failed: nothing new is started (destroy / the decode side fails what is queued)
            k = (int)(std::max_element(d->free_rows.begin(), d->free_rows.end()) - d->free_rows.begin());   // the emptiest decoder takes the whole batch
            int used = 0; long toks = 0;
            while (!d->q.empty()) {                                // oldest first, whatever fits the handle's windows and the free rows; classes mix
                ReqP r = d->q.front();
                if (r->cancelled) { d->q.pop_front(); d->queued_windows -= r->W; finish(d, r, SONIC_ERR_INVALID, "cancelled"); continue; }
                if (r->W > d->pre_cap) {
                    d->q.pop_front(); d->queued_windows -= r->W;
                    char m[128]; snprintf(m, sizeof m, "audio spans %d windows, engine max_batch is %d", r->W, d->pre_cap);
                    finish(d, r, SONIC_ERR_INVALID, m);
                    continue;
                }
                if ((int)batch.size() >= d->free_rows[k] || used + r->W > d->pre_cap) break;
                const long rt = (long)r->prompt.size() + (long)r->own.draft.size();
                if (d->draft && !batch.empty() && toks + rt > d->tok_cap) break;      // option draft_verify: prompts and drafts together fit one prefill (a request that alone does not is refused by it, by name)
                d->q.pop_front(); d->queued_windows -= r->W;
                batch.push_back(r); used += r->W; toks += rt;
            }
            if (batch.empty()) continue;
            d->free_rows[k] -= (int)batch.size();                  // reserved until the rows are fetched (or the prefill fails)
            ++d->batches;
            int running = 0; for (int j = 0; j < nd; ++j) running += d->n_rows - d->free_rows[j];
            busy = running > (int)batch.size();                    // rows running or reserved besides this batch's own
        }
        std::string err;
        int rc = prefill_batch(d, h, batch, busy, &err);
        std::unique_lock<std::mutex> lk(d->mu);
        if (rc == SONIC_OK) { hand_over(d, h, std::move(batch), k, lk); continue; }
        if (batch.size() == 1) { finish(d, batch[0], rc, err); release_rows(d, k, 1); continue; }
        // a per-request validation error must not poison its neighbours: one by one
        for (auto& r : batch) {
            lk.unlock();
            std::string e1;
            const int rc1 = prefill_batch(d, h, std::vector<ReqP>{r}, busy, &e1);
            lk.lock();
            if (rc1 != SONIC_OK) { finish(d, r, rc1, e1); release_rows(d, k, 1); }
            else hand_over(d, h, std::vector<ReqP>{r}, k, lk);
        }
    }
}

void decode_thread(sonic_dispatch* d, int k) {
    sonic_engine* e = d->dec[k];
    const int n_rows = d->n_rows;
    std::vector<ReqP> rows(n_rows);
    std::vector<int64_t> valid_after(n_rows, 0);
    int occupied = 0;
    int32_t fin[64], nn[64];
    auto fail_all = [&](int rc) {                                  // the engine failed: nothing queued or in flight on this loop can complete
        std::unique_lock<std::mutex> lk(d->mu);
        if (!d->failed) { d->failed = rc ? rc : SONIC_ERR_HIP; d->fail_msg = sonic_last_error(e); }
        for (auto& r : rows) if (r) { finish(d, r, d->failed, d->fail_msg); r.reset(); }
        for (auto& ho : d->hand[k]) { for (auto& r : ho->reqs) finish(d, r, d->failed, d->fail_msg); ho->taken = true; }
        d->hand[k].clear();
        while (!d->q.empty()) { finish(d, d->q.front(), d->failed, d->fail_msg); d->q.pop_front(); }
        d->queued_windows = 0;
        d->cv.notify_all();
    };
    for (;;) {
        std::vector<std::shared_ptr<Handover>> hs;
        {
            std::unique_lock<std::mutex> lk(d->mu);
            // idle = no row occupied and none reserved by a prefill in flight (free_rows counts both): a closing dispatcher keeps its decode loops
            // until every prefill that has taken rows has handed them over and they are fetched
            d->cv.wait(lk, [&] { return !d->hand[k].empty() || occupied > 0 || d->failed || (d->stop && d->free_rows[k] == n_rows); });
            if (d->failed) { lk.unlock(); fail_all(d->failed); return; }
            hs.assign(d->hand[k].begin(), d->hand[k].end()); d->hand[k].clear();
            if (d->stop && hs.empty() && occupied == 0 && d->free_rows[k] == n_rows) return;
        }
        for (auto& ho : hs) {
            const int n = (int)ho->reqs.size();
            std::vector<int32_t> src(n), dst;
            for (int i = 0; i < n_rows && (int)dst.size() < n; ++i) if (!rows[i]) dst.push_back(i);      // lowest free rows: a light load stays in the first 16
            for (int i = 0; i < n; ++i) src[i] = i;
            int64_t seq = 0;
            const int rc = (int)dst.size() == n ? sonic_splice_rows(e, ho->src, n, src.data(), dst.data(), &seq) : SONIC_ERR_INVALID;
            if (rc != SONIC_OK) {
                { std::unique_lock<std::mutex> lk(d->mu); d->hand[k].push_front(ho); }
                fail_all(rc); return;
            }
            for (int i = 0; i < n; ++i) { rows[dst[i]] = ho->reqs[i]; valid_after[dst[i]] = seq; }
            occupied += n;
            std::unique_lock<std::mutex> lk(d->mu);
            ho->taken = true;
            d->cv.notify_all();
        }
        if (occupied == 0) continue;
        int top = 0;
        for (int i = 0; i < n_rows; ++i) if (rows[i]) top = i + 1;
        int64_t seq = 0; int32_t nact = 0;
        int rc = sonic_service_step(e, 1, top, fin, nn, &seq, &nact);
        if (rc != SONIC_OK) { fail_all(rc); return; }
        std::vector<int32_t> dr, dc;
        for (int i = 0; i < n_rows; ++i) if (rows[i] && seq > valid_after[i] && fin[i]) { dr.push_back(i); dc.push_back(nn[i]); }
        int ld = 1; for (int c : dc) ld = c > ld ? c : ld;
        std::vector<int32_t> out; std::vector<float> olp;
        if (!dr.empty()) {                                         // one call for all of them: one wait, one release launch
            out.assign((size_t)dr.size() * ld, 0);
            if (d->lp) olp.assign((size_t)dr.size() * ld * d->lp_w, 0.f);
            rc = d->lp ? sonic_fetch_rows_lp(e, (int)dr.size(), dr.data(), dc.data(), out.data(), ld, olp.data())
                       : sonic_fetch_rows(e, (int)dr.size(), dr.data(), dc.data(), out.data(), ld);
            if (rc != SONIC_OK) { fail_all(rc); return; }
        }
        std::unique_lock<std::mutex> lk(d->mu);
        ++d->chunks;
        for (size_t j = 0; j < dr.size(); ++j) {
            ReqP r = rows[dr[j]]; rows[dr[j]].reset(); --occupied;
            r->ids.assign(out.begin() + j * ld, out.begin() + j * ld + dc[j]);
            if (d->lp) r->lp.assign(olp.begin() + j * ld * d->lp_w, olp.begin() + (j * ld + dc[j]) * d->lp_w);
            finish(d, r, SONIC_OK, "");
        }
        if (!dr.empty()) release_rows(d, k, (int)dr.size());
    }
}

}   // namespace

extern "C" {

SONIC_API int sonic_dispatch_create(sonic_engine* const* decoders, int n_dec, sonic_engine* const* prefills, int n_pre, int adaptive_tiles, sonic_dispatch** out) {
    if (!out) return SONIC_ERR_INVALID;
    *out = nullptr;
    if (!decoders || !prefills || n_dec < 1 || n_pre < 1) return SONIC_ERR_INVALID;
    sched_handles hs(decoders, n_dec, prefills, n_pre);
    if (!hs.check()) return SONIC_ERR_INVALID;
    const int32_t rows = *std::min_element(hs.max_batch.begin(), hs.max_batch.begin() + n_dec), cap = *std::min_element(hs.max_batch.begin() + n_dec, hs.max_batch.end());
    if (rows < 1 || rows > 64 || cap < 1) return SONIC_ERR_INVALID;
    const int K = engine_top_logprobs(decoders[0]);             // (a splice between handles of different K would be refused row by row: refuse the set)
    if (!hs.every([K](sonic_engine* h) { return engine_top_logprobs(h) == K; }))
        return engine_thread_fail(SONIC_ERR_INVALID, "sonic_dispatch_create: the handles differ in option top_logprobs (set it on the owner before its slots are created)");
    if (hs.any(engine_forced_parallel_on))
        return engine_thread_fail(SONIC_ERR_INVALID, "sonic_dispatch_create: option forced_parallel is on on a handle: a scoring handle takes no part in the dispatcher");
    sonic_dispatch* d = new sonic_dispatch();
    d->dec.assign(decoders, decoders + n_dec); d->pre.assign(prefills, prefills + n_pre);
    d->n_rows = rows; d->pre_cap = cap; d->adaptive_tiles = adaptive_tiles != 0;
    d->lp = hs.every(engine_token_logprobs_on);
    d->lp_w = d->lp ? 1 + 2 * K : 1;
    d->bias = hs.every(engine_request_bias_on);
    d->samp = hs.every(engine_sampling_on);
    d->trunc = hs.every(engine_truncation_on);
    d->gram = hs.every(engine_grammar_on);
    d->draft = hs.every(engine_draft_verify_on);
    d->tok_cap = engine_tok_cap(prefills[0]);
    for (sonic_engine* h : d->pre) d->tok_cap = std::min(d->tok_cap, engine_tok_cap(h));
    d->free_rows.assign(n_dec, rows); d->hand.resize(n_dec);
    for (int i = 0; i < n_dec; ++i) {
        const int rc = sonic_service_begin(d->dec[i]);
        if (rc != SONIC_OK) { for (int j = 0; j < i; ++j) (void)sonic_service_end(d->dec[j]); delete d; return rc; }
    }
    for (int i = 0; i < n_dec; ++i) d->threads.emplace_back(decode_thread, d, i);
    for (int i = 0; i < n_pre; ++i) d->threads.emplace_back(prefill_thread, d, d->pre[i]);
    *out = d;
    return SONIC_OK;
}

// the refusal of a value (named by `who`, the lead-in of every refusal of it) whose option is not on on every handle
static int option_off(const char* who, const char* option) {
    char m[256]; snprintf(m, sizeof m, "%s: option %s is off on a handle of this dispatcher (set it on the owner before its slots are created)", who, option);
    return engine_thread_fail(SONIC_ERR_INVALID, m);
}

// One request (include/sonic_hip.h sonic_dispatch_request), checked in ONE order and then queued; a refusal leaves nothing behind, here or on the calling thread:
//   1. NULL pointers and the record's size;
//   2. the audio and the prompt;
//   3. the values it brings, in the order of VALUES: bias, sampling with its cut, grammar, draft - for each, that its option is on on every handle, then its validity
//      (the message starts with the value's name: request_bias, sampling, truncation, grammar, draft);
//   4. under the lock: closed, failed, and the request joins the queue.
// Everything is copied before the call returns.
SONIC_API int sonic_dispatch_submit(sonic_dispatch* d, const sonic_dispatch_request* q, int64_t* ticket_out) {
    if (!d || !q || !ticket_out) return SONIC_ERR_INVALID;
    if (q->size != (int64_t)sizeof *q) {
        char m[160]; snprintf(m, sizeof m, "sonic_dispatch_submit: sonic_dispatch_request.size is %lld, this library's record has %zu bytes", (long long)q->size, sizeof *q);
        return engine_thread_fail(SONIC_ERR_INVALID, m);
    }
    const int W = q->W;
    if (W < 1 || !q->prompt_ids || q->prompt_len < 1 || q->max_new < 1 || !q->host_off) return SONIC_ERR_INVALID;
    if (q->rings && (!q->ring_start || !q->ring_n)) return SONIC_ERR_INVALID;
    if (!dispatch_pack::offsets_ok(q->host_off, W) || (q->host_off[W] > 0 && !q->host_pcm)) return SONIC_ERR_INVALID;
    ReqValues own;
    struct Held { sonic_grammar* g; ~Held() { if (g) engine_grammar_unref(g); } } held{nullptr};      // the grammar's reference, until the request is queued
    if (q->n_seq < 0 || (q->n_seq > 0 && (!q->seq_ids || !q->seq_off || !q->bias))) return SONIC_ERR_INVALID;
    if (q->n_seq > 0) {
        if (!d->bias) return option_off("request_bias", "request_bias");
        const int rc = engine_bias_validate(d->pre[0], q->seq_ids, q->seq_off, q->bias, q->n_seq);
        if (rc != SONIC_OK) return rc;
        own.bias = dispatch_pack::bias_table(q->seq_ids, q->seq_off, q->bias, q->n_seq);
    }
    if (q->sampled) {
        if (!d->samp) return option_off("sampling", "sampling");
        const int rc = engine_sampling_validate(q->temperature);
        if (rc != SONIC_OK) return rc;
        own.sampled = true; own.temperature = q->temperature; own.seed = q->seed;
    }
    if (q->cut) {
        if (!d->trunc) return option_off("truncation", "truncation");
        if (!q->sampled) return engine_thread_fail(SONIC_ERR_INVALID, "truncation: the request is not sampled (top_k / top_p / min_p cut what a sampling request draws from)");
        const float row[3] = {q->top_k, q->top_p, q->min_p};
        const int rc = engine_truncation_validate(row);
        if (rc != SONIC_OK) return rc;
        own.cut = true; memcpy(own.trunc, row, sizeof row);
    }
    if (q->grammar_id != 0) {
        if (!d->gram) return option_off("grammar", "grammar");
        held.g = engine_grammar_ref_id(d->pre[0], q->grammar_id);
        if (!held.g) {
            char m[128]; snprintf(m, sizeof m, "grammar: %d is not a live grammar of this dispatcher's weight owner", (int)q->grammar_id);
            return engine_thread_fail(SONIC_ERR_INVALID, m);
        }
    }
    if (q->n_draft < 0 || (q->n_draft > 0 && !q->draft_ids)) return SONIC_ERR_INVALID;
    if (q->n_draft > 0) {
        if (!d->draft) return option_off("draft", "draft_verify");
        const int rc = engine_draft_validate(d->pre[0], q->draft_ids, q->n_draft);
        if (rc != SONIC_OK) return rc;
        if (q->n_draft > q->max_new - 1) {
            char m[200]; snprintf(m, sizeof m, "draft: the draft holds %d ids, the request's budget of %d tokens leaves room for %d (the last token is the model's own; nothing is truncated)", (int)q->n_draft, (int)q->max_new, (int)q->max_new - 1);
            return engine_thread_fail(SONIC_ERR_INVALID, m);
        }
        if (!own.bias.val.empty() || (own.sampled && own.temperature > 0.f) || held.g)
            return engine_thread_fail(SONIC_ERR_INVALID, "draft: a drafted request carries no bias table, temperature > 0 or grammar (the verify pass applies the handle's processors only)");
        own.draft.assign(q->draft_ids, q->draft_ids + q->n_draft);
    }
    auto r = std::make_shared<Req>();
    r->W = W;
    r->off.assign(q->host_off, q->host_off + W + 1);
    if (r->off[W] > 0) r->pcm.assign(q->host_pcm, q->host_pcm + r->off[W]);
    if (q->rings) {
        r->rings.assign(q->rings, q->rings + W); r->ring_start.assign(q->ring_start, q->ring_start + W); r->ring_n.assign(q->ring_n, q->ring_n + W);
        for (int w = 0; w < W; ++w) r->any_ring = r->any_ring || q->rings[w];
    }
    r->prompt.assign(q->prompt_ids, q->prompt_ids + q->prompt_len); r->max_new = q->max_new;
    r->own = std::move(own);
    std::unique_lock<std::mutex> lk(d->mu);
    if (d->stop) return SONIC_ERR_INVALID;
    if (d->failed) return d->failed;
    r->own.gram = held.g; held.g = nullptr;                        // (the request keeps the reference until it completes)
    r->ticket = d->next_ticket++;
    d->q.push_back(r); d->queued_windows += W; ++d->outstanding;
    *ticket_out = r->ticket;
    d->cv.notify_all();
    return SONIC_OK;
}

// a request that is still queued leaves the queue (it completes with status SONIC_ERR_INVALID, "cancelled"); one that has reached a handle runs on
SONIC_API int sonic_dispatch_cancel(sonic_dispatch* d, int64_t ticket) {
    if (!d) return SONIC_ERR_INVALID;
    std::unique_lock<std::mutex> lk(d->mu);
    for (auto it = d->q.begin(); it != d->q.end(); ++it)
        if ((*it)->ticket == ticket) { ReqP r = *it; d->q.erase(it); d->queued_windows -= r->W; r->cancelled = true; finish(d, r, SONIC_ERR_INVALID, "cancelled"); return SONIC_OK; }
    return SONIC_ERR_INVALID;
}

// The next completed request, in completion order.  Blocks up to timeout_ms (< 0: until one completes, or the dispatcher has been closed and every
// request has been collected).  *ticket_out = 0: none (timeout, or closed and drained).  Otherwise *status_out is the request's sonic_status, its *n_out tokens are in out_ids
// (at most out_cap are copied) and err (if given) holds the engine's message for a failed request.
static int dispatch_next(sonic_dispatch* d, int timeout_ms, int64_t* ticket_out, int32_t* status_out, int32_t* out_ids, int out_cap, int32_t* n_out,
                         char* err, int err_cap, float* out_lp) {
    *ticket_out = 0;
    std::unique_lock<std::mutex> lk(d->mu);
    auto ready = [&] { return !d->done.empty() || (d->stop && d->outstanding == 0); };
    if (timeout_ms < 0) d->cv_done.wait(lk, ready);
    else if (!d->cv_done.wait_for(lk, std::chrono::milliseconds(timeout_ms), ready)) return SONIC_OK;
    if (d->done.empty()) return SONIC_OK;
    ReqP r = d->done.front(); d->done.pop_front(); --d->outstanding;
    *ticket_out = r->ticket;
    if (status_out) *status_out = r->status;
    const int n = (int)r->ids.size();
    if (n_out) *n_out = n;
    if (out_ids) memcpy(out_ids, r->ids.data(), (size_t)(n < out_cap ? n : out_cap) * 4);
    if (out_lp && (int)r->lp.size() == n * d->lp_w) memcpy(out_lp, r->lp.data(), (size_t)(n < out_cap ? n : out_cap) * d->lp_w * 4);
    if (err && err_cap > 0) { strncpy(err, r->err.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    if (d->stop && d->outstanding == 0) d->cv_done.notify_all();
    return SONIC_OK;
}

SONIC_API int sonic_dispatch_next(sonic_dispatch* d, int timeout_ms, int64_t* ticket_out, int32_t* status_out, int32_t* out_ids, int out_cap, int32_t* n_out,
                                  char* err, int err_cap) {
    if (!d || !ticket_out) return SONIC_ERR_INVALID;
    return dispatch_next(d, timeout_ms, ticket_out, status_out, out_ids, out_cap, n_out, err, err_cap, nullptr);
}
// sonic_dispatch_next plus the completed request's log-probabilities: out_lp[i] belongs to out_ids[i] (at most out_cap are copied); with option top_logprobs = K
// on the handles, token i's record of W = 1 + 2K floats sits at out_lp + i * W (out_lp holds out_cap * W floats).  Needs option
// token_logprobs on every handle of the dispatcher (set on the owner before its slots were created): SONIC_ERR_INVALID otherwise, err names the option.
SONIC_API int sonic_dispatch_next_lp(sonic_dispatch* d, int timeout_ms, int64_t* ticket_out, int32_t* status_out, int32_t* out_ids, int out_cap, int32_t* n_out,
                                     char* err, int err_cap, float* out_lp) {
    if (!d || !ticket_out || !out_lp) return SONIC_ERR_INVALID;
    if (!d->lp) {
        *ticket_out = 0;
        if (err && err_cap > 0) snprintf(err, (size_t)err_cap, "sonic_dispatch_next_lp: option token_logprobs is off on a handle of this dispatcher");
        return SONIC_ERR_INVALID;
    }
    return dispatch_next(d, timeout_ms, ticket_out, status_out, out_ids, out_cap, n_out, err, err_cap, out_lp);
}

SONIC_API int sonic_dispatch_stats(sonic_dispatch* d, int64_t* prefill_batches, int64_t* decode_chunks, int32_t* load_windows, int32_t* free_rows) {
    if (!d) return SONIC_ERR_INVALID;
    std::unique_lock<std::mutex> lk(d->mu);
    int fr = 0; for (int f : d->free_rows) fr += f;
    if (prefill_batches) *prefill_batches = d->batches;
    if (decode_chunks) *decode_chunks = d->chunks;
    if (load_windows) *load_windows = (int32_t)(d->n_rows * (int)d->dec.size() - fr + d->queued_windows);   // rows occupied or reserved + windows queued
    if (free_rows) *free_rows = fr;
    return SONIC_OK;
}

// requests still queued fail at once ("ASR engine is closed"), requests that have reached a handle complete; their results stay collectable by
// sonic_dispatch_next until sonic_dispatch_destroy.  Idempotent.
SONIC_API int sonic_dispatch_close(sonic_dispatch* d) {
    if (!d) return SONIC_OK;
    {
        std::unique_lock<std::mutex> lk(d->mu);
        if (d->stop) return SONIC_OK;
        d->stop = true;
        while (!d->q.empty()) { finish(d, d->q.front(), SONIC_ERR_INVALID, "ASR engine is closed"); d->q.pop_front(); }
        d->queued_windows = 0;
        d->cv.notify_all();
    }
    for (auto& t : d->threads) t.join();
    d->threads.clear();
    for (auto* e : d->dec) (void)sonic_service_end(e);
    std::unique_lock<std::mutex> lk(d->mu);
    d->cv_done.notify_all();
    return SONIC_OK;
}

SONIC_API int sonic_dispatch_destroy(sonic_dispatch* d) {
    if (!d) return SONIC_OK;
    (void)sonic_dispatch_close(d);
    delete d;
    return SONIC_OK;
}

}   // extern "C"
