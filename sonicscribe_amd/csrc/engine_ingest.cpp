// sonic_hip engine: PCM staging from the host, device-resident rings, mixed staging, and the batch entry points that start from staged PCM.
#include "engine_internal.h"
#include "ring_access.h"

// ------------------------------------------------------------------------------------------ C ABI: hot path
int stage_pcm_locked(sonic_engine* e, const int16_t* pcm, const int64_t* offsets, int W) {
    const sonic_dims& d = e->d;
    if (!pcm || !offsets) return fail(e, SONIC_ERR_INVALID, "null argument");
    if (W < 1 || W > e->Bm) return fail(e, SONIC_ERR_INVALID, "window count %d out of range 1..%d", W, e->Bm);
    const long cap = (long)d.n_frames * 160;
    for (int i = 0; i < W; ++i) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (n < 0 || n > cap) return fail(e, SONIC_ERR_INVALID, "window %d has %lld samples (max %ld)", i, (long long)n, cap);
        e->n_samples_h[i] = (int)n;
        if (n > 0) HIPC(e, hipMemcpyAsync(e->pcm + (size_t)i * cap, pcm + offsets[i], (size_t)n * 2, hipMemcpyHostToDevice, e->st));
    }
    HIPC(e, hipMemcpyAsync(e->n_samples_d, e->n_samples_h.data(), (size_t)W * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, stream_sync(e));
    e->W = W;
    return SONIC_OK;
}

// ------------------------------------------------------------------------------------------ device-resident ingest
// A ring holds the raw wire PCM of one session in HBM (the reference keeps the chunks in a host dict, audio_manager.py:21-33, and
// concatenates them on the host for every decode, :106-123).  Appends run on the ring's own stream under the ring's own lock, so the
// event-loop thread that feeds 2048-byte chunks never waits for a batch that is decoding under the engine lock.
struct sonic_ring {
    sonic_engine* e = nullptr;
    int16_t* buf = nullptr;
    int16_t* host = nullptr;               // pinned mirror: an append is a host memcpy + an async H2D copy, the caller never waits for the
                                           // device (a synchronous 2 KB copy queues behind whatever kernels occupy the GPU: 0.6-1.4 ms measured)
    int64_t cap = 0, head = 0;             // capacity in samples; samples appended so far (absolute index of the next one)
    std::mutex mu;
    hipStream_t st = nullptr;
    hipEvent_t read_ev = nullptr; bool read_pending = false;   // last staging kernel that read this ring (appends order behind it)
    hipEvent_t app_ev = nullptr; bool app_pending = false;     // last append (staging kernels order behind it)
    int64_t unsynced = 0;                  // samples whose H2D copy may still be reading the pinned mirror
};

extern "C" int sonic_ring_create(sonic_engine* e, int64_t capacity_samples, sonic_ring** out) {
    if (!e || !out) return SONIC_ERR_INVALID;
    ENTER(e);
    if (capacity_samples < 1024 || capacity_samples > ((int64_t)1 << 31)) return fail(e, SONIC_ERR_INVALID, "ring capacity %lld out of range", (long long)capacity_samples);
    sonic_ring* r = new sonic_ring();
    r->e = e; r->cap = capacity_samples;
    if (hipMalloc((void**)&r->buf, (size_t)capacity_samples * 2) != hipSuccess) { delete r; return fail(e, SONIC_ERR_OOM, "HIP out of memory (ring of %lld samples)", (long long)capacity_samples); }
    if (hipHostMalloc((void**)&r->host, (size_t)capacity_samples * 2, hipHostMallocDefault) != hipSuccess) { (void)hipFree(r->buf); delete r; return fail(e, SONIC_ERR_OOM, "pinned host memory exhausted (ring mirror)"); }
    if (hipStreamCreateWithFlags(&r->st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&r->read_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&r->app_ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipFree(r->buf); (void)hipHostFree(r->host); if (r->st) (void)hipStreamDestroy(r->st); if (r->read_ev) (void)hipEventDestroy(r->read_ev);
        delete r; return fail(e, SONIC_ERR_HIP, "ring stream / event creation failed");
    }
    zero_fill(e, r->buf, (size_t)capacity_samples * 2);
    HIPC(e, stream_sync(e));
    // rings live in the registry of the weight owner: every slot of an engine may stage from every ring of it
    sonic_engine* root = e->owner ? e->owner : e;
    r->e = root;
    { std::lock_guard<std::mutex> rl(root->rings_mu); root->rings.push_back(r); }
    root->ring_bytes += capacity_samples * 2;
    *out = r;
    return SONIC_OK;
}
void ring_free(sonic_ring* r) {
    {
        std::lock_guard<std::mutex> lk(r->mu);
        (void)hipSetDevice(r->e->device);
        (void)hipStreamSynchronize(r->st);
        (void)hipFree(r->buf); (void)hipHostFree(r->host); (void)hipStreamDestroy(r->st); (void)hipEventDestroy(r->read_ev); (void)hipEventDestroy(r->app_ev);
        r->e->ring_bytes -= r->cap * 2;
    }
    delete r;
}
extern "C" void sonic_ring_destroy(sonic_ring* r) {
    if (!r) return;
    {
        // Unregister first: a batch that names this ring from now on is refused (stage_mixed_locked looks the pointer up under the same lock
        // before it touches it); a batch that already holds the ring's lock finishes its staging kernels before ring_free gets the lock.
        std::lock_guard<std::mutex> lk(r->e->rings_mu);
        auto& v = r->e->rings;
        v.erase(std::remove(v.begin(), v.end(), r), v.end());
    }
    ring_free(r);
}
extern "C" int64_t sonic_ring_head(sonic_ring* r) {
    if (!r) return -1;
    std::lock_guard<std::mutex> lk(r->mu);
    return r->head;
}
// append n samples; *first_index = absolute index of pcm[0].  Returns at once (the samples are copied to the pinned mirror, the caller may
// reuse pcm); the H2D copy is queued on the ring's stream and every later staging kernel orders behind it.
extern "C" int sonic_ring_append(sonic_ring* r, const int16_t* pcm, int64_t n, int64_t* first_index) {
    if (!r || (!pcm && n > 0) || n < 0) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(r->mu);
    if (n > r->cap) return SONIC_ERR_INVALID;
    // failures are reported through sonic_last_error(NULL) of the calling thread (appends do not take the engine lock, so they cannot
    // write the engine's own error string)
    auto hip_fail = [&](const char* what, hipError_t er) { (void)hipGetLastError(); return fail(nullptr, SONIC_ERR_HIP, "sonic_ring_append: %s failed: %s", what, hipGetErrorString(er)); };
    hipError_t er = hipSetDevice(r->e->device);
    if (er != hipSuccess) return hip_fail("hipSetDevice", er);
    // No device-side ordering against the staging kernels is needed: a batch holds the locks of its rings from the range check until its
    // staging kernels have COMPLETED (stage_mixed_locked ends with a stream synchronise), and this function runs under the ring's lock.
    // (Rounds 2-3 also recorded an event behind the staging kernels and made the ring's stream wait for it here.  The runtime refuses
    // both hipStreamWaitEvent and hipEventSynchronize on an event whose stream is capturing at that moment - the engine thread captures a
    // decode graph for every new batch size - "operation not permitted on an event last recorded in a capturing stream": an append then
    // failed, or left a sticky error that failed an unrelated call later.  Found by tests/test_gpu_sessions.py in full-suite runs.)
    const int64_t pos = r->head % r->cap, first = n < r->cap - pos ? n : r->cap - pos;
    // A mirror slot is rewritten one full capacity later (30 s of audio), normally long after its copy has left; the stream is
    // drained before an append could overwrite samples whose copy has not been waited for (small rings, bursts).
    if (r->unsynced + n > r->cap) { er = hipStreamSynchronize(r->st); if (er != hipSuccess) return hip_fail("hipStreamSynchronize", er); r->unsynced = 0; }
    r->unsynced += n;
    if (first > 0) {
        memcpy(r->host + pos, pcm, (size_t)first * 2);
        er = hipMemcpyAsync(r->buf + pos, r->host + pos, (size_t)first * 2, hipMemcpyHostToDevice, r->st);
        if (er != hipSuccess) return hip_fail("hipMemcpyAsync", er);
    }
    if (n > first) {
        memcpy(r->host, pcm + first, (size_t)(n - first) * 2);
        er = hipMemcpyAsync(r->buf, r->host, (size_t)(n - first) * 2, hipMemcpyHostToDevice, r->st);
        if (er != hipSuccess) return hip_fail("hipMemcpyAsync (wrap)", er);
    }
    if (n > 0) { er = hipEventRecord(r->app_ev, r->st); if (er != hipSuccess) return hip_fail("hipEventRecord", er); r->app_pending = true; }
    if (first_index) *first_index = r->head;
    r->head += n;
    return SONIC_OK;
}

// windows of a batch from host memory (rings == NULL or rings[w] == NULL: int16 PCM already normalised by the caller, as
// sonic_stage_pcm) and / or from rings (raw wire PCM: a1 + a2 on the device, peak over the windows of one request)
static int stage_mixed_locked(sonic_engine* e, int W, const int16_t* host_pcm, const int64_t* host_off, sonic_ring* const* rings,
                              const int64_t* ring_start, const int32_t* ring_n, const int32_t* req_win, int R) {
    const sonic_dims& d = e->d;
    if (W < 1 || W > e->Bm || W > RING_MAX_WIN) return fail(e, SONIC_ERR_INVALID, "window count %d out of range 1..%d", W, e->Bm < RING_MAX_WIN ? e->Bm : RING_MAX_WIN);
    if (req_win) { if (R < 1 || R > W || req_win[0] != 0 || req_win[R] != W) return fail(e, SONIC_ERR_INVALID, "req_win does not cover the %d windows", W); }
    else if (R != W) return fail(e, SONIC_ERR_INVALID, "without req_win every window is its own request");
    const long cap = (long)d.n_frames * 160;
    RingStageArgs ra{};
    int max_n = 0; bool any_ring = false;
    // every ring of the batch stays locked from the range check until the staging kernels have run (this function ends with a stream
    // synchronise): an append in between could overwrite the oldest samples of a window that starts at the tail of its ring
    std::vector<sonic_ring*> used;
    std::vector<std::unique_lock<std::mutex>> held;
    if (rings) {
        sonic_engine* root = e->owner ? e->owner : e;
        std::lock_guard<std::mutex> rl(root->rings_mu);        // registry lookup + ring locks as one step against sonic_ring_destroy
        for (int w = 0; w < W; ++w)
            if (rings[w] && std::find(used.begin(), used.end(), rings[w]) == used.end()) {
                if (std::find(root->rings.begin(), root->rings.end(), rings[w]) == root->rings.end())
                    return fail(e, SONIC_ERR_INVALID, "window %d: ring belongs to another engine (or was destroyed)", w);
                used.push_back(rings[w]);
            }
        std::sort(used.begin(), used.end());                   // one lock order for every batch (two slots may stage from overlapping ring sets)
        held.reserve(used.size());
        for (sonic_ring* rg : used) held.emplace_back(rg->mu);
    }
    for (int r = 0, w = 0; r < R; ++r) {
        const int w1 = req_win ? req_win[r + 1] : r + 1;
        if (w1 <= w) return fail(e, SONIC_ERR_INVALID, "request %d has no window", r);
        for (; w < w1; ++w) {
            ra.req_of[w] = r;
            sonic_ring* rg = rings ? rings[w] : nullptr;
            if (rg) {
                const int64_t n = ring_n[w], st = ring_start[w];
                if (n < 0 || n > cap || st < 0 || st + n > rg->head || st < rg->head - rg->cap)
                    return fail(e, SONIC_ERR_INVALID, "window %d: samples [%lld, %lld) are not in the ring (holds [%lld, %lld))", w, (long long)st, (long long)(st + n),
                                (long long)(rg->head > rg->cap ? rg->head - rg->cap : 0), (long long)rg->head);
                if (rg->app_pending && hipStreamWaitEvent(e->st, rg->app_ev, 0) != hipSuccess) {   // the appended samples are (or will be) in HBM first
                    (void)hipGetLastError();
                    HIPC(e, hipEventSynchronize(rg->app_ev));
                }
                ra.ring[w] = rg->buf; ra.ring_cap[w] = rg->cap; ra.start[w] = st % rg->cap; ra.n[w] = (int)n;
                e->n_samples_h[w] = (int)n;
                if ((int)n > max_n) max_n = (int)n;
                any_ring = true;
            } else {
                if (!host_pcm || !host_off) return fail(e, SONIC_ERR_INVALID, "window %d: neither ring nor host samples", w);
                const int64_t n = host_off[w + 1] - host_off[w];
                if (n < 0 || n > cap) return fail(e, SONIC_ERR_INVALID, "window %d has %lld samples (max %ld)", w, (long long)n, cap);
                e->n_samples_h[w] = (int)n;
                if (n > 0) HIPC(e, hipMemcpyAsync(e->pcm + (size_t)w * cap, host_pcm + host_off[w], (size_t)n * 2, hipMemcpyHostToDevice, e->st));
            }
        }
    }
    if (any_ring) {
        ra.peak = e->ring_peak; ra.pcm = e->pcm; ra.win_cap = cap;
        launch_fill_i32(e->ring_peak, 0, e->Bm, e->st);
        launch_ring_stage(ra, W, max_n, e->st);
    }
    HIPC(e, hipMemcpyAsync(e->n_samples_d, e->n_samples_h.data(), (size_t)W * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    e->W = W;
    return SONIC_OK;
}
// sample ranges of rings for a reader outside the engine (sonic_vad_probs_rings): the registry, lock and range rules of stage_mixed_locked
int ring_ranges_acquire(sonic_engine* e, sonic_ring* const* ring, const int64_t* start, const int32_t* n, int64_t P, int device, hipStream_t st,
                        RingView* view, std::vector<std::unique_lock<std::mutex>>& held, std::string& err) {
    char msg[256];
    sonic_engine* root = e->owner ? e->owner : e;
    if (root->device != device) {
        snprintf(msg, sizeof msg, "the engine's rings are on device %d, the VAD handle on device %d", root->device, device);
        err = msg; return SONIC_ERR_INVALID;
    }
    std::vector<sonic_ring*> used;
    {
        std::lock_guard<std::mutex> rl(root->rings_mu);        // registry lookup + ring locks as one step against sonic_ring_destroy
        for (int64_t p = 0; p < P; ++p)
            if (std::find(used.begin(), used.end(), ring[p]) == used.end()) {
                if (!ring[p] || std::find(root->rings.begin(), root->rings.end(), ring[p]) == root->rings.end()) {
                    snprintf(msg, sizeof msg, "piece %lld: ring belongs to another engine (or was destroyed)", (long long)p);
                    err = msg; return SONIC_ERR_INVALID;
                }
                used.push_back(ring[p]);
            }
        std::sort(used.begin(), used.end());                   // the lock order of every batch and every VAD call
        held.reserve(used.size());
        for (sonic_ring* rg : used) held.emplace_back(rg->mu);
    }
    for (int64_t p = 0; p < P; ++p) {
        sonic_ring* rg = ring[p];
        const int64_t len = n[p], s0 = start[p];
        if (len < 0 || s0 < 0 || s0 + len > rg->head || s0 < rg->head - rg->cap) {
            snprintf(msg, sizeof msg, "piece %lld: samples [%lld, %lld) are not in the ring (holds [%lld, %lld))", (long long)p, (long long)s0,
                     (long long)(s0 + len), (long long)(rg->head > rg->cap ? rg->head - rg->cap : 0), (long long)rg->head);
            err = msg; held.clear(); return SONIC_ERR_INVALID;
        }
        view[p].buf = rg->buf; view[p].cap = rg->cap;
    }
    for (sonic_ring* rg : used)                                 // the appended samples are (or will be) in HBM first
        if (rg->app_pending && hipStreamWaitEvent(st, rg->app_ev, 0) != hipSuccess) {
            (void)hipGetLastError();
            const hipError_t er = hipEventSynchronize(rg->app_ev);
            if (er != hipSuccess) { err = std::string("hipEventSynchronize(app_ev) failed: ") + hipGetErrorString(er); held.clear(); return SONIC_ERR_HIP; }
        }
    return SONIC_OK;
}

extern "C" int sonic_stage_mixed(sonic_engine* e, const int16_t* host_pcm, const int64_t* host_off, sonic_ring* const* rings, const int64_t* ring_start,
                                 const int32_t* ring_n, int W, const int32_t* req_win, int R) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    return stage_mixed_locked(e, W, host_pcm, host_off, rings, ring_start, ring_n, req_win, R);
}
extern "C" int sonic_transcribe_mixed(sonic_engine* e, const int16_t* host_pcm, const int64_t* host_off, sonic_ring* const* rings, const int64_t* ring_start,
                                      const int32_t* ring_n, int W, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                                      const int32_t* max_new, int32_t* out_ids, int out_ld, int32_t* out_len, float* step_logits) {
    if (!e || !prompt_ids || !prompt_off || !max_new) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(stage_mixed_locked(e, W, host_pcm, host_off, rings, ring_start, ring_n, req_win, R));
    TRY(run_all(e, req_win, R, prompt_ids, prompt_off, max_new, step_logits != nullptr));
    return fetch_locked(e, out_ids, out_ld, out_len, step_logits);
}

extern "C" int sonic_stage_pcm(sonic_engine* e, const int16_t* pcm, const int64_t* offsets, int W) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    return stage_pcm_locked(e, pcm, offsets, W);
}

extern "C" int sonic_run_staged(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                                const int32_t* max_new, int want_step_logits) {
    if (!e || !prompt_ids || !prompt_off || !max_new) return SONIC_ERR_INVALID;
    ENTER(e);
    return run_all(e, req_win, R, prompt_ids, prompt_off, max_new, want_step_logits != 0);
}
