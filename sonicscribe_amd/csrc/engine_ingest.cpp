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
    // Rate ring (sonic_ring_create_rate, in_rate != 16000): appends take samples at in_rate, the resampler kernel (resample.hip) writes the
    // ring's 16 kHz int16 content; indices, head and every reader stay in 16 kHz samples.  The raw samples go through `lin`: the carry - the
    // last input samples the next frames still need, fewer than K - right-aligned in front of the piece that was just uploaded.
    bool rated = false;
    RsBank bank;
    int16_t* lin = nullptr;                // device: [carry_max | piece] samples at in_rate
    int16_t* host_in = nullptr;            // pinned mirror of the raw chunks: 2 * piece samples, used circularly (`mpos`, `unsynced`)
    int64_t carry_max = 0, piece = 0, carry = 0, mpos = 0;
    int64_t n_in = 0, emitted = 0;         // of the current stream: input samples so far, outputs already in the ring (= J(n_in))
    int64_t dev_bytes = 0;                 // what this ring added to the owner's ring_bytes
};
// outputs whose taps all exist after N input samples: whole frames only
static int64_t rate_emitted(const RsBank& b, int64_t N) { return N >= b.width + b.of ? (int64_t)b.nf * ((N - b.width - b.of) / b.of + 1) : 0; }

static int ring_create_locked(sonic_engine* e, int64_t capacity_samples, const RsBank* bank, sonic_ring** out) {
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
    r->dev_bytes = capacity_samples * 2;
    if (bank) {
        r->rated = true; r->bank = *bank;
        r->carry_max = (int64_t)bank->K + bank->of;
        // the largest chunk whose outputs can fit the ring, cut into pieces of at most 2^18 samples (chunking does not change a bit)
        const int64_t n_max = (capacity_samples / bank->nf + 2) * bank->of + bank->K;
        r->piece = n_max < ((int64_t)1 << 18) ? n_max : ((int64_t)1 << 18);
        const size_t lin_bytes = (size_t)(r->carry_max + r->piece) * 2;
        hipError_t er = hipMalloc((void**)&r->lin, lin_bytes);
        if (er == hipSuccess) er = hipHostMalloc((void**)&r->host_in, (size_t)r->piece * 4, hipHostMallocDefault);
        if (er != hipSuccess) {
            (void)hipGetLastError();
            if (r->lin) (void)hipFree(r->lin);
            (void)hipFree(r->buf); (void)hipHostFree(r->host); (void)hipStreamDestroy(r->st); (void)hipEventDestroy(r->read_ev); (void)hipEventDestroy(r->app_ev);
            delete r; return fail(e, SONIC_ERR_OOM, "out of memory (rate ring: %zu bytes of input staging)", lin_bytes);
        }
        r->dev_bytes += (int64_t)lin_bytes;
    }
    zero_fill(e, r->buf, (size_t)capacity_samples * 2);
    HIPC(e, stream_sync(e));
    // rings live in the registry of the weight owner: every slot of an engine may stage from every ring of it
    sonic_engine* root = e->owner ? e->owner : e;
    r->e = root;
    { std::lock_guard<std::mutex> rl(root->rings_mu); root->rings.push_back(r); }
    root->ring_bytes += r->dev_bytes;
    *out = r;
    return SONIC_OK;
}
extern "C" int sonic_ring_create(sonic_engine* e, int64_t capacity_samples, sonic_ring** out) {
    if (!e || !out) return SONIC_ERR_INVALID;
    ENTER(e);
    return ring_create_locked(e, capacity_samples, nullptr, out);
}
// A ring fed at in_rate (8 kHz telephony, 44.1 kHz files, 48 kHz capture): what the reference resamples on the host before anything else sees
// the audio (torchaudio Resample at backend/vad.py:63-67 and :108-112, set_frame_rate(16000) at backend/utils.py:18).  in_rate == 16000 is
// exactly sonic_ring_create's ring.
extern "C" int sonic_ring_create_rate(sonic_engine* e, int64_t capacity_samples, int32_t in_rate, sonic_ring** out) {
    if (!e || !out) return SONIC_ERR_INVALID;
    ENTER(e);
    if (in_rate == 16000) return ring_create_locked(e, capacity_samples, nullptr, out);
    RsBank b; std::string err;
    const int rc = resample_bank_get(e->owner ? e->owner : e, in_rate, 16000, &b, err);
    if (rc != SONIC_OK) return fail(e, rc, "%s", err.c_str());
    return ring_create_locked(e, capacity_samples, &b, out);
}
void ring_free(sonic_ring* r) {
    {
        std::lock_guard<std::mutex> lk(r->mu);
        (void)hipSetDevice(r->e->device);
        (void)hipStreamSynchronize(r->st);
        (void)hipFree(r->buf); (void)hipHostFree(r->host); (void)hipStreamDestroy(r->st); (void)hipEventDestroy(r->read_ev); (void)hipEventDestroy(r->app_ev);
        if (r->lin) (void)hipFree(r->lin);
        if (r->host_in) (void)hipHostFree(r->host_in);
        r->e->ring_bytes -= r->dev_bytes;
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
// kernel arguments of a rate ring's next outputs: the source is carry + chunk in `lin`, the first output lands at the ring's head
static ResampleArgs rate_args(sonic_ring* r) {
    const RsBank& b = r->bank;
    ResampleArgs a{};
    a.src = r->lin + r->carry_max - r->carry; a.src_base = r->n_in - r->carry;
    a.bank = b.dev; a.of = b.of; a.nf = b.nf; a.width = b.width; a.K = b.K; a.tile = b.tile; a.kc = b.kc;
    a.j0 = r->emitted; a.ring = r->buf; a.ring_cap = r->cap; a.ring_pos = r->head % r->cap;
    return a;
}
// sonic_ring_append on a rate ring (under the ring's lock): n samples at in_rate.  After N input samples in total the ring holds the outputs
// j < J(N) (rate_emitted: the frames whose taps all exist); the chunk is refused when its outputs exceed the capacity.  Non-blocking like the
// plain append: pinned mirror of the raw chunk, async H2D, the kernel and the carry move on the ring's stream, app_ev behind them.
static int rate_append_locked(sonic_ring* r, const int16_t* pcm, int64_t n, int64_t* first_index) {
    const RsBank& b = r->bank;
    const int64_t total = rate_emitted(b, r->n_in + n) - r->emitted;
    if (total > r->cap)
        return fail(nullptr, SONIC_ERR_INVALID, "sonic_ring_append: a chunk of %lld samples makes %lld outputs, the ring holds %lld", (long long)n, (long long)total, (long long)r->cap);
    auto hip_fail = [&](const char* what, hipError_t er) { (void)hipGetLastError(); return fail(nullptr, SONIC_ERR_HIP, "sonic_ring_append: %s failed: %s", what, hipGetErrorString(er)); };
    hipError_t er = hipSetDevice(r->e->device);
    if (er != hipSuccess) return hip_fail("hipSetDevice", er);
    if (first_index) *first_index = r->head;
    const int64_t M = 2 * r->piece;
    for (int64_t off = 0; off < n;) {
        const int64_t m = n - off < r->piece ? n - off : r->piece;
        // the mirror is a circular buffer of contiguous slots; the stream is drained before a slot could be rewritten under a pending copy
        if (r->mpos + m > M) { r->unsynced += M - r->mpos; r->mpos = 0; }
        if (r->unsynced + m > M) { er = hipStreamSynchronize(r->st); if (er != hipSuccess) return hip_fail("hipStreamSynchronize", er); r->unsynced = 0; }
        memcpy(r->host_in + r->mpos, pcm + off, (size_t)m * 2);
        er = hipMemcpyAsync(r->lin + r->carry_max, r->host_in + r->mpos, (size_t)m * 2, hipMemcpyHostToDevice, r->st);
        if (er != hipSuccess) return hip_fail("hipMemcpyAsync", er);
        r->mpos += m; r->unsynced += m;
        const int64_t N = r->n_in + m, J = rate_emitted(b, N);
        ResampleArgs a = rate_args(r);
        a.src_n = r->carry + m; a.n_out = J - r->emitted;
        launch_resample(a, false, r->st);
        // what the next frame (J / nf) still needs: the samples from its first tap on
        const int64_t lowest = (J / b.nf) * b.of - b.width > 0 ? (J / b.nf) * b.of - b.width : 0, keep = N - lowest;
        launch_resample_carry(r->lin, r->carry_max - keep, r->carry_max + m - keep, keep, r->st);
        if ((er = hipGetLastError()) != hipSuccess) return hip_fail("resample kernel launch", er);
        r->head += a.n_out; r->emitted = J; r->n_in = N; r->carry = keep;
        off += m;
    }
    if (n > 0) { er = hipEventRecord(r->app_ev, r->st); if (er != hipSuccess) return hip_fail("hipEventRecord", er); r->app_pending = true; }
    return SONIC_OK;
}
// Ends the stream of a rate ring: emits the outputs J(N) .. ceil(nf * N / of) - 1 with zeros beyond the N samples appended (the trim of the
// one-shot resampler); the next append starts a new stream with zero history.  Nothing to do on a 16 kHz ring.
extern "C" int sonic_ring_flush(sonic_ring* r) {
    if (!r) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(r->mu);
    if (!r->rated || r->n_in == 0) return SONIC_OK;
    const RsBank& b = r->bank;
    const int64_t total = ((int64_t)b.nf * r->n_in + b.of - 1) / b.of, n_out = total - r->emitted;
    if (n_out > r->cap) return fail(nullptr, SONIC_ERR_INVALID, "sonic_ring_flush: %lld outputs, the ring holds %lld", (long long)n_out, (long long)r->cap);
    auto hip_fail = [&](const char* what, hipError_t er) { (void)hipGetLastError(); return fail(nullptr, SONIC_ERR_HIP, "sonic_ring_flush: %s failed: %s", what, hipGetErrorString(er)); };
    hipError_t er = hipSetDevice(r->e->device);
    if (er != hipSuccess) return hip_fail("hipSetDevice", er);
    if (n_out > 0) {
        ResampleArgs a = rate_args(r);
        a.src_n = r->carry; a.n_out = n_out;
        launch_resample(a, false, r->st);
        if ((er = hipGetLastError()) != hipSuccess) return hip_fail("resample kernel launch", er);
        if ((er = hipEventRecord(r->app_ev, r->st)) != hipSuccess) return hip_fail("hipEventRecord", er);
        r->app_pending = true;
        r->head += n_out;
    }
    r->n_in = 0; r->emitted = 0; r->carry = 0;
    return SONIC_OK;
}
// Ring samples [first, first + n) to the host, behind every append so far: the device session's counterpart of the reference's per-session
// debug WAV dump (backend/debug.py:14-72).  The range rule is sonic_stage_mixed's.
extern "C" int sonic_ring_read(sonic_ring* r, int64_t first, int64_t n, int16_t* out_i16) {
    if (!r || (!out_i16 && n > 0)) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(r->mu);
    if (n < 0 || first < 0 || first + n > r->head || first < r->head - r->cap)
        return fail(nullptr, SONIC_ERR_INVALID, "sonic_ring_read: samples [%lld, %lld) are not in the ring (holds [%lld, %lld))", (long long)first, (long long)(first + n),
                    (long long)(r->head > r->cap ? r->head - r->cap : 0), (long long)r->head);
    if (n == 0) return SONIC_OK;
    auto hip_fail = [&](const char* what, hipError_t er) { (void)hipGetLastError(); return fail(nullptr, SONIC_ERR_HIP, "sonic_ring_read: %s failed: %s", what, hipGetErrorString(er)); };
    hipError_t er = hipSetDevice(r->e->device);
    if (er != hipSuccess) return hip_fail("hipSetDevice", er);
    const int64_t pos = first % r->cap, head_n = n < r->cap - pos ? n : r->cap - pos;
    // on the ring's own stream: in order behind the appends (and their kernels)
    if ((er = hipMemcpyAsync(out_i16, r->buf + pos, (size_t)head_n * 2, hipMemcpyDeviceToHost, r->st)) != hipSuccess) return hip_fail("hipMemcpyAsync", er);
    if (n > head_n && (er = hipMemcpyAsync(out_i16 + head_n, r->buf, (size_t)(n - head_n) * 2, hipMemcpyDeviceToHost, r->st)) != hipSuccess) return hip_fail("hipMemcpyAsync (wrap)", er);
    if ((er = hipStreamSynchronize(r->st)) != hipSuccess) return hip_fail("hipStreamSynchronize", er);
    r->unsynced = 0;
    return SONIC_OK;
}
// append n samples; *first_index = absolute index of pcm[0].  Returns at once (the samples are copied to the pinned mirror, the caller may
// reuse pcm); the H2D copy is queued on the ring's stream and every later staging kernel orders behind it.
// (A rate ring: n samples at its input rate, *first_index = the head before the call; rate_append_locked.)
extern "C" int sonic_ring_append(sonic_ring* r, const int16_t* pcm, int64_t n, int64_t* first_index) {
    if (!r || (!pcm && n > 0) || n < 0) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(r->mu);
    if (r->rated) return rate_append_locked(r, pcm, n, first_index);
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
    if (!e) return SONIC_ERR_INVALID;
    ENTER_CONSUME(e);
    if (!prompt_ids || !prompt_off || !max_new) return SONIC_ERR_INVALID;
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
    if (!e) return SONIC_ERR_INVALID;
    ENTER_CONSUME(e);
    if (!prompt_ids || !prompt_off || !max_new) return SONIC_ERR_INVALID;
    return run_all(e, req_win, R, prompt_ids, prompt_off, max_new, want_step_logits != 0);
}
