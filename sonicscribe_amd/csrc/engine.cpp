// sonic_hip engine: weights, HBM buffers, the mel -> encoder -> projector -> prefill -> greedy-decode
// pipeline on one HIP stream, hipGraph-captured decode step, and the C ABI of include/sonic_hip.h.
// One engine = one full model replica on one MI355X (replicas, no collectives).
// This unit: the shared helpers, the constant tables, create / slot / destroy / info / synchronise.  The other sections of the engine live in
// engine_generation.cpp (what a handle generates with: log-probabilities, guards, the per-request stages), engine_weights.cpp, engine_stages.cpp (the forward
// pass and the whole-batch run around it), engine_decode.cpp (the token step and its loop), engine_score.cpp (the runs that score given tokens), engine_f32.cpp,
// engine_ingest.cpp, engine_service.cpp, engine_options.cpp and engine_hooks.cpp; engine_internal.h is what they share.
#include "engine_internal.h"

static thread_local std::string g_create_err;

// ------------------------------------------------------------------------------------------ helpers
int fail(sonic_engine* e, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (e) e->err = buf; else g_create_err = buf;
    return code;
}

// Host -> device copy on the ENGINE stream, complete on return.  Never use the null-stream hipMemcpy for uploads: the
// engine stream is non-blocking, so a null-stream copy is not ordered against work still queued on it (dalloc's zero fill
// once wiped parts of a freshly uploaded RoPE table that way).
hipError_t h2d(sonic_engine* e, void* dst, const void* src, size_t bytes) {
    hipError_t r = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->st);
    if (r != hipSuccess) return r;
    return stream_sync(e);
}

// Device -> host on the ENGINE stream.  The synchronous hipMemcpy goes through the legacy stream, which implicitly synchronises with
// other streams of the process: with several engines in one process (replicas on one or several GPUs) it failed with "operation would
// make the legacy stream depend on a capturing blocking stream" while another engine's thread was capturing its decode graph.
hipError_t d2h_async(sonic_engine* e, void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->st);
}
hipError_t d2h(sonic_engine* e, void* dst, const void* src, size_t bytes) {
    hipError_t r = d2h_async(e, dst, src, bytes);
    return r == hipSuccess ? stream_sync(e) : r;
}
// Wait for the engine stream WITHOUT spinning.  hipStreamSynchronize busy-waits on this runtime when the machine shows more CPUs than contexts
// (256 visible): every waiting thread of every slot / rank burnt a CPU - 3.7 CPUs for three slots of one rank, far beyond a 16-CPU quota at eight
// ranks, and a job that exhausts its quota has ALL its threads frozen.  An event created with hipEventBlockingSync sleeps on an
// interrupt instead; the wake-up is slower by tens of microseconds, which the queued work hides (the decode loop keeps `lookahead` chunks ahead).
hipError_t stream_sync(sonic_engine* e) {
    if (!e->sync_ev) return hipStreamSynchronize(e->st);
    hipError_t r = hipEventRecord(e->sync_ev, e->st);
    return r == hipSuccess ? hipEventSynchronize(e->sync_ev) : r;
}
// zero fill by a kernel on the engine stream (hipMemsetAsync on a non-blocking stream: see TmpBuf::get, engine_hooks.cpp)
void zero_fill(sonic_engine* e, void* q, size_t bytes) {
    size_t left = bytes / 4; int* w = (int*)q;
    while (left > 0) { const int c = left > (1u << 30) ? (1 << 30) : (int)left; launch_fill_i32(w, 0, c, e->st); w += c; left -= c; }
}

static inline float bf16_round_host(float x) {
    uint32_t u; memcpy(&u, &x, 4);
    u = (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u;
    memcpy(&x, &u, 4); return x;
}

// ------------------------------------------------------------------------------------------ constants
static int build_constants(sonic_engine* e) {
    const sonic_dims& d = e->d;
    std::vector<float> win(400), ct(400), stb(400);
    for (int i = 0; i < 400; ++i) {
        win[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * i / 400.0));   // torch.hann_window(400), periodic
        ct[i] = (float)cos(2.0 * M_PI * i / 400.0);
        stb[i] = (float)sin(2.0 * M_PI * i / 400.0);
    }
    // slaney mel bank, HF:audio_utils.py:448-518,541-560,690-722 -> CSR per filter
    const int nm = d.n_mels, nf = nm + 2;
    auto hz2mel = [](double f) { return f >= 1000.0 ? 15.0 + log(f / 1000.0) * (27.0 / log(6.4)) : 3.0 * f / 200.0; };
    auto mel2hz = [](double m) { return m >= 15.0 ? 1000.0 * exp((log(6.4) / 27.0) * (m - 15.0)) : 200.0 * m / 3.0; };
    std::vector<double> ffq(nf);
    const double mmin = hz2mel(0.0), mmax = hz2mel(8000.0);
    for (int i = 0; i < nf; ++i) ffq[i] = mel2hz(i == nf - 1 ? mmax : mmin + (mmax - mmin) / (nf - 1) * i);
    std::vector<int> lo(nm), cnt(nm), off(nm);
    std::vector<float> w;
    for (int m = 0; m < nm; ++m) {
        int first = -1, last = -2;
        std::vector<float> taps(201);
        for (int b = 0; b < 201; ++b) {
            const double fb = (b == 200) ? 8000.0 : 8000.0 / 200.0 * b;
            const double down = -(ffq[m] - fb) / (ffq[m + 1] - ffq[m]), up = (ffq[m + 2] - fb) / (ffq[m + 2] - ffq[m + 1]);
            double v = down < up ? down : up; if (v < 0) v = 0;
            v *= 2.0 / (ffq[m + 2] - ffq[m]);
            taps[b] = (float)v;
            if (taps[b] != 0.f) { if (first < 0) first = b; last = b; }
        }
        if (first < 0) { first = 0; last = -1; }
        lo[m] = first; cnt[m] = last - first + 1; off[m] = (int)w.size();
        for (int b = first; b <= last; ++b) w.push_back(taps[b]);
    }
    float *dwin, *dct, *dst, *dw; int *dlo, *dcnt, *doff;
    TRY(dalloc(e, &dwin, 400)); TRY(dalloc(e, &dct, 400)); TRY(dalloc(e, &dst, 400)); TRY(dalloc(e, &dw, w.size()));
    TRY(dalloc(e, &dlo, nm)); TRY(dalloc(e, &dcnt, nm)); TRY(dalloc(e, &doff, nm));
    HIPC(e, hipMemcpyAsync(dwin, win.data(), 1600, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(dct, ct.data(), 1600, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(dst, stb.data(), 1600, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(dw, w.data(), w.size() * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(dlo, lo.data(), nm * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(dcnt, cnt.data(), nm * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(doff, off.data(), nm * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, stream_sync(e));
    e->lc = LogmelConst{dwin, dct, dst, dlo, dcnt, doff, dw};

    // RoPE tables: cos/sin computed in fp32 and cast to the activation dtype (modeling_glmasr.py:95-106)
    auto round_act = [&](float x) -> float { return e->f32 ? x : e->dt == DT_F16 ? (float)(_Float16)x : bf16_round_host(x); };
    auto rope_table = [&](int n_pos, int rd, float theta, float** out) -> int {
        const int half = rd / 2;
        std::vector<float> t((size_t)n_pos * rd);
        for (int p = 0; p < n_pos; ++p)
            for (int i = 0; i < half; ++i) {
                const float inv = 1.0f / powf(theta, (float)(2 * i) / (float)rd);
                const float ang = inv * (float)p;
                t[(size_t)p * rd + i] = round_act(cosf(ang));          // `cos.to(dtype=x.dtype)`: bf16 (native), fp16 (int8 / fp16 modes)
                t[(size_t)p * rd + half + i] = round_act(sinf(ang));
            }
        TRY(dalloc(e, out, t.size()));
        HIPC(e, h2d(e, *out, t.data(), t.size() * 4));
        return SONIC_OK;
    };
    if (e->dt == DT_BF16) {
        // GELU of every bf16 value with |x| in [2^-14, 16), computed exactly as the reference op sequence does it in fp32
        // (0.5 * x * (1 + erff(x / sqrt 2)), modeling_glmasr.py:299-300 / torch GELU(approximate="none")) and rounded to bf16 once
        std::vector<unsigned short> lut(GELU_LUT_N);
        for (int sgn = 0; sgn < 2; ++sgn)
            for (int i = 0; i < GELU_LUT_HALF; ++i) {
                const uint32_t bits = ((uint32_t)sgn << 31) | ((uint32_t)((GELU_LUT_E0 << 7) + i) << 16);
                float x; memcpy(&x, &bits, 4);
                const float y = bf16_round_host(0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)));
                uint32_t yb; memcpy(&yb, &y, 4);
                lut[sgn * GELU_LUT_HALF + i] = (unsigned short)(yb >> 16);
            }
        TRY(dalloc(e, &e->gelu_lut, GELU_LUT_N));
        HIPC(e, h2d(e, e->gelu_lut, lut.data(), GELU_LUT_N * 2));
    }
    TRY(rope_table(e->T, d.enc_rotary_dim, d.enc_theta, &e->enc_cs));
    TRY(rope_table(e->max_ctx, d.dec_head_dim, d.dec_theta, &e->dec_cs));
    return SONIC_OK;
}

// ------------------------------------------------------------------------------------------ create / destroy
// The HIP runtime spreads a process's streams over GPU_MAX_HW_QUEUES hardware queues (default 4), round-robin in creation order; streams that
// share a queue execute in order.  A handle owns ONE stream (finished rows leave through a pinned mirror, engine_service.cpp: the fetch stream every decoding
// handle had is gone), so a bulk pipeline of D decoding + P prefill handles owns D + P streams and the default 3x64+1 fits four queues: 4 and 8 queues measure
// the same there (profiles/hwq4_pipeline_ab.txt).  More handles than queues, or device rings, resampler and VAD streams beside them, still alias: when every
// handle also had a fetch stream, the prefill slot's stream landed on the queue of a decoding handle and the bulk pipeline lost 7 % (141 vs 151
// segments/s, profiles/round4_hw_queues.txt).  The runtime reads the variable once, at its first call, so it is the HOST PROCESS that has to set GPU_MAX_HW_QUEUES=8
// before anything touches HIP (`import sonicscribe_amd` and bench.py do it with setdefault).  The library itself no longer writes the
// environment (round 4's constructor did: setenv from a library constructor races with other threads' getenv and silently did nothing when torch
// had started the runtime first).  Instead the first sonic_create on a device MEASURES how many hardware queues the process really has and says so
// once on stderr when there are fewer than the pipeline wants; sonic_runtime_info reports the same numbers to the host.
#define SONIC_HW_QUEUES_WANTED 8
__global__ void hwq_probe_kernel(unsigned long long ticks) {      // spins for `ticks` of the 100 MHz constant clock (s_memrealtime)
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
static std::mutex g_hwq_mu;
static int g_hwq_measured[64];                                      // per device: 0 = not probed yet
// Eight streams each get one single-wave kernel that spins 300 us; streams that share a hardware queue run in order, so the wall time of the eight
// is ceil(8 / queues) x 300 us.  Run once per device and process (about 1 ms), before the engine creates its own streams; the probe streams are
// created and destroyed in one go (a multiple of every plausible queue count, so the runtime's round-robin hand-out is where it was).
static int probe_hw_queues(int device) {
    std::lock_guard<std::mutex> lk(g_hwq_mu);
    if (device < 0 || device >= 64) return 0;
    if (g_hwq_measured[device]) return g_hwq_measured[device];
    int cur = 0; (void)hipGetDevice(&cur);
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return 0; }
    constexpr int NS = 8; constexpr unsigned long long TICKS = 30000;   // 300 us
    hipStream_t st[NS] = {};
    int made = 0, q = 0;
    for (; made < NS; ++made) if (hipStreamCreateWithFlags(&st[made], hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
    if (made == NS) {
        double best = 1e30;
        for (int rep = 0; rep < 3; ++rep) {                           // rep 0 also loads the code object
            for (int i = 0; i < NS; ++i) (void)hipStreamSynchronize(st[i]);
            const auto t0 = std::chrono::steady_clock::now();
            for (int i = 0; i < NS; ++i) hipLaunchKernelGGL(hwq_probe_kernel, dim3(1), dim3(64), 0, st[i], rep == 0 ? 100ull : TICKS);
            for (int i = 0; i < NS; ++i) (void)hipStreamSynchronize(st[i]);
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (rep > 0 && us < best) best = us;
        }
        const double rounds = (best - 40.0) / (TICKS / 100.0);        // ~40 us of launch + synchronise overhead
        int r = (int)(rounds + 0.5); if (r < 1) r = 1; if (r > NS) r = NS;
        q = (NS + r - 1) / r;                                          // 1 round: >= 8 queues, 2 rounds: 4, 4 rounds: 2, 8 rounds: 1
        if (hipGetLastError() != hipSuccess) q = 0;
    }
    for (int i = 0; i < made; ++i) (void)hipStreamDestroy(st[i]);
    (void)hipSetDevice(cur);
    g_hwq_measured[device] = q;
    if (q > 0 && q < SONIC_HW_QUEUES_WANTED && !getenv("SONIC_QUIET")) {
        const char* env = getenv("GPU_MAX_HW_QUEUES");
        fprintf(stderr, "[sonic_hip] device %d: the HIP runtime of this process has %d hardware queue(s) for its streams (GPU_MAX_HW_QUEUES=%s%s); an engine with "
                        "slots, device rings and VAD wants %d - streams that share a queue run in order, and every handle, ring and VAD owns one (a bulk pipeline of D decoding + "
                        "P prefill handles alone needs D + P: the default 3x64+1 fits 4).  Set "
                        "GPU_MAX_HW_QUEUES=8 in the environment BEFORE the process first touches HIP / torch.cuda.\n", device, q, env ? env : "unset",
                env && atoi(env) >= SONIC_HW_QUEUES_WANTED ? ": set after the runtime had started" : "", SONIC_HW_QUEUES_WANTED);
    }
    return q;
}
extern "C" int sonic_runtime_info(int device_id, int32_t* hw_queues, int32_t* hw_queues_env, int32_t* hw_queues_wanted) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) { (void)hipGetLastError(); return fail(nullptr, SONIC_ERR_INVALID, "device %d not available", device_id); }
    if (hw_queues) *hw_queues = probe_hw_queues(device_id);
    if (hw_queues_env) { const char* v = getenv("GPU_MAX_HW_QUEUES"); *hw_queues_env = v ? atoi(v) : 0; }
    if (hw_queues_wanted) *hw_queues_wanted = SONIC_HW_QUEUES_WANTED;
    return SONIC_OK;
}

extern "C" int sonic_abi_version(void) { return SONIC_ABI_VERSION; }
extern "C" int sonic_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

static int check_dims(const sonic_dims& d, int max_batch, int max_ctx, int mode) {
    if (d.n_mels <= 0 || d.n_mels % 64 != 0) return fail(nullptr, SONIC_ERR_INVALID, "n_mels must be a positive multiple of 64");
    if (d.enc_d % 64 || d.enc_ff % 64 || d.dec_d % 256 || d.dec_ff % 256) return fail(nullptr, SONIC_ERR_INVALID, "hidden sizes must be multiples of 64 (encoder) / 256 (decoder)");
    if (d.enc_d / d.enc_heads != 64 || d.enc_d % d.enc_heads) return fail(nullptr, SONIC_ERR_INVALID, "encoder head_dim must be 64");
    if (d.dec_head_dim != 128) return fail(nullptr, SONIC_ERR_INVALID, "decoder head_dim must be 128");
    if (d.enc_rotary_dim % 16 || d.enc_rotary_dim > 64) return fail(nullptr, SONIC_ERR_INVALID, "encoder rotary dim must be a multiple of 16");
    if (d.dec_heads % d.dec_kv_heads || d.dec_heads / d.dec_kv_heads > 4) return fail(nullptr, SONIC_ERR_INVALID, "GQA group must divide and be <= 4");
    if (d.vocab % 64) return fail(nullptr, SONIC_ERR_INVALID, "vocab must be a multiple of 64");
    if (d.enc_T * 2 != d.n_frames || d.enc_T % d.merge || d.enc_T % 4) return fail(nullptr, SONIC_ERR_INVALID, "enc_T must be n_frames/2 and divisible by merge and 4");
    if ((2 * d.enc_d) % 128) return fail(nullptr, SONIC_ERR_INVALID, "2*enc_d must be a multiple of 128");
    if (max_batch < 1 || max_batch > 64) return fail(nullptr, SONIC_ERR_INVALID, "max_batch must be in 1..64");
    if (max_ctx < 64 || max_ctx % 64 || max_ctx > 8192) return fail(nullptr, SONIC_ERR_INVALID, "max_ctx must be a multiple of 64 in 64..8192");
    if (d.n_eos < 0 || d.n_eos > 8) return fail(nullptr, SONIC_ERR_INVALID, "n_eos must be 0..8");
    {   // every decode-step GEMM needs a weight-streaming tiling with 1..8 K slabs (a shape without one would silently produce zeros)
        const int QD = d.dec_heads * d.dec_head_dim, KD = d.dec_kv_heads * d.dec_head_dim;
        const int shapes[5][2] = {{QD + 2 * KD, d.dec_d}, {d.dec_d, QD}, {2 * d.dec_ff, d.dec_d}, {d.dec_d, d.dec_ff}, {d.vocab, d.dec_d}};
        const char* names[5] = {"qkv_proj", "o_proj", "gate/up_proj", "down_proj", "lm_head"};
        for (int i = 0; i < 5; ++i) {
            const int ks = (mode == SONIC_MODE_INT8 && i < 4) ? skinny_pick_ksplit_i8(shapes[i][0], shapes[i][1]) : skinny_pick_ksplit(shapes[i][0], shapes[i][1]);
            if (ks < 1 || ks > 8) return fail(nullptr, SONIC_ERR_INVALID, "decoder %s shape [%d x %d] has no decode-step tiling (K slabs = %d, need 1..8)", names[i], shapes[i][0], shapes[i][1], ks);
        }
    }
    return SONIC_OK;
}

// The main stream of a handle.  Experiments (tools/ab_stream_partition.sh, `make SONIC_AB=1` builds only): SONIC_EXP_PRIO / SONIC_EXP_CUS are comma lists indexed by the order in
// which this process created its handles - a stream priority (-1 high .. 1 low), or "lo-hi" = the CUs the handle's kernels may run on.
static hipError_t create_stream(hipStream_t* st) {
#ifdef SONIC_AB      // measured and lost (profiles/round4_stream_partition.txt): priorities change nothing, CU masks cost 19 .. 42 %
    static std::atomic<int> created{0};
    const int idx = created.fetch_add(1);
    auto field = [&](const char* env, char* out, size_t cap) -> bool {
        const char* v = getenv(env);
        if (!v) return false;
        for (int i = 0; i < idx && v; ++i) { v = strchr(v, ','); if (v) ++v; }
        if (!v || !*v || *v == ',') return false;
        size_t n = strcspn(v, ","); if (n >= cap) n = cap - 1;
        memcpy(out, v, n); out[n] = 0; return true;
    };
    char buf[64];
    if (field("SONIC_EXP_CUS", buf, sizeof buf)) {
        int lo = 0, hi = 255;
        if (sscanf(buf, "%d-%d", &lo, &hi) == 2 && lo >= 0 && hi >= lo && hi < 256) {
            uint32_t mask[8] = {0};
            for (int c = lo; c <= hi; ++c) mask[c / 32] |= 1u << (c % 32);
            return hipExtStreamCreateWithCUMask(st, 8, mask);
        }
    }
    if (field("SONIC_EXP_PRIO", buf, sizeof buf)) return hipStreamCreateWithPriority(st, hipStreamNonBlocking, atoi(buf));
#endif
    return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}
// Everything an engine (or a slot) owns besides weights and constants: its stream, PCM staging, activation buffers, KV cache, decode-step
// buffers, control words, events.
static int alloc_state(sonic_engine* e) {
    if (hipSetDevice(e->device) != hipSuccess) { e->err = "hipSetDevice failed"; return SONIC_ERR_HIP; }
    // waits sleep instead of spinning (see stream_sync): the runtime's default (hipDeviceScheduleAuto) spins when it sees more CPUs than GPUs
    if (!getenv("SONIC_SPIN_SYNC") && hipSetDeviceFlags(hipDeviceScheduleBlockingSync) != hipSuccess) (void)hipGetLastError();
    if (create_stream(&e->st) != hipSuccess) { e->err = "hipStreamCreate failed"; return SONIC_ERR_HIP; }
    if (!getenv("SONIC_SPIN_SYNC") && hipEventCreateWithFlags(&e->sync_ev, hipEventBlockingSync | hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); e->sync_ev = nullptr; }
    const sonic_dims& d = e->d;
    const int Bm = e->Bm, max_batch = e->Bm, max_ctx = e->max_ctx;
    e->T = d.enc_T; e->Tp = (d.enc_T + T_PAD_ALIGN - 1) / T_PAD_ALIGN * T_PAD_ALIGN; e->Ta = d.enc_T / d.merge; e->hd_e = d.enc_d / d.enc_heads;
    e->QD = d.dec_heads * d.dec_head_dim; e->KD = d.dec_kv_heads * d.dec_head_dim; e->qkvN = e->QD + 2 * e->KD;
    // prompt tokens of one batch: at most Ta audio rows per window plus text; a long max_ctx (multi-window requests) must not
    // multiply every prefill buffer by it
    { const int per = max_ctx < e->Ta + 256 ? max_ctx : e->Ta + 256; e->tok_cap = max_batch * per; }
    e->out_cap = max_ctx;
    const int T = e->T, C = d.enc_d;
    const size_t Mp = (size_t)Bm * T + 128;
    int s;
#define A(x) do { s = (x); if (s != SONIC_OK) return s; } while (0)
    A(dalloc(e, &e->pcm, (size_t)Bm * d.n_frames * 160)); A(dalloc(e, &e->n_samples_d, Bm)); A(dalloc(e, &e->ring_peak, Bm));
    A(dalloc(e, &e->logspec, (size_t)Bm * d.n_frames * d.n_mels)); A(dalloc(e, &e->segmax, Bm));
    A(dalloc(e, &e->feats_fm, (size_t)Bm * (d.n_frames + 2) * d.n_mels + 4096));
    A(dalloc(e, &e->h1, (size_t)Bm * (d.n_frames + 2) * C + 4096));
    A(dalloc(e, &e->x, Mp * C)); A(dalloc(e, &e->ln, Mp * C)); A(dalloc(e, &e->att, Mp * C));
    A(dalloc(e, &e->qk, Mp * 2 * C)); A(dalloc(e, &e->vt, (size_t)Bm * C * e->Tp)); A(dalloc(e, &e->ff, Mp * d.enc_ff));
    A(dalloc(e, &e->ph, ((size_t)Bm * e->Ta + 128) * 2 * d.dec_d)); A(dalloc(e, &e->pe, ((size_t)Bm * e->Ta + 128) * d.dec_d));
    const size_t tc = (size_t)e->tok_cap + 128;
    A(dalloc(e, &e->dx, tc * d.dec_d)); A(dalloc(e, &e->dhn, tc * d.dec_d)); A(dalloc(e, &e->dqkv, tc * e->qkvN));
    A(dalloc(e, &e->dq, tc * e->QD)); A(dalloc(e, &e->datt, tc * e->QD)); A(dalloc(e, &e->dact, tc * d.dec_ff));
    const size_t kvn = (size_t)d.dec_layers * Bm * d.dec_kv_heads * max_ctx * d.dec_head_dim;
    A(dalloc(e, &e->Kc, kvn)); A(dalloc(e, &e->Vc, kvn)); A(dalloc(e, &e->Vts, (size_t)Bm * d.dec_kv_heads * d.dec_head_dim * max_ctx));
    long mx = 2L * d.dec_ff; if (e->qkvN > mx) mx = e->qkvN; if (d.dec_d > mx) mx = d.dec_d;
    e->slabN = mx;
    A(dalloc(e, &e->ssq, (size_t)256 * 64));
    A(dalloc(e, &e->slab, (size_t)8 * 64 * mx)); A(dalloc(e, &e->lslab, (size_t)8 * 64 * d.vocab));
    A(dalloc(e, &e->slab2, (size_t)8 * 16 * d.dec_d)); A(dalloc(e, &e->sx2, (size_t)16 * d.dec_d));
    A(dalloc(e, &e->sx, (size_t)64 * d.dec_d)); A(dalloc(e, &e->shn, (size_t)64 * d.dec_d)); A(dalloc(e, &e->sq, (size_t)64 * e->QD));
    A(dalloc(e, &e->satt, (size_t)64 * e->QD)); A(dalloc(e, &e->sact, (size_t)64 * d.dec_ff));
    A(dalloc(e, &e->kv_len, 64)); A(dalloc(e, &e->tok_pos, 64)); A(dalloc(e, &e->n_new, 64)); A(dalloc(e, &e->finished, 64));
    A(dalloc(e, &e->max_new_d, 64)); A(dalloc(e, &e->n_active, 4)); A(dalloc(e, &e->out_ids, (size_t)64 * e->out_cap));
    A(dalloc(e, &e->step_ctr, 64)); A(dalloc(e, &e->seq_iota, 64)); A(dalloc(e, &e->mirrored, 64));
    if (e->i8) {
        // widest Linear8bitLt input: encoder MLP (enc_ff), projector (enc_d * merge), decoder MLP (dec_ff)
        int kmax = d.enc_ff; if (C * d.merge > kmax) kmax = C * d.merge; if (d.dec_ff > kmax) kmax = d.dec_ff; if (2 * d.dec_d > kmax) kmax = 2 * d.dec_d;
        if (e->QD > kmax) kmax = e->QD;
        e->q_kmax = kmax;
        size_t rows = Mp > tc ? Mp : tc;
        size_t qa_bytes = Mp * (size_t)(d.enc_ff > C * d.merge ? d.enc_ff : C * d.merge);
        if (tc * (size_t)d.dec_ff > qa_bytes) qa_bytes = tc * (size_t)d.dec_ff;
        if (((size_t)Bm * e->Ta + 128) * 2 * d.dec_d > qa_bytes) qa_bytes = ((size_t)Bm * e->Ta + 128) * 2 * d.dec_d;
        A(dalloc(e, &e->qa, qa_bytes + 4096)); A(dalloc(e, &e->q_sca, rows)); A(dalloc(e, &e->q_flags, (size_t)64 * kmax + 64));
        A(dalloc(e, &e->q_oc_cnt, 64)); A(dalloc(e, &e->q_oc_list, (size_t)64 * kmax)); A(dalloc(e, &e->win_req, 64));
        A(dalloc(e, &e->qkv_rm, Mp * 3 * C));
        e->defer_cap = Mp * (size_t)C > tc * (size_t)d.dec_d ? Mp * (size_t)C : tc * (size_t)d.dec_d;
        A(dalloc(e, &e->defer_tmp, e->defer_cap, false));
        A(dalloc(e, &e->hn_q, (size_t)64 * d.dec_d)); A(dalloc(e, &e->att_q, (size_t)64 * e->QD)); A(dalloc(e, &e->act_q, (size_t)64 * d.dec_ff));
        A(dalloc(e, &e->sca_hn, 64)); A(dalloc(e, &e->sca_att, 64)); A(dalloc(e, &e->sca_act, 64));
        A(dalloc(e, &e->oc_hn, 64)); A(dalloc(e, &e->oc_att, 64)); A(dalloc(e, &e->oc_act, 64));
        A(dalloc(e, &e->ol_hn, (size_t)64 * d.dec_d)); A(dalloc(e, &e->ol_att, (size_t)64 * e->QD)); A(dalloc(e, &e->ol_act, (size_t)64 * d.dec_ff));
        A(dalloc(e, &e->ov_hn, (size_t)64 * d.dec_d)); A(dalloc(e, &e->ov_att, (size_t)64 * e->QD)); A(dalloc(e, &e->ov_act, (size_t)64 * d.dec_ff));
        A(dalloc(e, &e->amax_att, 64 * 4)); A(dalloc(e, &e->amax_act, 64 * 4)); A(dalloc(e, &e->big_att, 64 * 4));
    }
    A(dalloc(e, &e->src, tc)); A(dalloc(e, &e->tok_seq, tc)); A(dalloc(e, &e->tok_pos_pf, tc));
    A(dalloc(e, &e->q_off, 64)); A(dalloc(e, &e->q_len, 64)); A(dalloc(e, &e->last_row, 64));
    {
        int iota[64]; for (int i = 0; i < 64; ++i) iota[i] = i;
        if (h2d(e, e->seq_iota, iota, sizeof iota) != hipSuccess) { e->err = "memcpy failed"; return SONIC_ERR_HIP; }
    }
    if (hipHostMalloc((void**)&e->n_active_h, (CHK_RING + 1) * 4, hipHostMallocDefault) != hipSuccess) { e->err = "hipHostMalloc failed"; return SONIC_ERR_HIP; }
    if (hipHostMalloc((void**)&e->svc_h, (size_t)CHK_RING * SVC_WORDS * 4, hipHostMallocDefault) != hipSuccess) { e->err = "hipHostMalloc failed"; return SONIC_ERR_HIP; }
    if (hipEventCreateWithFlags(&e->xfer_ev, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&e->splice_ev, hipEventDisableTiming) != hipSuccess) { e->err = "hipEventCreate failed"; return SONIC_ERR_HIP; }
    e->plan_cap = 3 * tc + 10 * 64;      // (three words per token; seven per request, a word and the 64 of run_upload_win_req behind them)
    for (int i = 0; i < 2; ++i) {
        if (hipHostMalloc((void**)&e->plan_buf[i], e->plan_cap * 4, hipHostMallocDefault) != hipSuccess) { e->err = "hipHostMalloc failed"; return SONIC_ERR_HIP; }
        if (hipEventCreateWithFlags(&e->plan_ev[i], (getenv("SONIC_SPIN_SYNC") ? 0 : hipEventBlockingSync) | hipEventDisableTiming) != hipSuccess) { e->err = "hipEventCreate failed"; return SONIC_ERR_HIP; }
    }
    e->plan_h = e->plan_buf[0];
    for (auto& v : e->ev) if (hipEventCreate(&v) != hipSuccess) { e->err = "hipEventCreate failed"; return SONIC_ERR_HIP; }
    e->gemm_ev.resize(8 * (size_t)(d.enc_layers > 0 ? d.enc_layers : 1));   // per layer: [start, end] of the QKV, o, fc1, fc2 GEMM launches
    for (auto& v : e->gemm_ev) if (hipEventCreate(&v) != hipSuccess) { e->err = "hipEventCreate failed"; return SONIC_ERR_HIP; }
#undef A
    for (auto& v : e->chk_ev) if (hipEventCreateWithFlags(&v, (getenv("SONIC_SPIN_SYNC") ? 0 : hipEventBlockingSync) | hipEventDisableTiming) != hipSuccess) { e->err = "hipEventCreate failed"; return SONIC_ERR_HIP; }
    e->n_samples_h.assign(Bm, 0);
    return SONIC_OK;
}

extern "C" int sonic_create(const sonic_dims* dims, int device_id, int mode, int max_batch, int max_ctx, sonic_engine** out) {
    if (!dims || !out) return fail(nullptr, SONIC_ERR_INVALID, "null argument");
    *out = nullptr;
    if (mode != SONIC_MODE_NATIVE && mode != SONIC_MODE_INT8 && mode != SONIC_MODE_F16 && mode != SONIC_MODE_F32) return fail(nullptr, SONIC_ERR_INVALID, "mode must be either 'native' or 'int8'");
    g_opts = LaunchOpts{};
    TRY(check_dims(*dims, max_batch, max_ctx, mode));
    if (mode == SONIC_MODE_INT8 && (dims->dec_ff > 8192 || dims->enc_d % 128 || dims->enc_ff % 128 || (dims->dec_heads * dims->dec_head_dim) % 128))
        return fail(nullptr, SONIC_ERR_INVALID, "int8 mode: dec_ff must be <= 8192 and every quantised K a multiple of 128");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, SONIC_ERR_HIP, "no HIP device available");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, SONIC_ERR_INVALID, "device %d out of range (%d devices)", device_id, ndev);
    (void)probe_hw_queues(device_id);                     // once per device and process; warns when streams will alias (see sonic_runtime_info)
    sonic_engine* e = new sonic_engine();
    if (const char* v = getenv("SONIC_KEEP_ROWMAJOR")) e->opt_prefill_rowmajor = atoi(v) >= 2;   // =2: keep the row-major decoder weights AND read them (A/B of whole test runs)
    e->d = *dims; e->device = device_id; e->mode = mode; e->Bm = max_batch; e->max_ctx = max_ctx;
    e->i8 = mode == SONIC_MODE_INT8; e->dt = (e->i8 || mode == SONIC_MODE_F16) ? DT_F16 : DT_BF16;
    e->f32 = mode == SONIC_MODE_F32;
    if (e->f32) e->f = new F32State();
    int s = alloc_state(e);
    if (s == SONIC_OK && e->f32) s = f32_alloc(e);
    if (s == SONIC_OK) s = build_constants(e);
    if (s == SONIC_OK && stream_sync(e) != hipSuccess) { e->err = "stream sync failed"; s = SONIC_ERR_HIP; }
    if (s != SONIC_OK) { g_create_err = e->err; sonic_destroy(e); return s; }
    *out = e;
    return SONIC_OK;
}

// Another batch in flight on the SAME weights (what the reference's file mode does in spirit: backend/main.py:429-445 keeps three decodes in
// flight on one model object).  The slot is a full engine handle - stage / run / fetch / rings / options all work on it - with its own stream,
// activation buffers, KV cache, PCM staging and decode graphs; every weight and constant pointer is the owner's, so sonic_weight_bytes of the
// owner does not move and the slot's is 0.  The decode loop is latency-bound: a second batch's MFMA-bound encoder / prefill and its
// decode steps fill the bubbles of the first one's.  Slots die with their owner at the latest; sonic_destroy(slot) releases one early.
extern "C" int sonic_slot_create(sonic_engine* parent, sonic_engine** out) {
    if (!parent || !out) return fail(nullptr, SONIC_ERR_INVALID, "null argument");
    *out = nullptr;
    sonic_engine* root = parent->owner ? parent->owner : parent;
    std::lock_guard<std::mutex> lk(root->mu);
    (void)hipGetLastError();
    if (!root->finalized) return fail(nullptr, SONIC_ERR_INVALID, "sonic_slot_create needs an engine whose weights are finalized");
    if (root->f32) return fail(nullptr, SONIC_ERR_UNSUPPORTED, "SONIC_MODE_F32 is a test kind: no slots");
    g_opts = root->opts;
    sonic_engine* e = new sonic_engine();
    e->d = root->d; e->device = root->device; e->mode = root->mode; e->Bm = root->Bm; e->max_ctx = root->max_ctx; e->i8 = root->i8; e->dt = root->dt;
    int s = alloc_state(e);
    if (s == SONIC_OK && stream_sync(e) != hipSuccess) { e->err = "stream sync failed"; s = SONIC_ERR_HIP; }
    if (s != SONIC_OK) { g_create_err = e->err; sonic_destroy(e); return s; }
    // the owner's weights and constants, by pointer (read-only on the request path)
    e->conv1w = root->conv1w; e->conv2w = root->conv2w; e->conv1b = root->conv1b; e->conv2b = root->conv2b;
    e->enc = root->enc; e->enc_nw = root->enc_nw; e->enc_nb = root->enc_nb; e->gelu_lut = root->gelu_lut;
    e->pj1w = root->pj1w; e->pj2w = root->pj2w; e->pj1b = root->pj1b; e->pj2b = root->pj2b; e->qpj1 = root->qpj1; e->qpj2 = root->qpj2;
    e->embed = root->embed; e->embed_t = root->embed_t; e->dec = root->dec; e->dec_nw = root->dec_nw;
    e->lc = root->lc; e->enc_cs = root->enc_cs; e->dec_cs = root->dec_cs;
    e->opts = root->opts; e->opt_no_graph = root->opt_no_graph; e->opt_no_fused_rope = root->opt_no_fused_rope; e->opt_no_gelu_lut = root->opt_no_gelu_lut;
    e->opt_i8_defer_thr = root->opt_i8_defer_thr; e->opt_i8_no_xq = root->opt_i8_no_xq; e->opt_i8_no_lnq = root->opt_i8_no_lnq; e->opt_i8_no_qkv_fuse = root->opt_i8_no_qkv_fuse;
    e->opt_decode_chunk = root->opt_decode_chunk; e->opt_no_pre_norm = root->opt_no_pre_norm; e->opt_decode_gemv = root->opt_decode_gemv; e->opt_fetch_stream = root->opt_fetch_stream;
    e->opt_fp8_weights = root->opt_fp8_weights; e->opt_fp8_chain = root->opt_fp8_chain; e->embed8 = root->embed8; e->embed_sc = root->embed_sc;      // mode fp8: the owner's e4m3 copies (the layers' ride in `dec`)
    if ((s = gen_inherit(e, root)) != SONIC_OK) { g_create_err = e->err; sonic_destroy(e); return s; }      // the owner's generation options, with their buffers
    e->weight_bytes = 0; e->finalized = true; e->owner = root;
    root->slots.push_back(e);
    *out = e;
    return SONIC_OK;
}
// what a caller that was handed engine pointers (sonic_pipeline_create) has to know about them: row capacity, context capacity, mode, device and
// the identity of the weight copy (the owner's address: equal for an engine and all of its slots)
extern "C" int sonic_engine_info(sonic_engine* e, int32_t* max_batch, int32_t* max_ctx, int32_t* mode, int32_t* device_id, const void** weights_id) {
    if (!e) return SONIC_ERR_INVALID;
    if (max_batch) *max_batch = e->Bm;
    if (max_ctx) *max_ctx = e->max_ctx;
    if (mode) *mode = e->mode;
    if (device_id) *device_id = e->device;
    if (weights_id) *weights_id = e->owner ? (const void*)e->owner : (const void*)e;
    return SONIC_OK;
}
extern "C" int sonic_slot_count(sonic_engine* e) {
    if (!e) return 0;
    sonic_engine* root = e->owner ? e->owner : e;
    std::lock_guard<std::mutex> lk(root->mu);
    return 1 + (int)root->slots.size();
}

extern "C" void sonic_destroy(sonic_engine* e) {
    if (!e) return;
    async_shutdown(e);                                   // the worker of sonic_run_staged_async finishes its batch and exits
    if (e->owner) {                                      // a slot leaves its owner's list (under the owner's lock: sonic_slot_create / sonic_slot_count walk it)
        std::lock_guard<std::mutex> lk(e->owner->mu);
        auto& v = e->owner->slots;
        v.erase(std::remove(v.begin(), v.end(), e), v.end());
    } else {
        std::vector<sonic_engine*> kids;
        { std::lock_guard<std::mutex> lk(e->mu); kids.swap(e->slots); }
        for (sonic_engine* k : kids) { k->owner = nullptr; k->finalized = false; sonic_destroy(k); }   // slots first: they read this engine's weights
    }
    (void)hipSetDevice(e->device);
    if (e->st) (void)stream_sync(e);
    if (e->splice_ev) {                                // a sibling that prefilled for this handle must not wait for an event that is about to be destroyed
        sonic_engine* root = e->owner ? e->owner : e;  // (the stream was just drained: every splice this handle queued has completed)
        std::lock_guard<std::mutex> lk(root->mu);
        if (root != e && root->wait_ev == e->splice_ev) root->wait_pending = false;
        for (sonic_engine* k : root->slots) if (k != e && k->wait_ev == e->splice_ev) k->wait_pending = false;
    }
    gen_release(e);                                    // the per-request stages' mirrors, the grammar references this handle holds, an owner's grammars
    for (sonic_ring* r : e->rings) ring_free(r);       // rings the caller left behind go with their engine
    e->rings.clear();
    resample_release(e);
    for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.second);
    for (void* p : e->allocs) (void)hipFree(p);
    if (e->dump) (void)hipFree(e->dump);
    if (e->force_d) (void)hipFree(e->force_d);
    if (e->taps) (void)hipFree(e->taps);
    if (e->feats_f32) (void)hipFree(e->feats_f32);
    if (e->n_active_h) (void)hipHostFree(e->n_active_h);
    for (int i = 0; i < 2; ++i) { if (e->plan_buf[i]) (void)hipHostFree(e->plan_buf[i]); if (e->plan_ev[i]) (void)hipEventDestroy(e->plan_ev[i]); }
    if (e->svc_h) (void)hipHostFree(e->svc_h);
    if (e->svc_out_h) (void)hipHostFree(e->svc_out_h);
    if (e->svc_lp_h) (void)hipHostFree(e->svc_lp_h);
    if (e->score_plan_h) (void)hipHostFree(e->score_plan_h);
    if (e->align_plan_h) (void)hipHostFree(e->align_plan_h);
    if (e->st_io) { (void)hipStreamSynchronize(e->st_io); (void)hipStreamDestroy(e->st_io); }      // (only a handle that fetched with option fetch_stream has one)
    if (e->xfer_ev) (void)hipEventDestroy(e->xfer_ev);
    if (e->splice_ev) (void)hipEventDestroy(e->splice_ev);
    for (auto& v : e->ev) if (v) (void)hipEventDestroy(v);
    for (auto& v : e->chk_ev) if (v) (void)hipEventDestroy(v);
    if (e->sync_ev) (void)hipEventDestroy(e->sync_ev);
    for (auto& v : e->gemm_ev) if (v) (void)hipEventDestroy(v);
    if (e->st) (void)hipStreamDestroy(e->st);
    delete e->f;                                        // (its device buffers were in e->allocs)
    delete e;
}

extern "C" const char* sonic_last_error(sonic_engine* e) { return e ? e->err.c_str() : g_create_err.c_str(); }
extern "C" int64_t sonic_weight_bytes(sonic_engine* e) { return e ? e->weight_bytes : 0; }
extern "C" int sonic_synchronize(sonic_engine* e) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    HIPC(e, stream_sync(e));
    return SONIC_OK;
}

// what ASRModel.get_model_info() reads from torch.cuda (asr.py:501-506: version, device name, total memory) ...
extern "C" int sonic_device_info(int device_id, char* name, int name_cap, int64_t* total_bytes, int64_t* free_bytes, int32_t* hip_runtime_version) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) { (void)hipGetLastError(); return fail(nullptr, SONIC_ERR_INVALID, "device %d not available", device_id); }
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, device_id) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, SONIC_ERR_HIP, "hipGetDeviceProperties failed"); }
    if (name && name_cap > 0) { snprintf(name, (size_t)name_cap, "%s", pr.name[0] ? pr.name : pr.gcnArchName); }   // (some boxes of the pool report an empty marketing name)
    if (total_bytes) *total_bytes = (int64_t)pr.totalGlobalMem;
    if (free_bytes) {
        size_t fr = 0, tot = 0; int cur = 0;
        (void)hipGetDevice(&cur);
        if (hipSetDevice(device_id) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); fr = 0; }
        (void)hipSetDevice(cur);
        *free_bytes = (int64_t)fr;
    }
    if (hip_runtime_version) { int v = 0; if (hipRuntimeGetVersion(&v) != hipSuccess) { (void)hipGetLastError(); v = 0; } *hip_runtime_version = v; }
    return SONIC_OK;
}
// ... and what the debug dict of transcribe() reads from the caching allocator (asr.py:453-457): allocated = bytes in this handle's live
// device allocations (weights, activations, KV cache; rings excluded; a slot: its own buffers, the weights are its owner's); there is no
// caching layer under the engine, so reserved = allocated
extern "C" int sonic_memory_info(sonic_engine* e, int64_t* allocated_bytes, int64_t* reserved_bytes) {
    if (!e) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    const int64_t live = e->alloc_bytes + (e->owner ? 0 : e->ring_bytes.load() + e->gram_bytes.load());      // rings and grammars are charged to the weight owner that registers them
    if (allocated_bytes) *allocated_bytes = live;
    if (reserved_bytes) *reserved_bytes = live;
    return SONIC_OK;
}
