// sonic_hip engine: the resampler's host side (kernel: resample.hip).  The coefficient banks, cached per rate pair on the weight owner and
// shared by its slots and rate rings (engine_ingest.cpp), and sonic_resample, the one-shot entry over a whole host buffer.
#include "engine_internal.h"

// The bank of torchaudio's sinc_interp_hann kernel (lowpass_filter_width 6, rolloff 0.99), the arithmetic of
// sonicscribe_amd/frontend.py resample_bank step by step in double, rounded once to fp32; [K][nf] on the device.
static void build_bank(int of, int nf, int width, int K, std::vector<float>& bank) {
    const double lpw = 6.0, base = (double)(of < nf ? of : nf) * 0.99, scale = base / (double)of;
    bank.resize((size_t)K * nf);
    for (int p = 0; p < nf; ++p)
        for (int k = 0; k < K; ++k) {
            double t = ((double)(-p) / (double)nf + (double)(k - width) / (double)of) * base;
            t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
            const double c = cos(t * M_PI / lpw / 2.0), window = c * c;
            t = t * M_PI;
            const double kern = t == 0.0 ? 1.0 : sin(t) / t;
            bank[(size_t)k * nf + p] = (float)(kern * window * scale);
        }
}

static int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

static int bank_get_locked(sonic_engine* root, int64_t in_rate, int64_t out_rate, RsBank* out, std::string& err) {
    char msg[256];
    if (in_rate <= 0 || out_rate <= 0) {
        snprintf(msg, sizeof msg, "resampler: sampling rates must be positive (got %lld -> %lld Hz)", (long long)in_rate, (long long)out_rate);
        err = msg; return SONIC_ERR_INVALID;
    }
    const int64_t g = gcd64(in_rate, out_rate), of = in_rate / g, nf = out_rate / g;
    const double base = (double)(of < nf ? of : nf) * 0.99;
    const int64_t width = (int64_t)ceil(6.0 * (double)of / base), K = 2 * width + of;
    if (of > RS_BANK_MAX_COEF || nf > RS_BANK_MAX_COEF || nf * K > RS_BANK_MAX_COEF) {
        snprintf(msg, sizeof msg, "resampler: %lld -> %lld Hz needs a bank of %lld phases x %lld taps = %.0f coefficients (limit %lld)", (long long)in_rate,
                 (long long)out_rate, (long long)nf, (long long)K, (double)nf * (double)K, (long long)RS_BANK_MAX_COEF);
        err = msg; return SONIC_ERR_INVALID;
    }
    auto it = root->rs_banks.find({(int)of, (int)nf});
    if (it != root->rs_banks.end()) { *out = it->second; return SONIC_OK; }
    RsBank b; b.of = (int)of; b.nf = (int)nf; b.width = (int)width; b.K = (int)K;
    resample_plan(b.of, b.nf, b.K, &b.tile, &b.kc);
    std::vector<float> h;
    build_bank(b.of, b.nf, b.width, b.K, h);
    hipError_t er = hipMalloc((void**)&b.dev, h.size() * 4);
    if (er == hipSuccess) er = hipMemcpy(b.dev, h.data(), h.size() * 4, hipMemcpyHostToDevice);   // complete on return: every stream may read it
    if (er != hipSuccess) {
        (void)hipGetLastError();
        if (b.dev) (void)hipFree(b.dev);
        err = std::string("resampler: bank upload failed: ") + hipGetErrorString(er);
        return er == hipErrorOutOfMemory ? SONIC_ERR_OOM : SONIC_ERR_HIP;
    }
    root->ring_bytes += (int64_t)h.size() * 4;
    root->rs_banks[{b.of, b.nf}] = b;
    *out = b;
    return SONIC_OK;
}
int resample_bank_get(sonic_engine* root, int64_t in_rate, int64_t out_rate, RsBank* out, std::string& err) {
    std::lock_guard<std::mutex> lk(root->rs_mu);
    return bank_get_locked(root, in_rate, out_rate, out, err);
}
void resample_release(sonic_engine* e) {
    for (auto& kv : e->rs_banks) (void)hipFree(kv.second.dev);
    e->rs_banks.clear();
    if (e->rs_st) { (void)hipStreamSynchronize(e->rs_st); (void)hipStreamDestroy(e->rs_st); e->rs_st = nullptr; }
    if (e->rs_in) (void)hipFree(e->rs_in);
    if (e->rs_out) (void)hipFree(e->rs_out);
    e->rs_in = nullptr; e->rs_out = nullptr;
}

// torchaudio.transforms.Resample(in_rate, out_rate)(wav) of backend/asr.py:255-261 over one whole buffer (zeros beyond both ends, trimmed to
// ceil(nf * n / of) outputs).  Its own lock and stream: it never takes the engine's batch lock, so it never queues behind a decode.
// Errors go to sonic_last_error(NULL) of the calling thread.
extern "C" int sonic_resample(sonic_engine* e, const int16_t* pcm_i16, const float* pcm_f32, int64_t n, int32_t in_rate, int32_t out_rate,
                              float* out_f32, int64_t out_cap, int64_t* n_out) {
    if (!e) return fail(nullptr, SONIC_ERR_INVALID, "sonic_resample: null engine");
    if (n < 0 || n > ((int64_t)1 << 34)) return fail(nullptr, SONIC_ERR_INVALID, "sonic_resample: sample count %lld out of range", (long long)n);
    if ((pcm_i16 != nullptr) == (pcm_f32 != nullptr) && n > 0) return fail(nullptr, SONIC_ERR_INVALID, "sonic_resample: exactly one of the int16 and the fp32 input is given");
    sonic_engine* root = e->owner ? e->owner : e;
    std::lock_guard<std::mutex> lk(root->rs_mu);
    (void)hipGetLastError();
    auto hip_fail = [&](const char* what, hipError_t er) {
        (void)hipGetLastError();
        return fail(nullptr, er == hipErrorOutOfMemory ? SONIC_ERR_OOM : SONIC_ERR_HIP, "sonic_resample: %s failed: %s", what, hipGetErrorString(er));
    };
    hipError_t er = hipSetDevice(root->device);
    if (er != hipSuccess) return hip_fail("hipSetDevice", er);
    if (in_rate <= 0 || out_rate <= 0) return fail(nullptr, SONIC_ERR_INVALID, "resampler: sampling rates must be positive (got %d -> %d Hz)", in_rate, out_rate);
    if (in_rate == out_rate) {                       // Resample with equal rates returns its input
        if (n_out) *n_out = n;
        if (!out_f32) return SONIC_OK;
        if (out_cap < n) return fail(nullptr, SONIC_ERR_INVALID, "sonic_resample: %lld outputs do not fit the buffer of %lld", (long long)n, (long long)out_cap);
        for (int64_t i = 0; i < n; ++i) out_f32[i] = pcm_f32 ? pcm_f32[i] : (float)pcm_i16[i] * (1.0f / 32768.0f);
        return SONIC_OK;
    }
    RsBank b; std::string err;
    const int rc = bank_get_locked(root, in_rate, out_rate, &b, err);
    if (rc != SONIC_OK) return fail(nullptr, rc, "%s", err.c_str());
    const int64_t total = (b.nf * n + b.of - 1) / b.of;
    if (n_out) *n_out = total;
    if (!out_f32 || total == 0) return SONIC_OK;     // a null output asks for the count only
    if (out_cap < total) return fail(nullptr, SONIC_ERR_INVALID, "sonic_resample: %lld outputs do not fit the buffer of %lld", (long long)total, (long long)out_cap);
    if (!root->rs_st && (er = hipStreamCreateWithFlags(&root->rs_st, hipStreamNonBlocking)) != hipSuccess) return hip_fail("hipStreamCreateWithFlags", er);
    const size_t in_bytes = (size_t)n * (pcm_f32 ? 4 : 2), out_bytes = (size_t)total * 4;
    if (in_bytes > root->rs_in_cap) {                // the stream is idle between calls: every call ends with a synchronise
        if (root->rs_in) { (void)hipFree(root->rs_in); root->ring_bytes -= (int64_t)root->rs_in_cap; root->rs_in = nullptr; root->rs_in_cap = 0; }
        if ((er = hipMalloc(&root->rs_in, in_bytes)) != hipSuccess) return hip_fail("hipMalloc (input)", er);
        root->rs_in_cap = in_bytes; root->ring_bytes += (int64_t)in_bytes;
    }
    if (out_bytes > root->rs_out_cap) {
        if (root->rs_out) { (void)hipFree(root->rs_out); root->ring_bytes -= (int64_t)root->rs_out_cap; root->rs_out = nullptr; root->rs_out_cap = 0; }
        if ((er = hipMalloc((void**)&root->rs_out, out_bytes)) != hipSuccess) return hip_fail("hipMalloc (output)", er);
        root->rs_out_cap = out_bytes; root->ring_bytes += (int64_t)out_bytes;
    }
    if ((er = hipMemcpyAsync(root->rs_in, pcm_f32 ? (const void*)pcm_f32 : (const void*)pcm_i16, in_bytes, hipMemcpyHostToDevice, root->rs_st)) != hipSuccess)
        return hip_fail("hipMemcpyAsync (input)", er);
    ResampleArgs a{};
    a.src = root->rs_in; a.src_base = 0; a.src_n = n;
    a.bank = b.dev; a.of = b.of; a.nf = b.nf; a.width = b.width; a.K = b.K; a.tile = b.tile; a.kc = b.kc;
    a.j0 = 0; a.n_out = total; a.out_f32 = root->rs_out;
    launch_resample(a, pcm_f32 != nullptr, root->rs_st);
    if ((er = hipGetLastError()) != hipSuccess) return hip_fail("resample kernel launch", er);
    if ((er = hipMemcpyAsync(out_f32, root->rs_out, out_bytes, hipMemcpyDeviceToHost, root->rs_st)) != hipSuccess) return hip_fail("hipMemcpyAsync (output)", er);
    if ((er = hipStreamSynchronize(root->rs_st)) != hipSuccess) return hip_fail("hipStreamSynchronize", er);
    return SONIC_OK;
}
