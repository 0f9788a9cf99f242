// C ABI of the Silero VAD network (sonic_vad_* in include/sonic_hip.h): a handle of its own, with its own stream, lock, weights and
// buffers.  It does not hang off sonic_engine: the reference builds the VAD apart from the ASR model (models_manager.py:34-49) and a
// VAD call must not queue behind a decoding batch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>
#include "vad_dev.h"
#include "ring_access.h"
#include "../../include/sonic_hip.h"

namespace {

struct TensorSpec {
    const char* name;
    int ndim;
    int64_t shape[3];
    bool transpose;       // [shape0][rest] -> [rest][shape0]
};

// the layer table of sonicscribe_amd/vad_net.py (names after the `_model.` prefix of load_silero_vad()'s state dict)
const TensorSpec kTensors[] = {
    {"stft.forward_basis_buffer", 3, {258, 1, 256}, true},
    {"encoder.0.reparam_conv.weight", 3, {128, 129, 3}, true}, {"encoder.0.reparam_conv.bias", 1, {128}, false},
    {"encoder.1.reparam_conv.weight", 3, {64, 128, 3}, true},  {"encoder.1.reparam_conv.bias", 1, {64}, false},
    {"encoder.2.reparam_conv.weight", 3, {64, 64, 3}, true},   {"encoder.2.reparam_conv.bias", 1, {64}, false},
    {"encoder.3.reparam_conv.weight", 3, {128, 64, 3}, true},  {"encoder.3.reparam_conv.bias", 1, {128}, false},
    {"decoder.rnn.weight_ih", 2, {512, 128}, true}, {"decoder.rnn.bias_ih", 1, {512}, false},
    {"decoder.rnn.bias_hh", 1, {512}, false},       {"decoder.rnn.weight_hh", 2, {512, 128}, false},
    {"decoder.decoder.2.weight", 3, {1, 128, 1}, false}, {"decoder.decoder.2.bias", 1, {1}, false},
};
constexpr int kNT = sizeof(kTensors) / sizeof(kTensors[0]);

int64_t numel(const TensorSpec& t) {
    int64_t n = 1;
    for (int i = 0; i < t.ndim; ++i) n *= t.shape[i];
    return n;
}

thread_local std::string g_create_err;

}  // namespace

struct sonic_vad {
    int dev = 0;
    hipStream_t st = nullptr;
    std::mutex mu;
    std::string err;
    float* d_w = nullptr;
    int64_t off[kNT] = {};
    bool loaded[kNT] = {};
    // one upload blob [pcm | windows | seq_base] (pinned mirror h_up), gate inputs and probabilities; all grow on demand
    char *d_up = nullptr, *h_up = nullptr;
    size_t up_cap = 0;
    float *d_gin = nullptr, *d_probs = nullptr, *h_probs = nullptr;
    int64_t win_cap = 0;
    hipEvent_t front_ev = nullptr;      // behind the front kernel of a ring call: the ring locks go back when it has completed
};

static int fail(sonic_vad* v, int code, const std::string& msg) {
    v->err = msg;
    return code;
}

static int hip_fail(sonic_vad* v, hipError_t e, const char* what) {
    return fail(v, e == hipErrorOutOfMemory ? SONIC_ERR_OOM : SONIC_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

static hipError_t grow_windows(sonic_vad* v, int64_t W) {
    if (W <= v->win_cap) return hipSuccess;
    const int64_t cap = std::max<int64_t>(W, v->win_cap * 3 / 2);
    (void)hipFree(v->d_gin); (void)hipFree(v->d_probs); (void)hipHostFree(v->h_probs);
    v->d_gin = v->d_probs = v->h_probs = nullptr;
    v->win_cap = 0;
    hipError_t e;
    if ((e = hipMalloc(&v->d_gin, cap * VAD_GATES * sizeof(float))) != hipSuccess) return e;
    if ((e = hipMalloc(&v->d_probs, cap * sizeof(float))) != hipSuccess) return e;
    if ((e = hipHostMalloc(&v->h_probs, cap * sizeof(float))) != hipSuccess) return e;
    v->win_cap = cap;
    return hipSuccess;
}

static hipError_t grow_upload(sonic_vad* v, size_t bytes) {
    if (bytes <= v->up_cap) return hipSuccess;
    const size_t cap = std::max(bytes, v->up_cap * 3 / 2);
    (void)hipFree(v->d_up); (void)hipHostFree(v->h_up);
    v->d_up = v->h_up = nullptr;
    v->up_cap = 0;
    hipError_t e;
    if ((e = hipMalloc(&v->d_up, cap)) != hipSuccess) return e;
    if ((e = hipHostMalloc(&v->h_up, cap)) != hipSuccess) return e;
    v->up_cap = cap;
    return hipSuccess;
}

static VadWeights device_weights(const sonic_vad* v) {
    VadWeights wt;
    const float** p[] = {&wt.basisT, &wt.w0T, &wt.b0, &wt.w1T, &wt.b1, &wt.w2T, &wt.b2, &wt.w3T, &wt.b3,
                               &wt.wihT, &wt.bih, &wt.bhh, &wt.whh, &wt.hw, &wt.hb};
    for (int i = 0; i < kNT; ++i) *p[i] = v->d_w + v->off[i];
    return wt;
}

extern "C" {

SONIC_API int sonic_vad_create(int device_id, int max_windows, sonic_vad** out) {
    if (!out) { g_create_err = "sonic_vad_create: out is NULL"; return SONIC_ERR_INVALID; }
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { g_create_err = "sonic_vad_create: no HIP device"; return SONIC_ERR_HIP; }
    if (device_id < 0 || device_id >= n || max_windows < 0) {
        g_create_err = "sonic_vad_create: device_id " + std::to_string(device_id) + " / max_windows " + std::to_string(max_windows) + " out of range";
        return SONIC_ERR_INVALID;
    }
    sonic_vad* v = new sonic_vad();
    v->dev = device_id;
    hipError_t e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&v->st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&v->front_ev, hipEventDisableTiming);
    int64_t total = 0;
    for (int i = 0; i < kNT; ++i) { v->off[i] = total; total += (numel(kTensors[i]) + 3) / 4 * 4; }   // 16-byte aligned tensors
    if (e == hipSuccess) e = hipMalloc(&v->d_w, total * sizeof(float));
    if (e == hipSuccess) e = grow_windows(v, max_windows);
    if (e == hipSuccess) e = grow_upload(v, (size_t)max_windows * (VAD_NEW * sizeof(int16_t) + sizeof(VadWindow) + sizeof(int64_t)) + 64);
    if (e != hipSuccess) {
        g_create_err = std::string("sonic_vad_create: ") + hipGetErrorString(e);
        const int code = e == hipErrorOutOfMemory ? SONIC_ERR_OOM : SONIC_ERR_HIP;
        sonic_vad_destroy(v);
        return code;
    }
    *out = v;
    return SONIC_OK;
}

SONIC_API void sonic_vad_destroy(sonic_vad* v) {
    if (!v) return;
    (void)hipSetDevice(v->dev);
    if (v->st) (void)hipStreamSynchronize(v->st);
    (void)hipFree(v->d_w); (void)hipFree(v->d_gin); (void)hipFree(v->d_probs); (void)hipFree(v->d_up);
    (void)hipHostFree(v->h_probs); (void)hipHostFree(v->h_up);
    if (v->front_ev) (void)hipEventDestroy(v->front_ev);
    if (v->st) (void)hipStreamDestroy(v->st);
    delete v;
}

SONIC_API const char* sonic_vad_last_error(sonic_vad* v) {
    return v ? v->err.c_str() : g_create_err.c_str();
}

SONIC_API int sonic_vad_load_tensor(sonic_vad* v, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!v) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(v->mu);
    if (!name || !data || (ndim > 0 && !shape)) return fail(v, SONIC_ERR_INVALID, "sonic_vad_load_tensor: NULL argument");
    int idx = -1;
    for (int i = 0; i < kNT; ++i)
        if (!strcmp(kTensors[i].name, name)) idx = i;
    if (idx < 0) return fail(v, SONIC_ERR_INVALID, std::string("sonic_vad_load_tensor: unknown tensor ") + name);
    const TensorSpec& t = kTensors[idx];
    bool ok = ndim == t.ndim;
    for (int i = 0; ok && i < ndim; ++i) ok = shape[i] == t.shape[i];
    if (!ok) {
        std::string want = "[", got = "[";
        for (int i = 0; i < t.ndim; ++i) want += std::to_string(t.shape[i]) + (i + 1 < t.ndim ? ", " : "");
        for (int i = 0; i < ndim; ++i) got += std::to_string(shape[i]) + (i + 1 < ndim ? ", " : "");
        return fail(v, SONIC_ERR_INVALID, std::string("sonic_vad_load_tensor: ") + name + " has shape " + got + "], expected " + want + "]");
    }
    const int64_t n = numel(t);
    std::vector<float> buf(data, data + n);
    if (t.transpose) {
        const int64_t rows = t.shape[0], cols = n / rows;
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t c = 0; c < cols; ++c) buf[c * rows + r] = data[r * cols + c];
    }
    (void)hipSetDevice(v->dev);
    hipError_t e = hipMemcpyAsync(v->d_w + v->off[idx], buf.data(), n * sizeof(float), hipMemcpyHostToDevice, v->st);
    if (e == hipSuccess) e = hipStreamSynchronize(v->st);
    if (e != hipSuccess) return hip_fail(v, e, "sonic_vad_load_tensor");
    v->loaded[idx] = true;
    return SONIC_OK;
}

SONIC_API int sonic_vad_probs(sonic_vad* v, const int16_t* pcm_i16, const float* pcm_f32, const int64_t* off, int B, float* probs) {
    if (!v) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(v->mu);
    for (int i = 0; i < kNT; ++i)
        if (!v->loaded[i]) return fail(v, SONIC_ERR_INVALID, std::string("sonic_vad_probs: weight tensor ") + kTensors[i].name + " not loaded");
    if (B < 0 || (B > 0 && (!off || !probs)) || (pcm_i16 == nullptr) == (pcm_f32 == nullptr))
        return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs: needs exactly one of pcm_i16 / pcm_f32, offsets[B + 1] and probs");
    if (B == 0) return SONIC_OK;
    if (off[0] < 0) return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs: offsets[0] < 0");
    std::vector<int64_t> seq(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        if (off[b + 1] < off[b]) return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs: offsets must not decrease");
        seq[b + 1] = seq[b] + (off[b + 1] - off[b] + VAD_NEW - 1) / VAD_NEW;
    }
    const int64_t W = seq[B], n_samp = off[B] - off[0];
    if (W > INT32_MAX / VAD_G) return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs: too many windows");
    if (W == 0) return SONIC_OK;
    const size_t esz = pcm_f32 ? sizeof(float) : sizeof(int16_t);
    const size_t pcm_bytes = (n_samp * esz + 15) / 16 * 16, win_bytes = W * sizeof(VadWindow), seq_bytes = (B + 1) * sizeof(int64_t);
    (void)hipSetDevice(v->dev);
    hipError_t e = grow_windows(v, W);
    if (e == hipSuccess) e = grow_upload(v, pcm_bytes + win_bytes + seq_bytes);
    if (e != hipSuccess) return hip_fail(v, e, "sonic_vad_probs: buffers");
    const char* src = pcm_f32 ? (const char*)(pcm_f32 + off[0]) : (const char*)(pcm_i16 + off[0]);
    memcpy(v->h_up, src, n_samp * esz);
    VadWindow* win = reinterpret_cast<VadWindow*>(v->h_up + pcm_bytes);
    for (int b = 0; b < B; ++b) {
        const int64_t n = off[b + 1] - off[b], s0 = off[b] - off[0];
        float div = 1.0f;
        if (pcm_f32) {                                  // backend/vad.py:24-38 _normalize_audio: / max|x| only when it exceeds 1
            float peak = 0.f;
            for (int64_t i = 0; i < n; ++i) peak = std::max(peak, std::fabs(pcm_f32[off[b] + i]));
            if (peak > 1.0f) div = peak;
        }
        for (int64_t w = 0; w < seq[b + 1] - seq[b]; ++w) {
            VadWindow& wd = win[seq[b] + w];
            wd.start = s0 + w * VAD_NEW;
            wd.n_valid = (int32_t)std::min<int64_t>(VAD_NEW, n - w * VAD_NEW);
            wd.has_ctx = w > 0;
            wd.div = div;
            wd.pad_ = 0;
        }
    }
    memcpy(v->h_up + pcm_bytes + win_bytes, seq.data(), seq_bytes);
    e = hipMemcpyAsync(v->d_up, v->h_up, pcm_bytes + win_bytes + seq_bytes, hipMemcpyHostToDevice, v->st);
    const VadWeights wt = device_weights(v);
    if (e == hipSuccess)
        e = vad_launch(v->d_up, pcm_f32 != nullptr, reinterpret_cast<const VadWindow*>(v->d_up + pcm_bytes), (int)W,
                       reinterpret_cast<const int64_t*>(v->d_up + pcm_bytes + win_bytes), B, wt, v->d_gin, v->d_probs, v->st);
    if (e == hipSuccess) e = hipMemcpyAsync(v->h_probs, v->d_probs, W * sizeof(float), hipMemcpyDeviceToHost, v->st);
    if (e == hipSuccess) e = hipStreamSynchronize(v->st);
    if (e != hipSuccess) return hip_fail(v, e, "sonic_vad_probs");
    memcpy(probs, v->h_probs, W * sizeof(float));
    return SONIC_OK;
}

SONIC_API int sonic_vad_probs_rings(sonic_vad* v, sonic_engine* eng, sonic_ring* const* piece_ring, const int64_t* piece_start, const int32_t* piece_n,
                                    const int64_t* seq_piece, int B, float* probs) {
    if (!v) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(v->mu);
    for (int i = 0; i < kNT; ++i)
        if (!v->loaded[i]) return fail(v, SONIC_ERR_INVALID, std::string("sonic_vad_probs_rings: weight tensor ") + kTensors[i].name + " not loaded");
    if (!eng || B < 0 || (B > 0 && (!seq_piece || !probs)))
        return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs_rings: needs an engine, seq_piece[B + 1] and probs");
    if (B == 0) return SONIC_OK;
    if (seq_piece[0] != 0) return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs_rings: seq_piece[0] must be 0");
    for (int b = 0; b < B; ++b)
        if (seq_piece[b + 1] < seq_piece[b]) return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs_rings: seq_piece must not decrease");
    const int64_t P = seq_piece[B];
    if (P > INT32_MAX) return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs_rings: too many pieces");
    if (P > 0 && (!piece_ring || !piece_start || !piece_n)) return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs_rings: NULL piece arrays");
    (void)hipSetDevice(v->dev);
    (void)hipGetLastError();
    std::vector<RingView> view(P);
    std::vector<std::unique_lock<std::mutex>> held;            // ring locks: from the range check until the front kernel has completed
    std::string why;
    const int rc = ring_ranges_acquire(eng, piece_ring, piece_start, piece_n, P, v->dev, v->st, view.data(), held, why);
    if (rc != SONIC_OK) return fail(v, rc, "sonic_vad_probs_rings: " + why);
    std::vector<int64_t> seq(B + 1, 0), len(B, 0);
    for (int b = 0; b < B; ++b) {
        for (int64_t p = seq_piece[b]; p < seq_piece[b + 1]; ++p) len[b] += piece_n[p];
        seq[b + 1] = seq[b] + (len[b] + VAD_NEW - 1) / VAD_NEW;
    }
    const int64_t W = seq[B];
    if (W > INT32_MAX / VAD_G) return fail(v, SONIC_ERR_INVALID, "sonic_vad_probs_rings: too many windows");
    if (W == 0) return SONIC_OK;
    const size_t piece_bytes = (P * sizeof(VadPiece) + 15) / 16 * 16, win_bytes = W * sizeof(VadRingWindow), seq_bytes = (B + 1) * sizeof(int64_t);
    hipError_t e = grow_windows(v, W);
    if (e == hipSuccess) e = grow_upload(v, piece_bytes + win_bytes + seq_bytes);
    if (e != hipSuccess) return hip_fail(v, e, "sonic_vad_probs_rings: buffers");
    VadPiece* pc = reinterpret_cast<VadPiece*>(v->h_up);
    VadRingWindow* win = reinterpret_cast<VadRingWindow*>(v->h_up + piece_bytes);
    for (int b = 0; b < B; ++b) {
        int64_t at = 0;
        for (int64_t p = seq_piece[b]; p < seq_piece[b + 1]; ++p) {
            pc[p].ring = view[p].buf; pc[p].cap = view[p].cap; pc[p].start = piece_start[p] % view[p].cap;
            pc[p].seq_off = at; pc[p].n = piece_n[p]; pc[p].pad_ = 0;
            at += piece_n[p];
        }
        int64_t p = seq_piece[b];                               // piece of the first sample each window reads; only moves forward
        for (int64_t w = 0; w < seq[b + 1] - seq[b]; ++w) {
            VadRingWindow& wd = win[seq[b] + w];
            wd.pos = w * VAD_NEW;
            wd.n_valid = (int32_t)std::min<int64_t>(VAD_NEW, len[b] - w * VAD_NEW);
            wd.has_ctx = w > 0;                                 // a sequence's first window has no context, whatever precedes it in the ring
            const int64_t first = wd.pos - (w > 0 ? VAD_CTX : 0);
            while (p + 1 < seq_piece[b + 1] && first >= pc[p].seq_off + pc[p].n) ++p;
            wd.piece = (int32_t)p; wd.piece_end = (int32_t)seq_piece[b + 1];
        }
    }
    memcpy(v->h_up + piece_bytes + win_bytes, seq.data(), seq_bytes);
    e = hipMemcpyAsync(v->d_up, v->h_up, piece_bytes + win_bytes + seq_bytes, hipMemcpyHostToDevice, v->st);
    if (e == hipSuccess)
        e = vad_launch_rings(reinterpret_cast<const VadPiece*>(v->d_up), reinterpret_cast<const VadRingWindow*>(v->d_up + piece_bytes), (int)W,
                             reinterpret_cast<const int64_t*>(v->d_up + piece_bytes + win_bytes), B, device_weights(v), v->d_gin, v->d_probs,
                             v->st, v->front_ev);
    if (e == hipSuccess) e = hipMemcpyAsync(v->h_probs, v->d_probs, W * sizeof(float), hipMemcpyDeviceToHost, v->st);
    // the rings stay locked until their last reader, the front kernel, is through (on any failure: until the stream is empty)
    if (e == hipSuccess) e = hipEventSynchronize(v->front_ev);
    if (e != hipSuccess) (void)hipStreamSynchronize(v->st);
    held.clear();
    if (e == hipSuccess) e = hipStreamSynchronize(v->st);
    if (e != hipSuccess) return hip_fail(v, e, "sonic_vad_probs_rings");
    memcpy(probs, v->h_probs, W * sizeof(float));
    return SONIC_OK;
}

}  // extern "C"
