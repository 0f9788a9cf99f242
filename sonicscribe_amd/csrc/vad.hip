// Silero VAD network (silero-vad 5.x / 6.x, 16 kHz branch; layer table in sonicscribe_amd/vad_net.py) for the reference's
// VADProcessor (backend/vad.py:84-126).  Two kernels, all fp32 (the probability meets a threshold; no reduced-precision operands):
//
//   vad_front_kernel   window-parallel: 576 samples (64 context + 512 new) -> reflection pad -> STFT magnitude [129][4] ->
//                      4 x (conv1d k3 + ReLU) -> W_ih x + b_ih + b_hh = the 512 LSTM gate inputs of the window.  A block takes
//                      VAD_G windows so that each weight it reads from L2 serves VAD_G windows.
//   vad_recur_kernel   sequence-parallel: one block per sequence walks its windows in order (LSTMCell, then the head
//                      sigmoid(w . relu(h) + b)).  Thread j owns gate row j of W_hh in registers for the whole loop; h goes
//                      through LDS; two barriers per step.
//
// Batch invariance: every output is one thread's fixed-order sum over weights and its own window's (or sequence's) data; where a
// window sits in the call or what else is in it changes no operation.  Device weights are stored transposed ([in][out]) so that
// consecutive threads (consecutive outputs) read consecutive addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vad_dev.h"

namespace {

constexpr int NT = 256;            // threads of the front kernel

struct FrontSmem {
    float sig[VAD_G][VAD_PADDED];                 // padded window (640)
    float spec[VAD_G][VAD_NF * VAD_FRAMES];       // [f][t]
    float e0[VAD_G][128 * 4];                     // [c][t]
    float e1[VAD_G][64 * 2];
    float e2[VAD_G][64];
    float e3[VAD_G][128];
};

// out[co][t] = relu(b[co] + sum_ci sum_k w[ci][k][co] * in[ci][t * S + k - 1]) for G windows; in / out are [c][t] per window
template <int CI, int CO, int TI, int TO, int S>
__device__ __forceinline__ void conv_k3(const float* __restrict__ wT, const float* __restrict__ b, const float* in, int in_stride,
                                        float* out, int out_stride) {
    for (int item = threadIdx.x; item < CO * TO; item += NT) {
        const int co = item % CO, t = item / CO;
        float acc[VAD_G];
        #pragma unroll
        for (int g = 0; g < VAD_G; ++g) acc[g] = 0.f;
        for (int ci = 0; ci < CI; ++ci) {
            #pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int ti = t * S + k - 1;
                if (ti < 0 || ti >= TI) continue;
                const float w = wT[(ci * 3 + k) * CO + co];
                #pragma unroll
                for (int g = 0; g < VAD_G; ++g) acc[g] = fmaf(w, in[g * in_stride + ci * TI + ti], acc[g]);
            }
        }
        const float bb = b[co];
        #pragma unroll
        for (int g = 0; g < VAD_G; ++g) out[g * out_stride + co * TO + t] = fmaxf(acc[g] + bb, 0.f);
    }
}

// everything behind the sample load: sm.sig[g][0 .. 575] of the block's windows -> their 512 gate inputs
__device__ __forceinline__ void front_rest(FrontSmem& sm, int w0, int W, const VadWeights& wt, float* __restrict__ gin) {
    __syncthreads();
    for (int i = threadIdx.x; i < VAD_G * (VAD_PADDED - VAD_IN); i += NT) {
        const int g = i / (VAD_PADDED - VAD_IN), k = i % (VAD_PADDED - VAD_IN);
        sm.sig[g][VAD_IN + k] = sm.sig[g][VAD_IN - 2 - k];
    }
    __syncthreads();
    // 2. STFT as conv1d (258 filters of 256 taps, stride 128, 4 frames) and magnitude; item = (frequency f, frame t)
    for (int item = threadIdx.x; item < VAD_NF * VAD_FRAMES; item += NT) {
        const int f = item % VAD_NF, t = item / VAD_NF;
        float re[VAD_G], im[VAD_G];
        #pragma unroll
        for (int g = 0; g < VAD_G; ++g) re[g] = im[g] = 0.f;
        for (int k = 0; k < VAD_NFFT; ++k) {
            const float br = wt.basisT[k * (2 * VAD_NF) + f], bi = wt.basisT[k * (2 * VAD_NF) + VAD_NF + f];
            #pragma unroll
            for (int g = 0; g < VAD_G; ++g) {
                const float x = sm.sig[g][t * VAD_HOP + k];
                re[g] = fmaf(br, x, re[g]);
                im[g] = fmaf(bi, x, im[g]);
            }
        }
        #pragma unroll
        for (int g = 0; g < VAD_G; ++g) sm.spec[g][f * VAD_FRAMES + t] = sqrtf(re[g] * re[g] + im[g] * im[g]);
    }
    __syncthreads();
    // 3. encoder
    conv_k3<VAD_NF, 128, 4, 4, 1>(wt.w0T, wt.b0, &sm.spec[0][0], VAD_NF * VAD_FRAMES, &sm.e0[0][0], 128 * 4);
    __syncthreads();
    conv_k3<128, 64, 4, 2, 2>(wt.w1T, wt.b1, &sm.e0[0][0], 128 * 4, &sm.e1[0][0], 64 * 2);
    __syncthreads();
    conv_k3<64, 64, 2, 1, 2>(wt.w2T, wt.b2, &sm.e1[0][0], 64 * 2, &sm.e2[0][0], 64);
    __syncthreads();
    conv_k3<64, 128, 1, 1, 1>(wt.w3T, wt.b3, &sm.e2[0][0], 64, &sm.e3[0][0], 128);
    __syncthreads();
    // 4. LSTM input half: gin[w][j] = (W_ih x)[j] + b_ih[j] + b_hh[j]
    for (int j = threadIdx.x; j < VAD_GATES; j += NT) {
        float acc[VAD_G];
        #pragma unroll
        for (int g = 0; g < VAD_G; ++g) acc[g] = 0.f;
        for (int i = 0; i < VAD_HID; ++i) {
            const float w = wt.wihT[i * VAD_GATES + j];
            #pragma unroll
            for (int g = 0; g < VAD_G; ++g) acc[g] = fmaf(w, sm.e3[g][i], acc[g]);
        }
        const float bb = wt.bih[j] + wt.bhh[j];
        #pragma unroll
        for (int g = 0; g < VAD_G; ++g)
            if (w0 + g < W) gin[(int64_t)(w0 + g) * VAD_GATES + j] = acc[g] + bb;
    }
}

__global__ void __launch_bounds__(NT) vad_front_kernel(const void* __restrict__ pcm, int is_f32, const VadWindow* __restrict__ win, int W,
                                                      VadWeights wt, float* __restrict__ gin) {
    __shared__ FrontSmem sm;
    const int w0 = blockIdx.x * VAD_G;
    // 1. samples: context (64 before the window's first new sample; zeros for a sequence's first window), 512 new ones (zeros past
    //    the end of the sequence), then the reflection pad on the right: pad[576 + k] = x[574 - k]
    for (int i = threadIdx.x; i < VAD_G * VAD_IN; i += NT) {
        const int g = i / VAD_IN, s = i % VAD_IN;
        float v = 0.f;
        if (w0 + g < W) {
            const VadWindow wd = win[w0 + g];
            const int rel = s - VAD_CTX;                          // sample index relative to the window's first new sample
            const bool ok = rel < 0 ? wd.has_ctx != 0 : rel < wd.n_valid;
            if (ok) {
                const int64_t idx = wd.start + rel;
                v = is_f32 ? static_cast<const float*>(pcm)[idx] / wd.div
                           : static_cast<float>(static_cast<const int16_t*>(pcm)[idx]) * (1.0f / 32768.0f);
            }
        }
        sm.sig[g][s] = v;
    }
    front_rest(sm, w0, W, wt, gin);
}

// The ring source: the same windows cut from int16 rings in HBM, in place (VadPiece / VadRingWindow in vad_dev.h).  A ring range starts at
// an arbitrary sample, so the loads are 2-byte loads, consecutive threads on consecutive samples; the value path is the int16 path above.
__global__ void __launch_bounds__(NT) vad_front_ring_kernel(const VadPiece* __restrict__ pieces, const VadRingWindow* __restrict__ win, int W,
                                                           VadWeights wt, float* __restrict__ gin) {
    __shared__ FrontSmem sm;
    const int w0 = blockIdx.x * VAD_G;
    for (int i = threadIdx.x; i < VAD_G * VAD_IN; i += NT) {
        const int g = i / VAD_IN, s = i % VAD_IN;
        float v = 0.f;
        if (w0 + g < W) {
            const VadRingWindow wd = win[w0 + g];
            const int rel = s - VAD_CTX;
            const bool ok = rel < 0 ? wd.has_ctx != 0 : rel < wd.n_valid;
            if (ok) {
                const int64_t q = wd.pos + rel;                    // index within the sequence
                int p = wd.piece;
                while (p + 1 < wd.piece_end && q >= pieces[p].seq_off + pieces[p].n) ++p;
                const VadPiece pc = pieces[p];
                const int64_t o = q - pc.seq_off;
                if (o >= 0 && o < pc.n) {
                    int64_t idx = pc.start + o;                     // < 2 * cap
                    if (idx >= pc.cap) idx -= pc.cap;
                    v = static_cast<float>(pc.ring[idx]) * (1.0f / 32768.0f);
                }
            }
        }
        sm.sig[g][s] = v;
    }
    front_rest(sm, w0, W, wt, gin);
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// block = one sequence; seq_base[B + 1]: its windows are gin rows seq_base[b] .. seq_base[b + 1] - 1, probabilities at the same indices
__global__ void __launch_bounds__(VAD_GATES) vad_recur_kernel(const float* __restrict__ gin, const int64_t* __restrict__ seq_base,
                                                             VadWeights wt, float* __restrict__ probs) {
    __shared__ float4 hs4[VAD_HID / 4];
    __shared__ float gs[VAD_GATES];
    float* hs = reinterpret_cast<float*>(hs4);
    const int j = threadIdx.x;
    const int64_t base = seq_base[blockIdx.x], T = seq_base[blockIdx.x + 1] - base;
    float w[VAD_HID];                                   // gate row j of W_hh: registers for the whole sequence
    #pragma unroll
    for (int i = 0; i < VAD_HID; i += 4) {
        const float4 v = *reinterpret_cast<const float4*>(wt.whh + j * VAD_HID + i);
        w[i] = v.x; w[i + 1] = v.y; w[i + 2] = v.z; w[i + 3] = v.w;
    }
    const float hw0 = j < 64 ? wt.hw[j] : 0.f, hw1 = j < 64 ? wt.hw[j + 64] : 0.f, hb = wt.hb[0];
    float c = 0.f;
    if (j < VAD_HID) hs[j] = 0.f;
    __syncthreads();
    float gnext = T > 0 ? gin[base * VAD_GATES + j] : 0.f;
    for (int64_t t = 0; t < T; ++t) {
        const float gx = gnext;
        if (t + 1 < T) gnext = gin[(base + t + 1) * VAD_GATES + j];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        #pragma unroll
        for (int i = 0; i < VAD_HID / 4; ++i) {
            const float4 h = hs4[i];
            a0 = fmaf(w[4 * i], h.x, a0); a1 = fmaf(w[4 * i + 1], h.y, a1);
            a2 = fmaf(w[4 * i + 2], h.z, a2); a3 = fmaf(w[4 * i + 3], h.w, a3);
        }
        gs[j] = gx + ((a0 + a1) + (a2 + a3));
        __syncthreads();
        if (j < VAD_HID) {                                // PyTorch LSTMCell: gates i, f, g, o
            const float ig = sigm(gs[j]), fg = sigm(gs[VAD_HID + j]), gg = tanhf(gs[2 * VAD_HID + j]), og = sigm(gs[3 * VAD_HID + j]);
            c = fg * c + ig * gg;
            hs[j] = og * tanhf(c);
        }
        __syncthreads();
        if (j < 64) {                                     // head: one wave, fixed reduction order
            float p = hw0 * fmaxf(hs[j], 0.f) + hw1 * fmaxf(hs[j + 64], 0.f);
            #pragma unroll
            for (int off = 32; off > 0; off >>= 1) p += __shfl_xor(p, off);
            if (j == 0) probs[base + t] = sigm(p + hb);
        }
    }
}

}  // namespace

hipError_t vad_launch(const void* pcm, int is_f32, const VadWindow* win, int W, const int64_t* seq_base, int B, const VadWeights& wt,
                      float* gin, float* probs, hipStream_t st) {
    if (W > 0) hipLaunchKernelGGL(vad_front_kernel, dim3((W + VAD_G - 1) / VAD_G), dim3(NT), 0, st, pcm, is_f32, win, W, wt, gin);
    if (B > 0) hipLaunchKernelGGL(vad_recur_kernel, dim3(B), dim3(VAD_GATES), 0, st, gin, seq_base, wt, probs);
    return hipGetLastError();
}

hipError_t vad_launch_rings(const VadPiece* pieces, const VadRingWindow* win, int W, const int64_t* seq_base, int B, const VadWeights& wt,
                            float* gin, float* probs, hipStream_t st, hipEvent_t front_done) {
    if (W > 0) hipLaunchKernelGGL(vad_front_ring_kernel, dim3((W + VAD_G - 1) / VAD_G), dim3(NT), 0, st, pieces, win, W, wt, gin);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && front_done) e = hipEventRecord(front_done, st);
    if (e != hipSuccess) return e;
    if (B > 0) hipLaunchKernelGGL(vad_recur_kernel, dim3(B), dim3(VAD_GATES), 0, st, gin, seq_base, wt, probs);
    return hipGetLastError();
}
