// Shared between vad.hip (kernels) and vad.cpp (C ABI): the Silero VAD network's sizes, the per-window table and the device weights.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum {
    VAD_NEW = 512,                  // new samples per window (16 kHz)
    VAD_CTX = 64,                   // context samples carried from the previous window
    VAD_IN = VAD_NEW + VAD_CTX,     // 576
    VAD_PADDED = VAD_IN + 64,       // reflection pad on the right
    VAD_NFFT = 256, VAD_HOP = 128, VAD_FRAMES = 4,
    VAD_NF = 129,                   // STFT bins (rows 0..128 real, 129..257 imaginary of the basis)
    VAD_HID = 128, VAD_GATES = 4 * VAD_HID,
    VAD_G = 8,                      // windows per block of the front kernel
};

// one window of one sequence: new samples [start, start + n_valid) of the input buffer (the rest of the 512 are zeros), the 64
// samples before `start` as context when has_ctx (not the sequence's first window), float input divided by div (_normalize_audio)
struct VadWindow {
    int64_t start;
    int32_t n_valid, has_ctx;
    float div;
    int32_t pad_;
};

// device layout: every matrix [in][out] (transposed from PyTorch's [out][in]) except whh, which stays [gate row][128]
struct VadWeights {
    const float *basisT;                      // [256][258]
    const float *w0T, *b0, *w1T, *b1, *w2T, *b2, *w3T, *b3;   // [ci * 3 + k][co]
    const float *wihT, *bih, *bhh;            // [128][512]
    const float *whh;                         // [512][128]
    const float *hw, *hb;                     // [128], [1]
};

hipError_t vad_launch(const void* pcm, int is_f32, const VadWindow* win, int W, const int64_t* seq_base, int B, const VadWeights& wt,
                      float* gin, float* probs, hipStream_t st);
