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

// Ring source (sonic_vad_probs_rings): a sequence is a run of pieces, each the samples [start, start + n) of an int16 ring in HBM, read
// in place.  `start` is already reduced into [0, cap) by the host; the kernel adds the offset within the piece and subtracts cap once when
// the sum passes the end of the buffer (n <= cap), so a window's 576 samples may straddle the wrap and may come from several pieces.
struct VadPiece {
    const int16_t* ring;            // base of the ring buffer
    int64_t cap;                    // its capacity in samples
    int64_t start;                  // buffer position of the piece's first sample, in [0, cap)
    int64_t seq_off;                // index of that sample within its sequence
    int32_t n, pad_;
};
// one window of a ring sequence: new samples [pos, pos + n_valid) of the sequence, context [pos - 64, pos) when has_ctx.  `piece` is the
// piece that holds the window's first sample read (pos - 64 with context, pos without), `piece_end` one past the sequence's last piece.
struct VadRingWindow {
    int64_t pos;
    int32_t piece, piece_end;
    int32_t n_valid, has_ctx;
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
// the same two kernels over ring pieces; front_done (may be NULL) is recorded behind the front kernel, the last reader of ring memory
hipError_t vad_launch_rings(const VadPiece* pieces, const VadRingWindow* win, int W, const int64_t* seq_base, int B, const VadWeights& wt,
                            float* gin, float* probs, hipStream_t st, hipEvent_t front_done);
