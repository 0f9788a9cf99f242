// What the log-probability kernels share (greedy.hip: greedy_kernel<T, true, ...>; score.hip: score_rows_kernel): the exponential of their sums and the
// per-thread lists / wave merge of the K best alternatives (option top_logprobs).
#pragma once
#include "common.h"

#define TK_NONE 0x7fffffff
__device__ __forceinline__ void tk_insert(float (&tv)[8], int (&ti)[8], float r, int id) {      // the caller has seen r > tv[7]
    tv[7] = r; ti[7] = id;
#pragma unroll
    for (int k = 7; k > 0; --k)
        if (tv[k] > tv[k - 1]) { const float fv = tv[k]; tv[k] = tv[k - 1]; tv[k - 1] = fv; const int fi = ti[k]; ti[k] = ti[k - 1]; ti[k - 1] = fi; }      // strict: equal values keep their order
}
// K rounds over the 64 lanes' sorted lists: lane r leaves with the r-th best pair of all of them (lanes >= K, and places without a finite score: (-inf, TK_NONE))
__device__ __forceinline__ void tk_merge(float (&tv)[8], int (&ti)[8], int K, int lane, float& mv, int& mi) {
    mv = -INFINITY; mi = TK_NONE;
    for (int r = 0; r < K; ++r) {
        float wv = tv[0]; int wi = ti[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(wv, o, 64); const int oi = __shfl_xor(wi, o, 64);
            if (ov > wv || (ov == wv && oi < wi)) { wv = ov; wi = oi; }
        }
        if (lane == r) { mv = wv; mi = wi; }
        if (wi != TK_NONE && ti[0] == wi) {          // the winner's lane pops its head
#pragma unroll
            for (int k = 0; k < 7; ++k) { tv[k] = tv[k + 1]; ti[k] = ti[k + 1]; }
            tv[7] = -INFINITY; ti[7] = TK_NONE;
        }
    }
}
__device__ __forceinline__ float lp_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
