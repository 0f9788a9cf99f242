// What the kernels that reduce one row of logits per block share (greedy.hip: greedy_kernel; rows.hip: rows_kernel), each piece written once: the vocabulary maps
// of a history and a score under them (HF's logits processors), the first-maximum butterfly, the log-probability sum's exponential, rescale, wave
// fold and block close (6.3), and the lists of the K best alternatives with their two merges and the record write (option top_logprobs; 6.7).  The contract of
// these kernels is bit-level - one block, one order - so a change to the accumulation scheme is made here, for all of them.
#pragma once
#include "common.h"

// ---------------------------------------------------------------- the history's maps
__device__ __forceinline__ float guard_score(float r, unsigned seen, unsigned banned, float p) {
    if (seen & 1u) r = r < 0.f ? r * p : __fdiv_rn(r, p);
    return (banned & 1u) ? -INFINITY : r;
}
__device__ __forceinline__ void guard_set(unsigned* map, int id, int V) {
    if ((unsigned)id < (unsigned)V) atomicOr(&map[id >> 5], 1u << (id & 31));
}
// seen = the ids of the history h[0 .. len); banned |= the continuations of earlier occurrences of its last n - 1 ids, and the suppress list.  Integer ORs into maps
// the block has zeroed: no order in them.  The caller puts a barrier behind
__device__ __forceinline__ void hist_maps(unsigned* g_seen, unsigned* g_ban, const int* h, int len, int n, const int* suppress, int n_suppress, int V, int tid) {
    for (int j = tid; j < len; j += 1024) guard_set(g_seen, h[j], V);
    if (n > 0) {                              // every n-gram h[j .. j + n) of the history whose first n - 1 ids are the history's last n - 1 bans its last id
        const int* last = h + len - (n - 1);  // (read only when an n-gram exists: j + n <= len)
        for (int j = tid; j + n <= len; j += 1024) {
            bool m = true;
            for (int k = 0; k < n - 1; ++k) m = m && h[j + k] == last[k];
            if (m) guard_set(g_ban, h[j + n - 1], V);
        }
    }
    for (int j = tid; j < n_suppress; j += 1024) guard_set(g_ban, suppress[j], V);
}

// ---------------------------------------------------------------- the first maximum
#define TK_NONE 0x7fffffff
// every lane leaves with the wave's largest value and, among equal values, the lowest id: torch.argmax's first maximum.  A macro where everything else here is a
// function: through a function, by reference or by value, hipcc allocates greedy_kernel's registers differently, and the instantiations the benchmark runs
// (greedy_kernel<T, false x 6>) keep their machine code only with the statements in place
#define FIRST_MAX_WAVE(v, id) \
    _Pragma("unroll") \
    for (int o = 32; o > 0; o >>= 1) { \
        const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(id, o, 64); \
        if (ov > v || (ov == v && oi < id)) { v = ov; id = oi; } \
    }

// ---------------------------------------------------------------- the log-probability sum
__device__ __forceinline__ float lp_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
// a sum held against the maximum lp_m, brought to the maximum M >= lp_m.  A sum that has seen nothing finite is 0: -inf - -inf is not formed
__device__ __forceinline__ float lp_rescale(float lp_s, float lp_m, float M) { return lp_m > -INFINITY ? lp_s * lp_exp(lp_m - M) : 0.f; }
// every lane holds the wave's maximum M: bring the lane's sum to it (an empty lane is the identity: 0, not 0 * exp(-inf + inf)) and add across the wave - the
// butterfly gives every lane the same tree, and a + b = b + a bit for bit
__device__ __forceinline__ float lp_wave_fold(float lp_s, float lp_m, float M) {
    lp_s = lp_rescale(lp_s, lp_m, M);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lp_s += __shfl_xor(lp_s, o, 64);
    return lp_s;
}
// thread 0: the 16 waves (maxima wm, sums ws) at the block's maximum M (an empty wave: 0), added as a fixed binary tree
__device__ __forceinline__ float lp_block_close(const float* wm, const float* ws, float M) {
    float q[16];
#pragma unroll
    for (int w = 0; w < 16; ++w) q[w] = lp_rescale(ws[w], wm[w], M);
#pragma unroll
    for (int h = 8; h > 0; h >>= 1)
#pragma unroll
        for (int w = 0; w < h; ++w) q[w] = q[2 * w] + q[2 * w + 1];
    return q[0];
}

// ---------------------------------------------------------------- the K best alternatives
__device__ __forceinline__ void tk_init(float (&tv)[8], int (&ti)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { tv[k] = -INFINITY; ti[k] = TK_NONE; }
}
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
        FIRST_MAX_WAVE(wv, wi)
        if (lane == r) { mv = wv; mi = wi; }
        if (wi != TK_NONE && ti[0] == wi) {          // the winner's lane pops its head
#pragma unroll
            for (int k = 0; k < 7; ++k) { tv[k] = tv[k + 1]; ti[k] = ti[k + 1]; }
            tv[7] = -INFINITY; ti[7] = TK_NONE;
        }
    }
}
// every wave: its threads' lists merged, the result staged in LDS as [place][wave] (lane w of wave 1 reads wave w's: consecutive words).  A barrier follows
__device__ __forceinline__ void tk_stage(float (&tv)[8], int (&ti)[8], int K, int lane, int wid, float* s_tkv, int* s_tki, float& mv, int& mi) {
    tk_merge(tv, ti, K, lane, mv, mi);
    if (lane < 8) { s_tkv[lane * 16 + wid] = mv; s_tki[lane * 16 + wid] = mi; }
}
// wave 1: lane w < 16 takes wave w's list, and the second merge leaves the block's r-th best pair in lane r
__device__ __forceinline__ void tk_merge_waves(float (&tv)[8], int (&ti)[8], int K, int lane, const float* s_tkv, const int* s_tki, float& mv, int& mi) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { tv[k] = lane < 16 ? s_tkv[k * 16 + lane] : -INFINITY; ti[k] = lane < 16 ? s_tki[k * 16 + lane] : TK_NONE; }
    tk_merge(tv, ti, K, lane, mv, mi);
}
// lane < K of wave 1: its place of the record r = [lp | K alternative lps | K ids as fp32], from the block's maximum M and sum - the values r[0] was formed from
__device__ __forceinline__ void tk_record(float* r, int K, int lane, float mv, int mi, float M, float sum) {
    const bool any = mi != TK_NONE;
    r[1 + lane] = any ? (float)(((double)mv - (double)M) - log((double)sum)) : -INFINITY;
    r[1 + K + lane] = any ? (float)mi : -1.f;      // (ids stay below 2^24: exact)
}
