// The cut of a truncating sampler (top_k / top_p / min_p; option truncation), found without a sort: a radix select over the monotone uint32 image of
// y = fdiv_rn(s, t), refined over three passes of 11 / 11 / 10 bits on one histogram of 2048 64-bit bins in LDS.  The bins hold counts (top_k; the tie break by id)
// or masses (top_p) as integers - a mass is rint(exp2((y - y_max) * log2 e) * 2^32) - added with integer LDS atomics: no order in them, so the cut is a pure function
// of the row's scores, whichever wave adds first.  The caller (greedy.hip) hands in a functor that recomputes the four y of a group from the slabs; nothing of size V
// is kept.  One block of 1024 threads; every function here is reached by all of them or by none (the barriers are inside).
#pragma once
#include "common.h"

typedef unsigned long long tr_u64;
#define TRUNC_BINS 2048
#define TRUNC_LDS_BYTES (TRUNC_BINS * 8)      // the histogram: static LDS of the TRUNC instantiations (s_trh), beside the GUARD / BIAS maps in dynamic LDS
#define TRUNC_ID_ALL 0x7fffffff               // a cut that keeps every id of its key

// larger y <-> larger key; -0.0 counts as +0.0 (the two compare equal as floats)
__device__ __forceinline__ unsigned trunc_key(float y) {
    unsigned u = __float_as_uint(y);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float trunc_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// the fixed-point mass of y against the row's maximum: at most 2^32 (y = y_max, exactly), 0 for -inf
__device__ __forceinline__ tr_u64 trunc_mass(float y, float ymax) {
    return (tr_u64)__builtin_rintf(__builtin_amdgcn_exp2f((y - ymax) * 1.44269504088896340736f) * 4294967296.f);
}
// is an id of key `key` inside the cut (kc, ic): a larger key, or the cut's key and an id up to ic
__device__ __forceinline__ bool trunc_keeps(unsigned key, int id, unsigned kc, int ic) { return key > kc || (key == kc && id <= ic); }

// The bins h[0 .. nb) read from the top: the first bin whose inclusive sum reaches T (1 <= T).  res[0] = the bin (~0: T is beyond the total), res[1] = the sum above
// it, res[2] = the bin's own value, res[3] = the total.  Thread t takes bins nb - 1 - 2t and the one below; a shuffle scan per wave, the waves' totals in s_w[16]
__device__ __forceinline__ void trunc_find(const tr_u64* h, int nb, tr_u64 T, tr_u64* s_w, tr_u64* res, int tid) {
    const int lane = tid & 63, wid = tid >> 6;
    const int b0 = nb - 1 - 2 * tid, b1 = b0 - 1;
    const tr_u64 v0 = b0 >= 0 ? h[b0] : 0ull, v1 = b1 >= 0 ? h[b1] : 0ull, loc = v0 + v1;
    tr_u64 inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const tr_u64 up = __shfl_up(inc, o, 64); if (lane >= o) inc += up; }
    if (lane == 63) s_w[wid] = inc;
    if (tid == 0) res[0] = ~0ull;
    __syncthreads();
    tr_u64 off = 0ull;
    for (int w = 0; w < wid; ++w) off += s_w[w];
    const tr_u64 ex = off + inc - loc;
    if (ex < T && T <= ex + v0) { res[0] = (tr_u64)b0; res[1] = ex; res[2] = v0; }
    else if (ex + v0 < T && T <= ex + loc) { res[0] = (tr_u64)b1; res[1] = ex + v0; res[2] = v1; }
    if (tid == 1023) res[3] = off + inc;
    __syncthreads();
}

// what a select descends on
enum { TS_COUNT = 0,      // keys of y, weight 1: the T-th largest y
       TS_MASS = 1,       // keys of y at or above key_ref (the top_k survivors), weight = the mass: the rank whose preceding mass first stays below frac * mass(K)
       TS_ID = 2 };       // ids (ascending) among the y of key key_ref, weight 1: the T-th lowest id
// One select.  y4(i, y): the four y of group i (i a multiple of 4, below V).  Leaves in out[0] the 32-bit key found (TS_ID: the id), out[1] the weight strictly in
// front of that key, out[2] the weight of the key itself, out[3] what is left of T behind out[1] (1 .. out[2]); returns false when T lies beyond the total (the caller then cuts nothing).  TS_MASS: T = ceil(frac * total)
// is formed here from the first pass's total, in float64 - before < frac * total and before < T are the same for an integer
template <int MODE, class Y4>
__device__ __forceinline__ bool trunc_select(Y4 y4, int V, int tid, tr_u64* h, tr_u64* s_w, tr_u64* res, tr_u64 T, float frac, unsigned key_ref, float ymax, tr_u64* out) {
    unsigned pre = 0u; tr_u64 front = 0ull, own = 0ull;
    for (int level = 0; level < 3; ++level) {
        const int shift = level == 0 ? 21 : level == 1 ? 10 : 0, width = level == 2 ? 10 : 11, nb = 1 << width;
        for (int w = tid; w < TRUNC_BINS; w += 1024) h[w] = 0ull;
        __syncthreads();
        for (int i = tid * 4; i < V; i += 4096) {
            float y[4];
            y4(i, y);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned key = trunc_key(y[j]);
                unsigned sk = key; bool in = true; tr_u64 wt = 1ull;
                if constexpr (MODE == TS_MASS) { in = key >= key_ref; wt = trunc_mass(y[j], ymax); }
                if constexpr (MODE == TS_ID) { sk = ~(unsigned)(i + j); in = key == key_ref; }
                if (level > 0) in = in && (sk >> (shift + width)) == pre;
                if (in && wt) atomicAdd(&h[(sk >> shift) & (unsigned)(nb - 1)], wt);
            }
        }
        __syncthreads();
        if (MODE == TS_MASS && level == 0) {
            trunc_find(h, nb, ~0ull, s_w, res, tid);      // (no bin reaches it: the pass leaves the total)
            const tr_u64 total = res[3];
            __syncthreads();                             // res is rewritten below
            T = (tr_u64)ceil((double)frac * (double)total);
            if (T < 1ull) T = 1ull;
        }
        trunc_find(h, nb, T, s_w, res, tid);
        const tr_u64 bin = res[0], above = res[1];
        own = res[2];
        __syncthreads();                                 // (res and h are rewritten by the next level)
        if (bin == ~0ull) return false;
        T -= above; front += above;
        pre = (pre << width) | (unsigned)bin;
    }
    out[0] = MODE == TS_ID ? (tr_u64)~pre : (tr_u64)pre; out[1] = front; out[2] = own; out[3] = T;
    return true;
}

// The cut of one row.  tw: the row's three words (top_k; the bits of top_p, 0: off; the bits of lnm, 0: off); ymax: the row's maximum of y (finite).  Leaves (kc, ic): an id is kept iff trunc_keeps(key, id, kc, ic).
//   top_k  kc_k = the key of the k-th largest y, every id of it kept (k >= V: off; a k-th value of -inf keeps everything: every key is at or above it)
//   top_p  over the keys >= kc_k: the key at which the mass in front first reaches T = ceil(top_p * mass(K)) once the key's own ids are added; of its c ids of mass w
//          each the j = ceil((T - front) / w) lowest stay (1 <= j <= c: front < T <= front + c w), found by a select over the ids when j < c
//   min_p  kc_m = the key of fadd_rn(ymax, lnm), every id of it kept
// and the most restrictive of the three: the largest key, at equal keys the lowest id
template <class Y4>
__device__ __forceinline__ void trunc_cut(Y4 y4, int V, int tid, const unsigned* tw, float ymax, tr_u64* h, tr_u64* s_w, tr_u64* res, unsigned& kc, int& ic) {
    const unsigned top_k = tw[0]; const float top_p = __uint_as_float(tw[1]), lnm = __uint_as_float(tw[2]);
    kc = 0u; ic = TRUNC_ID_ALL;
    tr_u64 out[4];
    unsigned kk = 0u;
    if (top_k >= 1u && top_k < (unsigned)V && trunc_select<TS_COUNT>(y4, V, tid, h, s_w, res, (tr_u64)top_k, 0.f, 0u, ymax, out)) kk = (unsigned)out[0];
    kc = kk;
    if (tw[1] != 0u && top_p > 0.f && top_p < 1.f && trunc_select<TS_MASS>(y4, V, tid, h, s_w, res, 0ull, top_p, kk, ymax, out)) {
        const unsigned kp = (unsigned)out[0];
        const tr_u64 w = trunc_mass(trunc_unkey(kp), ymax);      // every id of a key has the key's y, hence its mass: own = c w
        int ip = TRUNC_ID_ALL;
        if (w > 0ull) {
            const tr_u64 c = out[2] / w, j = (out[3] + w - 1ull) / w;      // out[3] = T - front, in 1 .. own
            if (j < c && trunc_select<TS_ID>(y4, V, tid, h, s_w, res, j < 1ull ? 1ull : j, 0.f, kp, ymax, out)) ip = (int)(unsigned)out[0];
        }
        if (kp > kc || (kp == kc && ip < ic)) { kc = kp; ic = ip; }
    }
    if (tw[2] != 0u) {                                   // (word 0: off; min_p = 1 arrives as -0.0)
        const unsigned km = trunc_key(ymax + lnm);
        if (km > kc) { kc = km; ic = TRUNC_ID_ALL; }
    }
}
