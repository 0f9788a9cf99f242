// The parallel forced run's row kernel (option forced_parallel): the log-probability of a GIVEN token, and the K best alternatives, from one row of
// lm_head logits in the activation type - one block per score row, one pass over the row.  Under teacher forcing every input token is known in advance, so the
// whole forced continuation is one prefill and its logits are the rows of one GEMM; this kernel is what the greedy controller's LP / TOPK part becomes when nothing
// has to be chosen, fed or counted.  The arithmetic follows greedy_kernel<T, true> (greedy.hip) statement by statement: every thread keeps its running maximum
// `best` and the sum lp_s of exp(l - lp_m) over the values it visits - per trip (16 values: two 16-byte loads of a 16-bit type, four of fp32) the old sum is rescaled
// once, then the trip's terms are added in visiting order; threads are brought to their wave's maximum and added by the xor butterfly, waves to the block's maximum
// and added as a fixed tree by thread 0; exp is v_exp_f32 (lp_exp, topk.h); the closing (l_tok - max) - log(sum) is fp64, rounded once.  The target's logit is the T
// value at row[target], read directly.  No logits processor is applied, whatever the handle carries: the row is the raw model distribution at temperature 1.
// One block, one order: a row's record does not depend on the launch's other rows, its index, the chunk it rides in or the handle.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "topk.h"

template <typename T, bool TOPK>
__global__ __launch_bounds__(1024) void score_rows_kernel(ScoreArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T), U = 16 / VEC;      // elements per 16-byte load, loads per trip: 16 values per thread and trip
    typedef typename std::conditional<sizeof(T) == 4, f32x4, typename ET<T>::v8>::type VT;
    __shared__ float sv[16];                     // the waves' maxima ...
    __shared__ float ss_lp[16];                  // ... and their sums, each against its own maximum
    __shared__ float s_tkv[TOPK ? 128 : 1];      // TOPK: the waves' lists, [place][wave] ...
    __shared__ int s_tki[TOPK ? 128 : 1];        // ... and their ids
    __shared__ float s_tk_hand[2];               // thread 0 -> wave 1: the block's maximum and sum, the values the record's first float was formed from
    [[maybe_unused]] float tv[8]; [[maybe_unused]] int ti[8]; [[maybe_unused]] float mv = -INFINITY; [[maybe_unused]] int mi = TK_NONE;
    if constexpr (TOPK) {
#pragma unroll
        for (int k = 0; k < 8; ++k) { tv[k] = -INFINITY; ti[k] = TK_NONE; }
    }
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (b >= a.n) return;
    const T* row = (const T*)a.logits + (long)b * a.ld;
    const int rec = a.rec[b], tgt = a.target[b];
    const bool vec_ok = (((unsigned long long)row) & 15ull) == 0;      // 16-byte loads where the row allows them; the visiting order is the same without
    float* dump = a.dump ? a.dump + ((long)(rec % a.out_ld) * a.R + rec / a.out_ld) * a.V : nullptr;
    float best = -INFINITY, lp_m = -INFINITY, lp_s = 0.f;      // the thread's sum is lp_s * exp(lp_m); a thread that saw nothing holds (-inf, 0)
    for (int g0 = tid; (long)g0 * VEC < a.V; g0 += 1024 * U) {
        float v[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = (g0 + u * 1024) * VEC;
            if (vec_ok && i + VEC <= a.V) {
                const VT x = *(const VT*)(row + i);
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[u][j] = (float)x[j];
            } else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[u][j] = i + j < a.V ? (float)row[i + j] : -INFINITY;      // beyond the row: the sum's identity
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = (g0 + u * 1024) * VEC;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float r = v[u][j];
                if (dump && i + j < a.V) dump[i + j] = r;
                best = fmaxf(best, r);
                if constexpr (TOPK) if (r > tv[7]) tk_insert(tv, ti, r, i + j);      // (a thread visits its ids in ascending order; -inf is never inserted)
            }
        }
        // the trip's values against the maximum so far: one rescale of the old sum, then the terms in visiting order.  While nothing finite has been seen the sum
        // stays 0: -inf - -inf is not formed, here or in the terms
        lp_s = lp_m > -INFINITY ? lp_s * lp_exp(lp_m - best) : 0.f; lp_m = best;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < VEC; ++j) lp_s += best > -INFINITY ? lp_exp(v[u][j] - best) : 0.f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    // every lane now holds the wave's maximum: bring the lane's sum to it (an empty lane is the identity) and add across the wave - the butterfly gives every
    // lane the same tree, and a + b = b + a bit for bit
    lp_s = lp_m > -INFINITY ? lp_s * lp_exp(lp_m - best) : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lp_s += __shfl_xor(lp_s, o, 64);
    if (lane == 0) { sv[wid] = best; ss_lp[wid] = lp_s; }
    if constexpr (TOPK) {
        tk_merge(tv, ti, a.topk, lane, mv, mi);
        if (lane < 8) { s_tkv[lane * 16 + wid] = mv; s_tki[lane * 16 + wid] = mi; }
    }
    __syncthreads();
    if constexpr (TOPK) if (wid == 1) {              // lane w < 16 takes wave w's list; the merge runs beside thread 0's closing arithmetic
#pragma unroll
        for (int k = 0; k < 8; ++k) { tv[k] = lane < 16 ? s_tkv[k * 16 + lane] : -INFINITY; ti[k] = lane < 16 ? s_tki[k * 16 + lane] : TK_NONE; }
        tk_merge(tv, ti, a.topk, lane, mv, mi);
    }
    if (tid == 0) {
        float M = sv[0];
        for (int w = 1; w < 16; ++w) M = fmaxf(M, sv[w]);
        float q[16];                              // the 16 waves at the block's maximum (an empty wave: 0), added as a fixed binary tree
#pragma unroll
        for (int w = 0; w < 16; ++w) q[w] = sv[w] > -INFINITY ? ss_lp[w] * lp_exp(sv[w] - M) : 0.f;
#pragma unroll
        for (int h = 8; h > 0; h >>= 1)
#pragma unroll
            for (int w = 0; w < h; ++w) q[w] = q[2 * w] + q[2 * w + 1];
        if ((unsigned)tgt < (unsigned)a.V) {
            if (a.out_ids) a.out_ids[rec] = tgt;
            if (a.out_lp) a.out_lp[(long)rec * (TOPK ? 1 + 2 * a.topk : 1)] = (float)(((double)(float)row[tgt] - (double)M) - log((double)q[0]));
        }
        s_tk_hand[0] = M; s_tk_hand[1] = q[0];
    }
    if constexpr (TOPK) {
        __syncthreads();
        if (wid == 1 && lane < a.topk && a.out_lp) {
            const int K = a.topk;
            float* r = a.out_lp + (long)rec * (1 + 2 * K);
            const bool any = mi != TK_NONE;
            r[1 + lane] = any ? (float)(((double)mv - (double)s_tk_hand[0]) - log((double)s_tk_hand[1])) : -INFINITY;
            r[1 + K + lane] = any ? (float)mi : -1.f;      // (ids stay below 2^24: exact)
        }
    }
}

template <typename T> static void score_launch(const ScoreArgs& a, hipStream_t s) {
    if (a.topk >= 1 && a.topk <= 8 && a.out_lp) hipLaunchKernelGGL((score_rows_kernel<T, true>), dim3(a.n), dim3(1024), 0, s, a);
    else hipLaunchKernelGGL((score_rows_kernel<T, false>), dim3(a.n), dim3(1024), 0, s, a);
}
void launch_score_rows(const ScoreArgs& a, hipStream_t s) {
    if (a.n < 1) return;
    if (a.dt == DT_F32) { score_launch<float>(a, s); return; }
    DT_SWITCH(a.dt, T, score_launch<T>(a, s));
}

// Test hook route (the greedy hook's slab form of a logits row): v + w, then ks = 2 ..., rounded to T as greedy_kernel rounds what it compares
template <typename T> __global__ void score_slab_rows_kernel(const float* slabs, int ksplit, long ks_stride, int V, T* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= V) return;
    const float* lg = slabs + (long)b * V;
    float f = lg[i];
    if (ksplit > 1) f += lg[ks_stride + i];
    for (int ks = 2; ks < ksplit; ++ks) f += lg[ks * ks_stride + i];
    out[(long)b * V + i] = (T)rT<T>(f);
}
void launch_score_slab_rows(const float* slabs, int ksplit, int mpad, int V, int B, void* out, int dt, hipStream_t s) {
    const dim3 grid((V + 255) / 256, B);
    const long st = (long)mpad * V;
    if (dt == DT_F32) { hipLaunchKernelGGL(score_slab_rows_kernel<float>, grid, dim3(256), 0, s, slabs, ksplit, st, V, (float*)out); return; }
    DT_SWITCH(dt, T, hipLaunchKernelGGL(score_slab_rows_kernel<T>, grid, dim3(256), 0, s, slabs, ksplit, st, V, (T*)out));
}
