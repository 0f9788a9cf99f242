// The row kernel of the two passes that read the lm_head's logits as the rows of one prefill GEMM: the parallel forced run (option forced_parallel) and
// draft-verified decoding (option draft_verify; 6.11).
// rows_kernel<T, CHOOSE, GUARD, TOPK>: one block per row, one pass over the row's V logits in the activation type; the record of a GIVEN token target[i] -
// log_softmax(s)[target] and, with TOPK, the K best ids of s by (value descending, id ascending).  One kernel, four flags: what a flag adds sits behind its
// `if constexpr`, and no flag changes an arithmetic statement of the sum.  The arithmetic follows greedy_kernel<T, true> (greedy.hip) statement by statement, through
// the pieces of rowlp.h: every thread keeps its running maximum `best` and the sum lp_s of exp(s - lp_m) over the values it visits - per trip (16 values: two 16-byte
// loads of a 16-bit type, four of fp32) the old sum is rescaled once, then the trip's terms are added in visiting order; threads are brought to their wave's maximum
// and added by the xor butterfly, waves to the block's maximum and added as a fixed tree by thread 0; exp is v_exp_f32 (lp_exp); the closing (s_tok - max) - log(sum)
// is fp64, rounded once.  The target's logit is the T value at row[target], read directly.  One block, one order: a row's record does not depend on the launch's
// other rows, its index, the chunk it rides in or the handle.
// CHOOSE = false, GUARD = false is the forced run's kernel (bf16, fp16, fp32): s is the raw row, no logits processor is applied, whatever the handle carries; the
// record goes to out_lp[rec[i]] and the target to out_ids[rec[i]].
// CHOOSE (bf16, fp16) adds what the model itself would emit at the row: beside the running maximum every thread keeps the id that reached it first (strict >: a
// thread visits its ids in ascending order), and the reductions prefer the lower id among equal values - torch.argmax's first maximum, to choice[i]; a row whose
// scores are all -inf gives 0.  Its caller asks for the record by row (lp_by_row): a staging array [row][1 + 2K], from which draft_accept_kernel copies the accepted ones.
// GUARD (with CHOOSE): the handle's processors (sonic_set_generation) on the scores, as greedy_kernel<T, ., true> applies them - the block builds the "seen" /
// "banned" bitmaps of the row's history hist[hrow][0 .. hlen) = prompt || draft[0 .. n) in LDS (hist_maps) and every value goes through guard_score ahead of the
// compare, the sum and the lists; the dump stays raw.
// draft_accept_kernel: one block per request - the first position whose choice differs from the draft id (a = D when none does), the accepted ids and records into
// the request's output rows, and the row state a prefill of prompt || draft[0 .. a) would have left: n_new = step counter = a, kv_len = P + a, last_row = the hidden
// row that decides token a.  A request without a draft is left as the plan set it.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "rowlp.h"

extern __shared__ unsigned v_bits[];
template <typename T, bool CHOOSE, bool GUARD, bool TOPK>
__global__ __launch_bounds__(1024) void rows_kernel(RowsArgs a) {
    static_assert(CHOOSE || !GUARD, "the processors live in the instantiations that choose (the forced run scores the raw distribution)");
    constexpr int VEC = 16 / (int)sizeof(T), U = 16 / VEC;      // elements per 16-byte load, loads per trip: 16 values per thread and trip
    typedef typename std::conditional<sizeof(T) == 4, f32x4, typename ET<T>::v8>::type VT;
    __shared__ float sv[16];                     // the waves' maxima ...
    __shared__ int si[CHOOSE ? 16 : 1];          // ... CHOOSE: the ids that reached them first ...
    __shared__ float ss_lp[16];                  // ... and the waves' sums, each against its own maximum
    __shared__ float s_tkv[TOPK ? 128 : 1];      // TOPK: the waves' lists, [place][wave] ...
    __shared__ int s_tki[TOPK ? 128 : 1];        // ... and their ids
    __shared__ float s_tk_hand[2];               // thread 0 -> wave 1: the block's maximum and sum, the values the record's first float was formed from
    [[maybe_unused]] float tv[8]; [[maybe_unused]] int ti[8]; [[maybe_unused]] float mv = -INFINITY; [[maybe_unused]] int mi = TK_NONE;
    if constexpr (TOPK) tk_init(tv, ti);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (b >= a.n) return;
    const T* row = (const T*)a.logits + (long)b * a.ld;
    const int rec = a.rec[b], tgt = a.target[b];
    const bool vec_ok = (((unsigned long long)row) & 15ull) == 0;      // 16-byte loads where the row allows them; the visiting order is the same without
    float* dump = a.dump ? a.dump + ((long)(rec % a.out_ld) * a.R + rec / a.out_ld) * a.V : nullptr;
    const int ri = a.lp_by_row ? b : rec;      // where the row's record goes
    [[maybe_unused]] unsigned* g_seen = nullptr; [[maybe_unused]] unsigned* g_ban = nullptr;
    if constexpr (GUARD) {
        const int nw = (a.V + 31) >> 5;
        g_seen = v_bits; g_ban = v_bits + nw;
        for (int w = tid; w < 2 * nw; w += 1024) v_bits[w] = 0u;
        __syncthreads();
        hist_maps(g_seen, g_ban, a.hist + (long)a.hrow[b] * a.hist_ld, min(max(a.hlen[b], 0), a.hist_ld), a.ngram, a.suppress, a.n_suppress, a.V, tid);
        __syncthreads();
    }
    float best = -INFINITY, lp_m = -INFINITY, lp_s = 0.f;      // the thread's sum is lp_s * exp(lp_m); a thread that saw nothing holds (-inf, 0)
    [[maybe_unused]] int bi = TK_NONE;
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
            [[maybe_unused]] unsigned sb = 0u, bb = 0u;      // GUARD: the group's VEC bits of each map (i is a multiple of VEC, VEC divides 32)
            if constexpr (GUARD) if (i < a.V) { sb = g_seen[i >> 5] >> (i & 31); bb = g_ban[i >> 5] >> (i & 31); }
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float r = v[u][j];
                if (dump && i + j < a.V) dump[i + j] = r;
                if constexpr (GUARD) { r = guard_score(r, sb >> j, bb >> j, a.rep_penalty); v[u][j] = r; }
                if constexpr (CHOOSE) { if (r > best) { best = r; bi = i + j; } }      // strict > keeps the first maximum within a thread
                else best = fmaxf(best, r);
                if constexpr (TOPK) if (r > tv[7]) tk_insert(tv, ti, r, i + j);      // (a thread visits its ids in ascending order; -inf is never inserted)
            }
        }
        // the trip's values against the maximum so far: one rescale of the old sum, then the terms in visiting order.  While nothing finite has been seen the sum
        // stays 0: -inf - -inf is not formed, here or in the terms
        lp_s = lp_rescale(lp_s, lp_m, best); lp_m = best;
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < VEC; ++j) lp_s += best > -INFINITY ? lp_exp(v[u][j] - best) : 0.f;
    }
    if constexpr (CHOOSE) { FIRST_MAX_WAVE(best, bi) }
    else {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    }
    lp_s = lp_wave_fold(lp_s, lp_m, best);
    if (lane == 0) { sv[wid] = best; ss_lp[wid] = lp_s; if constexpr (CHOOSE) si[wid] = bi; }
    if constexpr (TOPK) tk_stage(tv, ti, a.topk, lane, wid, s_tkv, s_tki, mv, mi);
    __syncthreads();
    if constexpr (TOPK) if (wid == 1) tk_merge_waves(tv, ti, a.topk, lane, s_tkv, s_tki, mv, mi);      // beside thread 0's closing arithmetic
    if (tid == 0) {
        float M = sv[0];
        if constexpr (CHOOSE) {
            int mid = si[0];
            for (int w = 1; w < 16; ++w) if (sv[w] > M || (sv[w] == M && si[w] < mid)) { M = sv[w]; mid = si[w]; }
            a.choice[b] = mid == TK_NONE ? 0 : mid;     // every score -inf: the first of equal values
        } else {
            for (int w = 1; w < 16; ++w) M = fmaxf(M, sv[w]);
        }
        const float sum = lp_block_close(sv, ss_lp, M);
        if ((unsigned)tgt < (unsigned)a.V) {
            if (a.out_ids) a.out_ids[rec] = tgt;
            if (a.out_lp) {
                float lt = (float)row[tgt];
                if constexpr (GUARD) lt = guard_score(lt, g_seen[tgt >> 5] >> (tgt & 31), g_ban[tgt >> 5] >> (tgt & 31), a.rep_penalty);
                a.out_lp[(long)ri * (TOPK ? 1 + 2 * a.topk : 1)] = (float)(((double)lt - (double)M) - log((double)sum));
            }
        }
        s_tk_hand[0] = M; s_tk_hand[1] = sum;
    }
    if constexpr (TOPK) {
        __syncthreads();
        if (wid == 1 && lane < a.topk && a.out_lp) tk_record(a.out_lp + (long)ri * (1 + 2 * a.topk), a.topk, lane, mv, mi, s_tk_hand[0], s_tk_hand[1]);
    }
}

template <typename T, bool CHOOSE, bool GUARD> static void rows_launch(const RowsArgs& a, hipStream_t s) {
    const size_t lds = GUARD ? greedy_guard_lds(a.V) : 0;
    if (a.topk >= 1 && a.topk <= 8 && a.out_lp) hipLaunchKernelGGL((rows_kernel<T, CHOOSE, GUARD, true>), dim3(a.n), dim3(1024), lds, s, a);
    else hipLaunchKernelGGL((rows_kernel<T, CHOOSE, GUARD, false>), dim3(a.n), dim3(1024), lds, s, a);
}
// choice == NULL: the forced run's instantiations, the fp32 kind's among them.  Else hist != NULL: the GUARD ones (the caller has checked that greedy_guard_lds(V)
// fits, as sonic_set_generation does)
void launch_rows(const RowsArgs& a, hipStream_t s) {
    if (a.n < 1) return;
    if (!a.choice) {
        if (a.dt == DT_F32) { rows_launch<float, false, false>(a, s); return; }
        DT_SWITCH(a.dt, T, (rows_launch<T, false, false>(a, s)));
    } else if (a.hist) { DT_SWITCH(a.dt, T, (rows_launch<T, true, true>(a, s))); }
    else { DT_SWITCH(a.dt, T, (rows_launch<T, true, false>(a, s))); }
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

__global__ __launch_bounds__(256) void draft_accept_kernel(DraftAcceptArgs a) {
    __shared__ int s_a;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int D = a.req[r], row0 = a.req[64 + r], P = a.req[128 + r];      // the request's draft length, its first verify row, its prompt length
    if (D <= 0) { if (tid == 0) a.accepted[r] = 0; return; }             // no draft: the row stays as the plan set it
    if (tid == 0) s_a = D;
    __syncthreads();
    for (int n = tid; n < D; n += 256) if (a.ver_tok[row0 + n] != a.draft[row0 + n]) atomicMin(&s_a, n);
    __syncthreads();
    const int acc = s_a;
    for (int n = tid; n < acc; n += 256) a.out_ids[(long)r * a.out_ld + n] = a.draft[row0 + n];
    if (a.out_lp) for (int j = tid; j < acc * a.lp_w; j += 256) a.out_lp[(long)r * a.out_ld * a.lp_w + j] = a.ver_rec[(long)row0 * a.lp_w + j];
    if (tid == 0) {
        a.n_new[r] = acc; a.kv_len[r] = P + acc; a.step_counter[r] = acc;
        if (acc > 0) a.tok_pos[r] = P + acc - 1;      // where the last accepted token sits (a row that ends at the head keeps it: tok_pos = kv_len - 1)
        a.last_row[r] = a.req[192 + r] + P - 1 + acc;      // the hidden row that decides token `acc`
        a.accepted[r] = acc;
    }
}
void launch_draft_accept(const DraftAcceptArgs& a, int R, hipStream_t s) {
    if (R > 0) hipLaunchKernelGGL(draft_accept_kernel, dim3(R), dim3(256), 0, s, a);
}
