// Draft-verified decoding (option draft_verify): what the model itself would emit at every position of a draft, from the rows of the prefill's lm_head
// GEMM - and how much of the draft that accepts.
// verify_rows_kernel<T, GUARD, TOPK>: one block per draft position, one pass over the row's V logits in the activation type.  It is score_rows_kernel (score.hip) with
// a choice added: the visiting order (16 values per thread and trip, 16-byte loads where the row allows them), the sum of exp(s - max) per trip, the butterfly and the
// fixed tree over the waves, lp_exp and the fp64 closing step are that kernel's, statement by statement; beside the running maximum every thread keeps the id that
// reached it first (strict >: a thread visits its ids in ascending order), and the reductions prefer the lower id among equal values - torch.argmax's first maximum.
// A row whose scores are all -inf gives 0.  GUARD: the handle's processors (sonic_set_generation) on the scores, as greedy_kernel<T, ., true> applies them - the block
// builds the "seen" / "banned" bitmaps of the position's history hist[hrow][0 .. hlen) = prompt || draft[0 .. n) in LDS (that kernel's prologue) and every value goes
// through guard_score ahead of the compare, the sum and the lists; the dump stays raw.  The position's record - log_softmax(s)[draft id] and, with TOPK, the K best
// ids of s by (value descending, id ascending) - goes to a staging array [row][1 + 2K]: draft_accept_kernel copies the accepted ones.
// draft_accept_kernel: one block per request - the first position whose choice differs from the draft id (a = D when none does), the accepted ids and records into
// the request's output rows, and the row state a prefill of prompt || draft[0 .. a) would have left: n_new = step counter = a, kv_len = P + a, last_row = the hidden
// row that decides token a.  A request without a draft is left as the plan set it.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "guard.h"
#include "topk.h"

extern __shared__ unsigned v_bits[];
template <typename T, bool GUARD, bool TOPK>
__global__ __launch_bounds__(1024) void verify_rows_kernel(VerifyArgs a) {
    constexpr int VEC = 16 / (int)sizeof(T), U = 16 / VEC;      // elements per 16-byte load, loads per trip: 16 values per thread and trip
    typedef typename std::conditional<sizeof(T) == 4, f32x4, typename ET<T>::v8>::type VT;
    __shared__ float sv[16];                     // the waves' maxima ...
    __shared__ int si[16];                       // ... the ids that reached them first ...
    __shared__ float ss_lp[16];                  // ... and the waves' sums, each against its own maximum
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
    [[maybe_unused]] unsigned* g_seen = nullptr; [[maybe_unused]] unsigned* g_ban = nullptr;
    if constexpr (GUARD) {
        const int nw = (a.V + 31) >> 5;
        g_seen = v_bits; g_ban = v_bits + nw;
        for (int w = tid; w < 2 * nw; w += 1024) v_bits[w] = 0u;
        __syncthreads();
        // greedy_kernel's prologue on the position's history: seen = its ids; banned = the continuations of earlier occurrences of its last n - 1 ids, and the suppress list
        const int* h = a.hist + (long)a.hrow[b] * a.hist_ld;
        const int len = min(max(a.hlen[b], 0), a.hist_ld), n = a.ngram;
        for (int j = tid; j < len; j += 1024) guard_set(g_seen, h[j], a.V);
        if (n > 0) {
            const int* last = h + len - (n - 1);  // (read only when an n-gram exists: j + n <= len)
            for (int j = tid; j + n <= len; j += 1024) {
                bool m = true;
                for (int k = 0; k < n - 1; ++k) m = m && h[j + k] == last[k];
                if (m) guard_set(g_ban, h[j + n - 1], a.V);
            }
        }
        for (int j = tid; j < a.n_suppress; j += 1024) guard_set(g_ban, a.suppress[j], a.V);
        __syncthreads();
    }
    float best = -INFINITY, lp_m = -INFINITY, lp_s = 0.f;      // the thread's sum is lp_s * exp(lp_m); a thread that saw nothing holds (-inf, 0)
    int bi = TK_NONE;
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
                if (r > best) { best = r; bi = i + j; }      // strict > keeps the first maximum within a thread
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
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    // every lane now holds the wave's maximum: bring the lane's sum to it (an empty lane is the identity) and add across the wave - the butterfly gives every
    // lane the same tree, and a + b = b + a bit for bit
    lp_s = lp_m > -INFINITY ? lp_s * lp_exp(lp_m - best) : 0.f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lp_s += __shfl_xor(lp_s, o, 64);
    if (lane == 0) { sv[wid] = best; si[wid] = bi; ss_lp[wid] = lp_s; }
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
        float M = sv[0]; int mid = si[0];
        for (int w = 1; w < 16; ++w) if (sv[w] > M || (sv[w] == M && si[w] < mid)) { M = sv[w]; mid = si[w]; }
        float q[16];                              // the 16 waves at the block's maximum (an empty wave: 0), added as a fixed binary tree
#pragma unroll
        for (int w = 0; w < 16; ++w) q[w] = sv[w] > -INFINITY ? ss_lp[w] * lp_exp(sv[w] - M) : 0.f;
#pragma unroll
        for (int h = 8; h > 0; h >>= 1)
#pragma unroll
            for (int w = 0; w < h; ++w) q[w] = q[2 * w] + q[2 * w + 1];
        a.ver_tok[b] = mid == TK_NONE ? 0 : mid;     // every score -inf: the first of equal values
        if (a.ver_rec && (unsigned)tgt < (unsigned)a.V) {
            float lt = (float)row[tgt];
            if constexpr (GUARD) lt = guard_score(lt, g_seen[tgt >> 5] >> (tgt & 31), g_ban[tgt >> 5] >> (tgt & 31), a.rep_penalty);
            a.ver_rec[(long)b * (TOPK ? 1 + 2 * a.topk : 1)] = (float)(((double)lt - (double)M) - log((double)q[0]));
        }
        s_tk_hand[0] = M; s_tk_hand[1] = q[0];
    }
    if constexpr (TOPK) {
        __syncthreads();
        if (wid == 1 && lane < a.topk && a.ver_rec) {
            const int K = a.topk;
            float* r = a.ver_rec + (long)b * (1 + 2 * K);
            const bool any = mi != TK_NONE;
            r[1 + lane] = any ? (float)(((double)mv - (double)s_tk_hand[0]) - log((double)s_tk_hand[1])) : -INFINITY;
            r[1 + K + lane] = any ? (float)mi : -1.f;      // (ids stay below 2^24: exact)
        }
    }
}

template <typename T, bool GUARD> static void verify_launch(const VerifyArgs& a, hipStream_t s) {
    const size_t lds = GUARD ? greedy_guard_lds(a.V) : 0;
    if (a.topk >= 1 && a.topk <= 8 && a.ver_rec) hipLaunchKernelGGL((verify_rows_kernel<T, GUARD, true>), dim3(a.n), dim3(1024), lds, s, a);
    else hipLaunchKernelGGL((verify_rows_kernel<T, GUARD, false>), dim3(a.n), dim3(1024), lds, s, a);
}
// hist != NULL: the GUARD instantiations (the caller has checked that greedy_guard_lds(V) fits, as sonic_set_generation does)
void launch_verify_rows(const VerifyArgs& a, hipStream_t s) {
    if (a.n < 1) return;
    if (a.hist) { DT_SWITCH(a.dt, T, (verify_launch<T, true>(a, s))); }
    else { DT_SWITCH(a.dt, T, (verify_launch<T, false>(a, s))); }
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
