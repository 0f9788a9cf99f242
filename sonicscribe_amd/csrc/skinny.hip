// Decode-step GEMMs for gfx950, slab form: M <= 64 activation rows against a fragment-tiled weight matrix (tile_weights.hip).
//
//   skinny_kernel  partial[ks][M<=64][N] = X . W^T over a K slice  -- decode-step weight streaming (K10/K11)
//
// Three kernels (the one-shot register kernel, its bench-only read floor, the shared-X kernel), then the pickers that choose
// a tiling per shape, then the launchers, ending in launch_skinny.  The slabs are summed by the consumer (elementwise.hip, greedy.hip);
// the fused RMSNorm / SwiGLU / residual forms of the same step are in skinny_fused.hip.
#include <type_traits>

#include "common.h"
#include "int8_util.h"

// ------------------------------------------------------------------------------------------------
// skinny_kernel: decode-step GEMM, M <= 64 rows.  HBM-bound weight streaming: every weight byte is read once, straight
// to VGPRs (no LDS round trip for an operand no other wave shares).  The step is latency-bound, not bandwidth-bound, so
// the kernel is "one-shot": a block owns 16 weight rows x (8 waves * KW * 32) of K; every wave issues ALL of its weight
// loads (nontemporal, 1 KiB each) and activation loads before its first MFMA, so the whole matrix is in flight at once.
// D[n][m] (A-operand = W rows, B-operand = X rows); the 8 K-slices of a block are summed through LDS in fixed order
// (deterministic, no float atomics) and stored as fp32.  K = 2048 needs no split at all (one slab); down_proj
// (K = 6144) leaves 3 slabs for its consumer.
template <typename KD, int MB, int KW, bool NT>
__global__ __launch_bounds__(512) void skinny_kernel(SkinnyArgs a) {
    typedef typename KD::elem ET_; typedef typename KD::frag Frag;
    __shared__ f32x4 red[8][MB][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int kb = (blockIdx.y * 8 + wid) * (KW * 32);
    // fragment-tiled weights (tile_weights_kernel): k-step s of row tile t is the contiguous 1 KiB block (t*K/32 + s)
    const ET_* wp = (const ET_*)a.W + ((long)blockIdx.x * (a.K >> 5) + (kb >> 5)) * 512 + lane * 8;
    Frag wf[KW];
#pragma unroll
    for (int u = 0; u < KW; ++u) wf[u] = NT ? __builtin_nontemporal_load((const Frag*)(wp + u * 512)) : *(const Frag*)(wp + u * 512);
    Frag xf[MB][KW];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        int row = mb * 16 + r; row = row < a.M ? row : a.M - 1;
        const ET_* xp = (const ET_*)a.X + (long)row * a.ldx + kb + g * 8;
#pragma unroll
        for (int u = 0; u < KW; ++u) xf[mb][u] = *(const Frag*)(xp + u * 32);
    }
    f32x4 acc[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < KW; ++u)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[mb] = KD::mfma(wf[u], xf[mb][u], acc[mb]);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) red[wid][mb][lane] = acc[mb];
    __syncthreads();
    const int mpad = MB * 16;
    for (int o = tid; o < 16 * mpad; o += 512) {
        const int m = o >> 4, nl = o & 15, mb = m >> 4, ln = (nl >> 2) * 16 + (m & 15), j = nl & 3;
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) s += red[w][mb][ln][j];
        a.P[((long)blockIdx.y * mpad + m) * a.N + n0 + nl] = s;
    }
}

// floor: read the same weight bytes, fully coalesced 16 B/lane, one-shot, trivially reduced (bench only)
template <int KW>
__global__ __launch_bounds__(512) void skinny_readfloor_kernel(SkinnyArgs a) {
    const int tid = threadIdx.x;
    const bf16_t* base = a.W + ((long)blockIdx.x * gridDim.y + blockIdx.y) * (8L * KW * 512) ;
    bf16x8 v[KW];
#pragma unroll
    for (int u = 0; u < KW; ++u) v[u] = __builtin_nontemporal_load((const bf16x8*)(base + ((long)u * 512 + tid) * 8));
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < KW; ++u) s += bf2f(v[u][0]) + bf2f(v[u][7]);
    if (s == 123.456f) a.P[0] = s;
}

// skinny_xs_kernel: the decode-step GEMM with the activation slice SHARED through LDS.  Measured on MI355X (tools/
// bench_skinny.py): the weight stream is not the limiter of the one-shot kernels above -- their time scales with M,
// i.e. with the per-wave 64-byte-per-row gathers of X out of L2.  Here a block owns BN = 16*WN weight rows and a K slice
// of BKk = WK*KSW*32; the X slice [M][BKk] is DMA'd ONCE per block into LDS in full 128-byte lines (swizzled on the
// source address, conflict-free ds_read_b128 fragments) and read by all 8 waves; weights go straight to VGPRs from the
// fragment-tiled copy (every wave load is one contiguous 1 KiB, each weight byte read once, nontemporal).  The WK
// K-slices of a block are summed through LDS; K/BKk slabs are left for the consumer (2 for K = 2048 with BKk = 1024).
// NT = 16-row weight tiles per wave (default 1).  The per-CU vector-memory pipe bounds these kernels (W bytes + the X image of every
// block that lands on the CU), so at 48-64 activation rows - where the image of a 1024-deep slice is 64 KiB of int8 - a block should own as
// many weight rows as keeps the grid at one block per CU: gate/up of the full-size model as 96 rows x 1024 (128 x 2 = 256 blocks, 96 KiB
// of W per 64 KiB image) instead of 32 rows x 1024 (768 blocks, three images per CU).
// XQ (int8 kind): the activation rows arrive unquantised (fp16) with their absmax; the block quantises its slice on the way into LDS.  This
// removes the separate one-block-per-row quantisation launch between a producer that does not own whole rows (decode attention: one block
// per (row, kv head); the fused gate/up kernel: 24 columns per block) and the projection that consumes it.
// PRE (16-bit kinds, M <= 2; round 6): the block computes its X slice itself from the PREVIOUS projection's slabs - X = RMSNorm(x + sum of slabs), the
// arithmetic of add_rmsnorm_kernel statement by statement (thread c of a row's 256 owns columns 8c .. 8c + 7; slabs added in ascending order from 0.f;
// sum of squares per thread in column order, wave butterfly, the row's four wave partials in order) - so the standalone add+RMSNorm launch between
// down_proj and the next q|k|v projection (or the lm_head) disappears at no change of any bit.  Every block redoes the whole row (it needs the row's
// sum of squares): 68 KiB of slab and residual reads per row and block out of L2, which pays below three rows.  The updated residual row is written
// by block (0, 0) to a SECOND buffer (other blocks still read the old one), so the residual stream ping-pongs between two buffers layer by layer.
template <typename KD, int MB, int WN, int WK, int KSW, int NT = 1, bool XQ = false, bool PRE = false>
__global__ __launch_bounds__(512) void skinny_xs_kernel(SkinnyArgs a) {
    typedef typename KD::elem ET_; typedef typename KD::frag Frag; typedef typename KD::acc Acc;
    // element size; elements per 16-B chunk, per MFMA k-step, per 128-B LDS row, per 1-KiB weight tile
    constexpr int EB = sizeof(ET_), CE = 16 / EB, KS = 64 / EB, ROWE = 128 / EB, TILE_E = 1024 / EB;
    constexpr int BKk = WK * KSW * KS, NKB = BKk / ROWE, RG = MB * 2, NI = NKB * RG, KBS = MB * 2048, PW = (NI + 7) / 8;
    constexpr int NL = NT * KSW;                                     // weight loads of a wave
    static_assert(WN * WK == 8 && (WK * KSW) % 2 == 0, "8 waves, whole 128-byte K blocks");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int wn = wid % WN, wk = wid / WN;
    const int n0 = blockIdx.x * (WN * NT * 16) + wn * NT * 16;
    const int kb = blockIdx.y * BKk;
    KT(a, 0);
    // X slice first (small, out of L2): it has to be complete in LDS - for all waves - before the first MFMA
    // XQ: fp16 rows -> registers (asm loads: the compiler must not see them, or its own wait counts would include the weight loads below),
    // G8 = groups of 8 elements per row of the slice; group idx = p * 512 + tid of the MB * 16 * G8 groups: row idx / G8, group idx % G8
    constexpr int G8 = BKk / 8, XTOT = MB * 16 * G8, XP = XQ ? (XTOT + 511) / 512 : 1;
    static_assert(!XQ || KD::I8, "XQ: int8 kind");
    f16x8 xq[XP]; f32x4 xam[XP];
    if constexpr (XQ) {
#pragma unroll
        for (int p = 0; p < XP; ++p) {
            const int idx = min(p * 512 + tid, XTOT - 1);
            int row = idx / G8; row = row < a.M ? row : a.M - 1;
            const f16_t* src = (const f16_t*)a.X + (long)row * a.ldx + kb + (idx % G8) * 8;
            const float* am = a.x_amax + row * 4;
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xq[p]) : "v"(src) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xam[p]) : "v"(am) : "memory");
        }
    } else if constexpr (PRE) {
        // requested below, beside the weights (asm loads + one counted wait: the weights stay in flight while the rows are normalised)
    } else {
        const int lr = lane >> 3, lc = (lane & 7) ^ lr;
#pragma unroll
        for (int t = 0; t < PW; ++t) {
            const int ii = NI % 8 == 0 ? wid * PW + t : wid + t * 8;
            if (NI % 8 == 0 || ii < NI) {
                const int kblock = ii / RG, rg = ii % RG;
                int row = rg * 8 + lr; row = row < a.M ? row : a.M - 1;
                const ET_* src = (const ET_*)a.X + (long)row * a.ldx + kb + kblock * ROWE + lc * CE;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(smem + ii * 1024), 16, 0, 0);
            }
        }
    }
    // PRE: this thread's share of the previous projection's slabs, the residual row and the norm weight (19 loads of 16 bytes), requested first
    static_assert(!PRE || (!KD::I8 && !XQ), "PRE: 16-bit kinds");
    __shared__ float pre_part[8];
    const int prow = tid >> 8, pc = tid & 255;                       // PRE: row 0 -> threads 0 .. 255, row 1 -> 256 .. 511
    const bool pvalid = PRE && prow < a.M && pc < (a.K >> 3);
    f32x4 pnw0, pnw1, psl0[8], psl1[8]; i32x4 pxr;
    if constexpr (PRE) {
        const int cc = pvalid ? pc : 0, rr = prow < a.M ? prow : 0;
        const float* wq = a.pre_w + cc * 8;
        const ET_* xq = (const ET_*)a.pre_x + (long)rr * a.K + cc * 8;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(pnw0) : "v"(wq) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=v"(pnw1) : "v"(wq) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(pxr) : "v"(xq) : "memory");
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const float* sp = a.pre_P + ((long)(ks < a.pre_ks ? ks : 0) * a.pre_mpad + rr) * a.K + cc * 8;
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(psl0[ks]) : "v"(sp) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=v"(psl1[ks]) : "v"(sp) : "memory");
        }
    }
    // then the weights (HBM, nontemporal): asm loads with hand-counted waits, so that k-step u is multiplied as soon as ITS fragment
    // has landed (vmcnt retires in order) instead of after the whole slice - the compiler's own bookkeeping falls back to vmcnt(0)
    // when LDS-DMA and register loads are in flight together
    const long tile_stride = (long)(a.K / KS) * TILE_E;              // elements between the 16-row tiles n and n + 16 at one k-step
    const ET_* wp = (const ET_*)a.W + ((long)(n0 >> 4) * (a.K / KS) + ((kb + wk * (KSW * KS)) / KS)) * TILE_E + lane * CE;
    Frag wf[NT][KSW];
#pragma unroll
    for (int u = 0; u < KSW; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const ET_* wpt = wp + t * tile_stride;
            if (u < 4) asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=v"(wf[t][u]) : "v"(wpt), "n"(u * 1024) : "memory");
            else asm volatile("global_load_dwordx4 %0, %1, off offset:%2 nt" : "=v"(wf[t][u]) : "v"(wpt + (u / 4) * 4 * TILE_E), "n"((u % 4) * 1024) : "memory");
        }
    Acc acc[NT][MB];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][mb][e] = 0;
    KT(a, 1);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NL) : "memory");       // this wave's X pieces are in LDS (XQ / PRE: in registers)
    if constexpr (PRE) {
        typedef typename std::conditional<std::is_same<ET_, f16_t>::value, f16x8, bf16x8>::type PV8;
        asm volatile("" : "+v"(pnw0), "+v"(pnw1), "+v"(pxr));
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+v"(psl0[ks]), "+v"(psl1[ks]));
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            if (ks < a.pre_ks) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc[j] += psl0[ks][j]; acc[4 + j] += psl1[ks][j]; }
            }
        const PV8 tx = __builtin_bit_cast(PV8, pxr);
        PV8 ox; float v[8]; float ssq = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { ox[j] = (ET_)((float)tx[j] + rT<ET_>(acc[j])); v[j] = (float)ox[j]; ssq += v[j] * v[j]; }
        if (!pvalid) ssq = 0.f;
        if (pvalid && a.pre_xout && blockIdx.x == 0 && blockIdx.y == 0) *(PV8*)((ET_*)a.pre_xout + (long)prow * a.K + pc * 8) = ox;
        ssq = wave_sum(ssq);
        if (lane == 0) pre_part[wid] = ssq;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                // (raw barrier: __syncthreads would add a vmcnt(0) fence - the weights are still in flight)
        asm volatile("" ::: "memory");
        float tot = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) tot += pre_part[(prow & 1) * 4 + i];
        const float rs = 1.0f / sqrtf(tot / a.K + a.pre_eps);
        const int kcol = pc * 8 - kb;                                // this thread's 8 columns inside the block's K slice?
        if (pvalid && kcol >= 0 && kcol < BKk) {
            PV8 oy;
#pragma unroll
            for (int j = 0; j < 8; ++j) oy[j] = (ET_)((j < 4 ? pnw0[j & 3] : pnw1[j & 3]) * rT<ET_>(v[j] * rs));
            const int kblock = kcol / ROWE, ch = (kcol % ROWE) / CE;
            // image rows beyond M hold copies of the last row (as the DMA path's clamped rows): their outputs are never consumed
            for (int m = prow; m < MB * 16; m += (prow == a.M - 1 ? 1 : MB * 16))
                *(PV8*)(smem + kblock * KBS + m * 128 + ((ch ^ (m & 7)) << 4)) = oy;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if constexpr (XQ) {
        // quantise (int8_util.h quant_emit_row's arithmetic) and park in the image: byte (row m, element k) of a 128-element k-block at
        // kblock * KBS + m * 128 + ((chunk ^ (m & 7)) << 4) + k % 16
#pragma unroll
        for (int p = 0; p < XP; ++p) {
            asm volatile("" : "+v"(xq[p]), "+v"(xam[p]));
            const int idx = p * 512 + tid;
            if (XTOT % 512 != 0 && idx >= XTOT) continue;
            const int m = idx / G8, g8 = idx % G8, kblock = g8 >> 4, c = (g8 & 15) >> 1, half = g8 & 1;
            const float bm = fmaxf(fmaxf(xam[p][0], xam[p][1]), fmaxf(xam[p][2], xam[p][3])), scale = 127.0f / bm;
            int pk[2] = {0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float y = (float)xq[p][j];
                const bool out = !(fabsf(y) < LLM_INT8_THRESHOLD);
                const int qv = (out || !(bm > 0.f)) ? 0 : (int)rintf(y * scale);
                pk[j >> 2] |= (qv & 0xFF) << ((j & 3) * 8);
            }
            *(int2*)(smem + kblock * KBS + m * 128 + ((c ^ (m & 7)) << 4) + half * 8) = make_int2(pk[0], pk[1]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();                                    // (raw barrier: __syncthreads would add a vmcnt(0) fence)
    KT(a, 2);
#pragma unroll
    for (int u = 0; u < KSW; ++u) {
        const int kg = wk * KSW + u, kblock = kg >> 1, half = kg & 1;
        Frag xf[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int m = mb * 16 + r;
            xf[mb] = *(const Frag*)(smem + kblock * KBS + m * 128 + (((half * 4 + g) ^ (m & 7)) << 4));
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            asm volatile("s_waitcnt vmcnt(%1)" : "+v"(wf[t][u]) : "n"(NL - 1 - (u * NT + t)) : "memory");
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) acc[t][mb] = KD::mfma(wf[t][u], xf[mb], acc[t][mb]);
        }
    }
    KT(a, 3);
    __syncthreads();
    KT(a, 4);
    Acc* red = (Acc*)smem;   // [WK][WN * NT][MB][64]
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) red[((wk * (WN * NT) + wn * NT + t) * MB + mb) * 64 + lane] = acc[t][mb];
    __syncthreads();
    constexpr int BNR = WN * NT * 16, mpad = MB * 16;
    const int nb0 = blockIdx.x * BNR;
    // One (16-row tile, 16-row block of X) per wave-iteration: a lane adds the WK partials of its own accumulator position (whole fragments,
    // ds_read_b128, ascending k from zero as before - same bits) and stores its four consecutive columns at once.  (Round 4 walked the outputs one
    // by one: WK scalar LDS reads and a 4-byte store each, 4 - 8 store instructions per wave: 1.1 us of a 4.6 us kernel.)
    for (int task = wid; task < WN * NT * MB; task += 8) {
        const int wn2 = task / MB, mb = task % MB;
        Acc sum;
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[e] = 0;
#pragma unroll
        for (int k = 0; k < WK; ++k) {
            const Acc v = red[((k * (WN * NT) + wn2) * MB + mb) * 64 + lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[e] += v[e];
        }
        // D[n][m]: lane (r, g) holds columns 4g .. 4g + 3 of X row r; int8: exact int32 partial products, the consumer dequantises (int8_util.h)
        *(Acc*)((typename std::conditional<KD::I8, int, float>::type*)a.P + ((long)blockIdx.y * mpad + mb * 16 + r) * a.N + nb0 + wn2 * 16 + 4 * g) = sum;
    }
    KT(a, 5);
}

static int skinny_pick_kw(int K) {
    for (int kw = 8; kw >= 1; kw >>= 1)
        if (K % (256 * kw) == 0 && K / (256 * kw) <= 8) return kw;
    return 0;
}
// config: 1 = BIG (64 rows x 1024 k per block), 3 = 64 rows x 768 k, 2 = SMALL (32 rows x 512 k), 0 = one-shot register kernel (small K)
static int skinny_pick_cfg(int N, int K) {
    if (g_opts.skinny_variant >= 2) return 0;
    // 768-deep slices where they put a block on more CUs than 1024-deep ones without exceeding one block per CU: down_proj of the full-size
    // model (2048 x 6144) is 32 x 8 = 256 blocks instead of 32 x 6 = 192 - the weight stream is bound by how many CUs pull it
    if (!g_opts.no_skinny768 && K % 768 == 0 && N % 64 == 0 && K / 768 <= 8 && (long)(N / 64) * (K / 768) <= 256 &&
        (K % 1024 != 0 || (long)(N / 64) * (K / 768) > (long)(N / 64) * (K / 1024)) && (long)(N / 64) * (K / 768) >= 192) return 3;
    if (K % 1024 == 0 && N % 64 == 0 && K / 1024 <= 8 && (long)(N / 64) * (K / 1024) >= 192) return 1;
    // 48 rows x 512 where that is one block per CU and 32 x 512 is not: the QKV projection of the full-size model (3072 x 2048) as 64 x 4 = 256 blocks
    // instead of 96 x 4 = 384 (half of the CUs got two blocks, each with its own 32 - 64 KiB X image through the CU's vector-memory path)
    if (!g_opts.no_skinny48 && K % 512 == 0 && N % 48 == 0 && K / 512 <= 8 && (long)(N / 48) * (K / 512) <= 256 && (long)(N / 48) * (K / 512) >= 192 &&
        (long)(N / 32) * (K / 512) > 256) return 4;
    if (K % 512 == 0 && N % 32 == 0 && K / 512 <= 8) return 2;
    if (K % 1024 == 0 && N % 64 == 0 && K / 1024 <= 8) return 1;
    return 0;
}
int skinny_pick_ksplit(int N, int K) {
    const int cfg = skinny_pick_cfg(N, K);
    if (cfg == 1) return K / 1024;
    if (cfg == 3) return K / 768;
    if (cfg == 2 || cfg == 4) return K / 512;
    const int kw = skinny_pick_kw(K);
    return kw ? K / (256 * kw) : 0;
}

template <typename KD, int MB, int KW> static void launch_skinny_v(const SkinnyArgs& a, hipStream_t s) {
    dim3 grid(a.N / 16, a.ksplit), block(512);
    const int v = g_opts.skinny_variant;
    if (v == 9) hipLaunchKernelGGL((skinny_readfloor_kernel<KW>), grid, block, 0, s, a);
    else if (v == 3) hipLaunchKernelGGL((skinny_kernel<KD, MB, KW, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((skinny_kernel<KD, MB, KW, true>), grid, block, 0, s, a);
}
template <typename KD, int MB> static void launch_skinny_mb(const SkinnyArgs& a, int kw, hipStream_t s) {
    switch (kw) {
        case 8: launch_skinny_v<KD, MB, 8>(a, s); break;
        case 4: launch_skinny_v<KD, MB, 4>(a, s); break;
        case 2: launch_skinny_v<KD, MB, 2>(a, s); break;
        default: launch_skinny_v<KD, MB, 1>(a, s); break;
    }
}
template <typename KD, int MB, int WN, int WK, int KSW, int NT = 1, bool XQ = false, bool PRE = false> static void launch_xs_v(const SkinnyArgs& a, int nkslices, hipStream_t s) {
    constexpr int EB = sizeof(typename KD::elem), KS = 64 / EB, ROWE = 128 / EB;
    constexpr int NI = (WK * KSW * KS / ROWE) * MB * 2;
    const size_t img = (size_t)NI * 1024, red = (size_t)8 * NT * MB * 1024, lds = img > red ? img : red;
    if (lds > 65536) ensure_dyn_lds((const void*)skinny_xs_kernel<KD, MB, WN, WK, KSW, NT, XQ, PRE>, (int)lds);
    hipLaunchKernelGGL((skinny_xs_kernel<KD, MB, WN, WK, KSW, NT, XQ, PRE>), dim3(a.N / (WN * NT * 16), nkslices), dim3(512), lds, s, a);
}
// PRE form (SkinnyArgs.pre_P): M <= 2, 16-bit kinds, any of the shared-X tilings
bool skinny_pre_eligible(int M, int N, int K) { return M >= 1 && M <= 2 && K % 8 == 0 && K <= 2048 && skinny_pick_cfg(N, K) != 0; }
template <typename KD> static void launch_skinny_xs_pre(const SkinnyArgs& a, int cfg, hipStream_t s) {
    if (cfg == 1) launch_xs_v<KD, 1, 4, 2, 16, 1, false, true>(a, a.K / 1024, s);
    else if (cfg == 3) launch_xs_v<KD, 1, 4, 2, 12, 1, false, true>(a, a.K / 768, s);
    else if (cfg == 4) launch_xs_v<KD, 1, 1, 8, 2, 3, false, true>(a, a.K / 512, s);
    else launch_xs_v<KD, 1, 2, 4, 4, 1, false, true>(a, a.K / 512, s);
}
template <typename KD, int MB> static void launch_skinny_xs(const SkinnyArgs& a, int cfg, hipStream_t s) {
    if (cfg == 1) launch_xs_v<KD, MB, 4, 2, 16>(a, a.K / 1024, s);
    else if (cfg == 3) launch_xs_v<KD, MB, 4, 2, 12>(a, a.K / 768, s);
    else if (cfg == 4) launch_xs_v<KD, MB, 1, 8, 2, 3>(a, a.K / 512, s);
    else launch_xs_v<KD, MB, 2, 4, 4>(a, a.K / 512, s);
}
// int8 operands (Linear8bitLt decode step): 32 * NT weight rows x (4 * KSW * 64) of K per block.  The slabs are exact int32 sums, so the
// K split changes no bit of the result and is chosen per shape for one block per CU (full-size model, 256 CUs):
//   cfg 1  96 rows x 1024   gate/up 128 x 2 = 256 blocks          (N % 96 == 0, K % 1024 == 0, >= 192 blocks)
//   cfg 2  64 rows x  768   down     32 x 8 = 256 blocks          (N % 64 == 0, K % 768 == 0, <= 8 slices, >= 192 blocks)
//   cfg 3  32 rows x  512   o_proj   64 x 4 = 256 blocks          (K % 512 == 0, <= 8 slices, 32 x 1024 would give < 192 blocks, this <= 320)
//   cfg 0  32 rows x 1024   q/k/v    96 x 2 = 192 blocks          (K % 1024 == 0)
//   cfg 4  32 rows x  256   tiny test configurations              (K % 256 == 0)
int skinny_i8_cfg(int N, int K) {
    if (N % 32) return -1;
    if (!g_opts.no_skinny_i8_wide) {
        if (K % 1024 == 0 && N % 96 == 0 && (long)(N / 96) * (K / 1024) >= 192) return 1;
        if (K % 768 == 0 && N % 64 == 0 && K / 768 <= 8 && (long)(N / 64) * (K / 768) >= 192 && (long)(N / 64) * (K / 768) <= 320) return 2;
        if (K % 1024 == 0 && (long)(N / 32) * (K / 1024) < 192 && K / 512 <= 8 && (long)(N / 32) * (K / 512) <= 320) return 3;
    }
    if (K % 1024 == 0) return 0;
    if (K % 256 == 0) return 4;
    return -1;
}
int skinny_pick_ksplit_i8(int N, int K) {
    switch (skinny_i8_cfg(N, K)) {
        case 0: case 1: return K / 1024;
        case 2: return K / 768;
        case 3: return K / 512;
        case 4: return K / 256;
        default: return 0;
    }
}
template <int MB> static void launch_skinny_i8(const SkinnyArgs& a, hipStream_t s) {
    if (a.x_amax) {                  // fp16 rows quantised while staged (the configurations the decode step uses for o_proj / down_proj)
        switch (skinny_i8_cfg(a.N, a.K)) {
            case 2: launch_xs_v<KI8, MB, 2, 4, 3, 2, true>(a, a.K / 768, s); break;
            case 3: launch_xs_v<KI8, MB, 2, 4, 2, 1, true>(a, a.K / 512, s); break;
            case 0: case 1: launch_xs_v<KI8, MB, 2, 4, 4, 1, true>(a, a.K / 1024, s); break;
            default: launch_xs_v<KI8, MB, 2, 4, 1, 1, true>(a, a.K / 256, s); break;
        }
        return;
    }
    switch (skinny_i8_cfg(a.N, a.K)) {
        case 1: launch_xs_v<KI8, MB, 2, 4, 4, 3>(a, a.K / 1024, s); break;
        case 2: launch_xs_v<KI8, MB, 2, 4, 3, 2>(a, a.K / 768, s); break;
        case 3: launch_xs_v<KI8, MB, 2, 4, 2>(a, a.K / 512, s); break;
        case 0: launch_xs_v<KI8, MB, 2, 4, 4>(a, a.K / 1024, s); break;
        default: launch_xs_v<KI8, MB, 2, 4, 1>(a, a.K / 256, s); break;
    }
}
template <typename KD> static void launch_skinny_16(const SkinnyArgs& a, hipStream_t s) {
    const int cfg = skinny_pick_cfg(a.N, a.K);
    const int mb = (a.M + 15) / 16;
    if (a.pre_P) { launch_skinny_xs_pre<KD>(a, cfg, s); return; }      // (the caller checked skinny_pre_eligible)
    if (cfg) { MB_SWITCH(mb, MB, launch_skinny_xs<KD, MB>(a, cfg, s)); return; }
    const int kw = skinny_pick_kw(a.K);
    MB_SWITCH(mb, MB, launch_skinny_mb<KD, MB>(a, kw, s));
}
void launch_skinny(const SkinnyArgs& a, hipStream_t s) {
    if (a.i8) { MB_SWITCH((a.M + 15) / 16, MB, launch_skinny_i8<MB>(a, s)); return; }
    if (a.dt == DT_F16) launch_skinny_16<KF16>(a, s); else launch_skinny_16<KBF16>(a, s);
}
