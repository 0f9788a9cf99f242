// bf16 MFMA GEMMs for gfx950.
//
//   gemm_kernel    C[M][N] = A[M][K] . W[N][K]^T (+ epilogue)      -- encoder / projector / prefill linears,
//                  conv stem as im2col-free GEMM (torch nn.Linear layout, so both
//                  operands are K-contiguous and every MFMA fragment is one 16-byte LDS read)
//
// gemm_kernel: 128x128x64 block tile, 4 waves (2x2), 64x64 per wave as 4x4 v_mfma_f32_16x16x32_bf16,
// operands staged HBM->LDS with global_load_lds_dwordx4 (16 B/lane, lane-linear LDS image), XOR
// swizzle applied on the *source* address and again on the fragment read (chunk ^= row & 7) so the
// ds_read_b128 fragment reads are bank-conflict free; two LDS stages, next tile's DMA in flight
// under the current tile's MFMAs; one barrier per K step.  MFMA roles are swapped (A-operand = W
// rows, B-operand = activation rows) so each lane ends up with 4 consecutive output columns of one
// row and the epilogue stores 8-byte bf16 quads.
#include <type_traits>

#include "common.h"
#include "int8_util.h"

#define BM 128
#define BN 128
#define BK 64
#define STAGE_BYTES ((BM + BN) * BK * 2)

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// NS = stages of the operand ring.  2: one k-step in flight, two blocks per CU hide each other's load latency (large grids).  4: three k-steps in
// flight with counted waits, one block per CU - for grids that do not fill the chip anyway (the <= 128 ragged rows a prefill GEMM cuts off its
// 256x256 launch: 16 blocks whose k-step was one full L2 round trip, 0.54 us, with NS = 2).  Same k order per accumulator: same bits.
// WM x WN = 16x16 MFMA tiles per wave (4 waves as 2 x 2): block tile (32 WM) x (32 WN).  4 x 4 = 128 x 128 is the general kernel; 1 x 2 =
// 32 x 64 is for problems of a few hundred rows (the ragged tail rows, the streaming partials): such a GEMM is bound by how many CUs pull
// operands (~65 GB/s each), and 16 tiles of 128 x 128 leave 240 CUs idle - 52 us for the 128 x 2048 x 6144 tail of a prefill down_proj.
// Every output element still sums its k-blocks of 32 in ascending order on the same MFMA instruction: the tile shape changes no bit.
template <typename KD, int EPI, int NS = 2, int WM = 4, int WN = 4>
__global__ __launch_bounds__(256, NS == 2 ? 2 : 1) void gemm_kernel(GemmArgs a) {
    constexpr int TBM = 32 * WM, TBN = 32 * WN, TSTAGE = (TBM + TBN) * BK * 2;
    static_assert(EPI != EPI_SWIGLU || WN % 2 == 0, "gate / up pairs of 16-column groups per wave");
    typedef typename KD::elem ET_; typedef typename KD::out OT; typedef typename KD::frag Frag; typedef typename KD::acc Acc;
    typedef typename ET<OT>::v4 O4;
    constexpr int EB = sizeof(ET_), CE = 16 / EB, BKE = 128 / EB;   // bytes per element, elements per 16-B chunk / per 128-B tile row
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;

    // ---- tile id: XCD-aware (blocks b, b+8, ... share an L2) + grouped raster (8 tile-rows per group)
    const int tilesM = (a.M + TBM - 1) / TBM, tilesN = (a.N + TBN - 1) / TBN;
    const int nt = tilesM * tilesN;
    int id;
    {
        const int bid = blockIdx.x, q = nt >> 3, r = nt & 7, xcd = bid & 7, loc = bid >> 3;
        id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    int tm, tn;
    {
        const int GM = 8, gsz = GM * tilesN, g = id / gsz, first = g * GM;
        const int gm = min(GM, tilesM - first), in = id - g * gsz;
        tm = first + in % gm;
        tn = in / gm;
    }
    const int m0 = tm * TBM, n0 = tn * TBN;
    const ET_* A = (const ET_*)a.A + (long)blockIdx.z * a.strideA;
    OT* C = (OT*)a.C + (long)blockIdx.z * a.strideC;
    const OT* R = (EPI == EPI_BIAS_RESID) ? (const OT*)a.R + (long)blockIdx.z * a.strideR : nullptr;

    // ---- per-lane DMA source pointers (4 row groups of 8 rows per wave, per operand)
    const int lr = lane >> 3, lp = lane & 7, lc = lp ^ lr;  // LDS row-in-group, physical chunk, logical chunk
    const ET_* srcA[WM];                                     // (WM / WN row groups of 8 rows per wave and operand)
    const ET_* srcW[WN];
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        int ra = m0 + (wid * WM + i) * 8 + lr; ra = ra < a.M ? ra : a.M - 1;
        srcA[i] = A + (long)ra * a.lda + lc * CE;
    }
#pragma unroll
    for (int i = 0; i < WN; ++i) {
        int rw = n0 + (wid * WN + i) * 8 + lr; rw = rw < a.N ? rw : a.N - 1;
        srcW[i] = (const ET_*)a.W + (long)rw * a.K + lc * CE;
        if (a.w_tiled) {
            // fragment-tiled W (GemmArgs.w_tiled): piece wid * WN + i of the stage = (row tile p >> 1, k-step p & 1), 1 KiB contiguous, lane-linear
            const int p = wid * WN + i;
            int nb = n0 + (p >> 1) * 16; nb = nb + 16 <= a.N ? nb : a.N - 16;
            srcW[i] = (const ET_*)a.W + ((long)(nb >> 4) * (a.K / (BKE / 2)) + (p & 1)) * (BKE / 2 * 16) + lane * CE;
        }
    }
    const int kmulW = a.w_tiled ? 16 : 1;
    auto stage_load = [&](int stage, int k0) {
        char* sA = smem + stage * TSTAGE;
        char* sB = sA + TBM * BK * 2;
#pragma unroll
        for (int i = 0; i < WM; ++i) glds16(srcA[i] + k0, sA + (wid * WM + i) * 1024);
#pragma unroll
        for (int i = 0; i < WN; ++i) glds16(srcW[i] + k0 * kmulW, sB + (wid * WN + i) * 1024);
    };

    Acc acc[WN][WM];  // [ni][mi]
#pragma unroll
    for (int i = 0; i < WN; ++i)
#pragma unroll
        for (int j = 0; j < WM; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][j][e] = 0;

    const bool vtile = (EPI == EPI_QKV_VT) && (n0 >= a.n_split);
    const int fr = lane & 15, fg = lane >> 4;
    const int nk = a.K / BKE;
#pragma unroll
    for (int p = 0; p < NS - 1; ++p) stage_load(p, min(p, nk - 1) * BKE);
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt % NS;
        // stage kt has landed when at most NS - 2 later stage loads (WM + WN DMA instructions each) are still in flight
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * (WM + WN)) : "memory");
        __syncthreads();
        // the slot consumed in step kt - 1 is free for step kt + NS - 1 (past the end: the last block again, into a slot nobody reads - keeps
        // the wait counts constant)
        if (NS > 2 || kt + 1 < nk) stage_load((kt + NS - 1) % NS, min(kt + NS - 1, nk - 1) * BKE);
        const char* sA = smem + cur * TSTAGE;
        const char* sB = sA + TBM * BK * 2;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            Frag xf[WM], wf[WN];
            const int c = kk * 4 + fg;
#pragma unroll
            for (int i = 0; i < WM; ++i) {
                const int rx = wr * (WM * 16) + i * 16 + fr;
                xf[i] = *(const Frag*)(sA + rx * 128 + ((c ^ (rx & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < WN; ++i) {
                const int rw = wc * (WN * 16) + i * 16 + fr;
                wf[i] = *(const Frag*)(sB + (a.w_tiled ? ((wc * WN + i) * 2 + kk) * 1024 + lane * 16 : rw * 128 + ((c ^ (rw & 7)) << 4)));
            }
            if (vtile) {
#pragma unroll
                for (int ni = 0; ni < WN; ++ni)
#pragma unroll
                    for (int mi = 0; mi < WM; ++mi) acc[ni][mi] = KD::mfma(xf[mi], wf[ni], acc[ni][mi]);
            } else {
#pragma unroll
                for (int ni = 0; ni < WN; ++ni)
#pragma unroll
                    for (int mi = 0; mi < WM; ++mi) acc[ni][mi] = KD::mfma(wf[ni], xf[mi], acc[ni][mi]);
            }
        }
    }

    // ---- epilogue
    if (vtile) {
        // acc[ni][mi][j] = D[m = mrow + j][n = ncol]; V^T[seg][n - n_split][t .. t+3]
#pragma unroll
        for (int ni = 0; ni < WN; ++ni) {
            const int n = n0 + wc * (WN * 16) + ni * 16 + fr;
            const float bv = (a.bias && n < a.N) ? a.bias[n] : 0.f;
#pragma unroll
            for (int mi = 0; mi < WM; ++mi) {
                const int m = m0 + wr * (WM * 16) + mi * 16 + fg * 4;
                if (m < a.M && n < a.N) {
                    const int seg = m / a.seg_T, t = m - seg * a.seg_T;
                    O4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = (OT)gemm_lin<KD, EPI != EPI_BIAS_GELU>(a, acc[ni][mi][j], m + j, n, bv, I8Row{0.f, 0, 0, false}, 0.f);   // (16-bit kinds only)
                    *(O4*)((OT*)a.Vt + (long)seg * a.vt_seg_stride + (long)(n - a.n_split) * a.vt_ld + t) = o;
                }
            }
        }
        return;
    }
    if (EPI == EPI_SWIGLU && a.gu8) {
        // gate / up in 8-row groups (GemmArgs.gu8): lanes fg < 2 hold four gate columns of a 16-row tile, lanes fg >= 2 their up partners
        // (v_permlane32_swap: the lower half finishes columns 2, 3 of its group of four, the upper half columns 0, 1 - see gemm256.hip)
        typedef typename ET<OT>::v2 O2;
#pragma unroll
        for (int ni = 0; ni < WN; ++ni) {
            const int oc = ((n0 + wc * (WN * 16) + ni * 16) >> 1) + (fg & 1) * 4 + (fg < 2 ? 2 : 0);
#pragma unroll
            for (int mi = 0; mi < WM; ++mi) {
                const int m = m0 + wr * (WM * 16) + mi * 16 + fr;
                const f32x4 v = {(float)acc[ni][mi][0], (float)acc[ni][mi][1], (float)acc[ni][mi][2], (float)acc[ni][mi][3]};
                const auto s0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[2]), __float_as_uint(v[0]), false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[3]), __float_as_uint(v[1]), false, false);
                if (m < a.M && (n0 + wc * (WN * 16) + ni * 16) < a.N) {
                    O2 o;
                    o[0] = (OT)(rT<OT>(silu_f(rT<OT>(__uint_as_float(s0[0])))) * rT<OT>(__uint_as_float(s0[1])));
                    o[1] = (OT)(rT<OT>(silu_f(rT<OT>(__uint_as_float(s1[0])))) * rT<OT>(__uint_as_float(s1[1])));
                    *(O2*)(C + (long)m * a.ldc + oc) = o;
                }
            }
        }
        return;
    }
    if (EPI == EPI_SWIGLU) {
#pragma unroll
        for (int q = 0; q < WN / 2; ++q) {
            const int oc = ((n0 + wc * (WN * 16)) >> 1) + q * 16 + fg * 4;
            const int ng = n0 + wc * (WN * 16) + q * 32 + fg * 4;    // gate columns ng .. ng+3, up columns ng+16 ..
            f32x4 sbg = {0.f, 0.f, 0.f, 0.f}, sbu = {0.f, 0.f, 0.f, 0.f};
            if constexpr (KD::I8) if (ng + 19 < a.N) { sbg = *(const f32x4*)(a.q.scb + ng); sbu = *(const f32x4*)(a.q.scb + ng + 16); }
#pragma unroll
            for (int mi = 0; mi < WM; ++mi) {
                const int m = m0 + wr * (WM * 16) + mi * 16 + fr;
                if (m < a.M && (n0 + wc * (WN * 16) + q * 32) < a.N) {
                    const I8Row rw = i8_row<KD>(a, m);
                    O4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float g = gemm_lin<KD, EPI != EPI_BIAS_GELU>(a, acc[2 * q][mi][j], m, ng + j, 0.f, rw, sbg[j]), u = gemm_lin<KD, EPI != EPI_BIAS_GELU>(a, acc[2 * q + 1][mi][j], m, ng + 16 + j, 0.f, rw, sbu[j]);
                        o[j] = (OT)(rT<OT>(silu_f(g)) * u);
                    }
                    *(O4*)(C + (long)m * a.ldc + oc) = o;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int ni = 0; ni < WN; ++ni) {
        const int n = n0 + wc * (WN * 16) + ni * 16 + fg * 4;
        if (n >= a.N) continue;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.bias) {
            const f32x4 b4 = *(const f32x4*)(a.bias + n);
            bv[0] = b4[0]; bv[1] = b4[1]; bv[2] = b4[2]; bv[3] = b4[3];
        }
        f32x4 sb = {0.f, 0.f, 0.f, 0.f};
        if constexpr (KD::I8) sb = *(const f32x4*)(a.q.scb + n);
#pragma unroll
        for (int mi = 0; mi < WM; ++mi) {
            const int m = m0 + wr * (WM * 16) + mi * 16 + fr;
            if (m >= a.M) continue;
            const I8Row rw = i8_row<KD>(a, m);
            O4 o;
            float l[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) l[j] = gemm_lin<KD, EPI != EPI_BIAS_GELU>(a, acc[ni][mi][j], m, n + j, bv[j], rw, sb[j]);
            if (EPI == EPI_BIAS_RESID) {
                if (rw.defer) {                                   // finished by launch_i8_outlier_side (outlier sum, then the residual)
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = (OT)l[j];
                    *(O4*)((OT*)a.q.defer_out + (long)blockIdx.z * a.strideC + (long)m * a.ldc + n) = o;
                    continue;
                }
                const O4 rv = *(const O4*)(R + (long)m * a.ldr + n);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (OT)(l[j] + (float)rv[j]);
            } else if (EPI == EPI_BIAS_GELU) {
                if (std::is_same<KD, KBF16>::value && a.gelu_lut) {      // the same table as the 256x256 kernel, read from global memory
                    unsigned t[4]; int idx[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { idx[j] = gelu_lut_index(l[j]); t[j] = a.gelu_lut[gelu_lut_slot(l[j], idx[j])]; }
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = (OT)gelu_lut_value(l[j], idx[j], t[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = (OT)gelu_erf(l[j]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = (OT)l[j];
            }
            *(O4*)(C + (long)m * a.ldc + n) = o;
        }
    }
}

bool gemm256_eligible(const GemmArgs& a, int epi);
void launch_gemm256(const GemmArgs& a, int epi, hipStream_t s);
void launch_gemm256p(const GemmArgs& a, int epi, int cus, hipStream_t s);
thread_local LaunchOpts g_opts;

static void launch_gemm128(const GemmArgs& a, int epi, int shape, hipStream_t s);
static int device_cus() {
    static int n = 0;
    if (!n) { int dev = 0; hipDeviceProp_t p; n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256; }
    return n;
}
// the 256x256 tile: persistent kernel for the 16-bit kinds (gemm256p.hip), one launch per tile round otherwise (int8 kinds, batched conv stem)
static void launch_tile256(const GemmArgs& a, int epi, hipStream_t s) {
#ifdef SONIC_AB      // the persistent form lost every A/B: it ships only in `make SONIC_AB=1` builds
    if (!a.q.sca && a.batch <= 1 && g_opts.gemm256_persist) { launch_gemm256p(a, epi, (g_opts.gemm256_persist_cus < device_cus() ? g_opts.gemm256_persist_cus : device_cus()), s); return; }
#endif
    launch_gemm256(a, epi, s);
}
// A 256x256 tile owns a CU, so a grid of fewer tiles than CUs leaves the rest of the chip idle for the whole GEMM (one 5 s request through
// the encoder: 30 .. 120 tiles per linear on 256 CUs).  The 128x128 kernel cuts the same problem into four times as many tiles, two to a CU,
// at about `gemm_small_eff` % of the big kernel's per-CU rate when both are full: it gets the GEMM whenever its tile rounds, priced that way,
// are fewer.  Both kernels produce the same bits (tests/test_gpu_parity.py test_gemm256_path), so the choice never shows in a result.  Not the
// q|k|v epilogue: its fused RoPE exists only on the 256x256 tile (it rotates the rounded linear with the separate pass's operations - the same bits,
// tests/test_gpu_gemm_forms.py - but the 128x128 kernel would need that pass back).
static bool small_grid_prefers128(const GemmArgs& a, int epi, long cus) {
    const int eff = g_opts.gemm_small_eff;
    if (eff <= 0 || epi == EPI_QKV_VT) return false;
    const long batch = a.batch > 0 ? a.batch : 1;
    const long t256 = (long)((a.M + 255) / 256) * ((a.N + 255) / 256) * batch, t128 = (long)((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN) * batch;
    const long r256 = (t256 + cus - 1) / cus, r128 = (t128 + 2 * cus - 1) / (2 * cus);
    return r128 * 50 < r256 * eff;      // a round of 128x128 tiles is half the work per CU of a round of 256x256 tiles
}
// shape of a 128x128-kernel launch over M rows: 0 = 128 x 128 tiles, two-stage ring, two blocks per CU; 1 = 32 x 64 tiles, four-stage ring (grids of 128 x 128 tiles
// that would leave half of the CUs idle); 2 = 32 x 32 tiles (when even the 32 x 64 grid covers at most half of the CUs; not for the SwiGLU epilogue, whose gate / up
// pairs need 32 columns per wave: it stays at 1).  The q|k|v epilogue exists at shape 0 only.
static int gemm128_shape(const GemmArgs& a, int M, int epi, int cus) {
    if (epi == EPI_QKV_VT) return 0;
    const int tilesM = (M + BM - 1) / BM, tilesN = (a.N + BN - 1) / BN;
    const int batch = a.batch > 0 ? a.batch : 1;
    int shape = (!g_opts.gemm128_shallow && (long)tilesM * tilesN * batch <= cus / 2 && a.K / (128 / (a.q.sca ? 1 : 2)) >= 4) ? 1 : 0;
    if (shape == 1 && epi != EPI_SWIGLU && (long)((M + 31) / 32) * ((a.N + 63) / 64) * batch <= cus / 2) shape = 2;
    return shape;
}
// The whole routing decision of one GEMM, in one place: launch_gemm launches from it and nothing else decides (the route witness of the tests reads the same record).
GemmPlan gemm_plan(const GemmArgs& a, int epi) {
    GemmPlan p{0, a.M, 0, device_cus()};
    if (!g_opts.gemm_force128 && gemm256_eligible(a, epi) && !small_grid_prefers128(a, epi, p.cus)) {
        p.rows256 = a.M; p.rows128 = 0;
        // Wave quantisation: a 256x256 tile occupies a whole CU, so (tiles mod CUs) small means a nearly empty extra round (prefill at
        // M = 8320: 33 x 8 = 264 tiles on 256 CUs, two rounds for 1.03).  If cutting the ragged last <= 128 rows off saves a round, those
        // rows go to the 128x128 kernel instead (same math per row; rows are independent in every epilogue but QKV+V^T).
        const int cus = p.cus, ntn = (a.N + 255) / 256, Mm = (a.M / 256) * 256, tail = a.M - Mm;
        if (tail > 0 && tail <= 128 && Mm >= 512 && epi != EPI_QKV_VT && a.batch <= 1) {
            const long full = (long)((a.M + 255) / 256) * ntn, main_tiles = (long)(Mm / 256) * ntn;
            if ((main_tiles + cus - 1) / cus < (full + cus - 1) / cus) { p.rows256 = Mm; p.rows128 = tail; }
        }
    }
    if (p.rows128 > 0) p.shape128 = gemm128_shape(a, p.rows128, epi, p.cus);
    return p;
}
thread_local GemmPlan g_last_gemm_plan{0, 0, 0, 0};
void launch_gemm(const GemmArgs& a, int epi, hipStream_t s) {
    if (a.q.sca && a.w_tiled && epi == EPI_BIAS_GELU) {
        // gemm_lin<KD, false> compiles the tiled outlier gather out of the GELU epilogue (int8_util.h): such a launch would add outlier columns read at row-major
        // addresses of a tiled copy.  No caller has one (the decoder's tiled linears use SwiGLU); one that appears must not get wrong numbers quietly
        fprintf(stderr, "[sonic_hip] launch_gemm: int8 EPI_BIAS_GELU from a fragment-tiled W is not compiled (gemm_lin WK); give the GELU linear the row-major codes\n");
        abort();
    }
    const GemmPlan p = gemm_plan(a, epi);
    g_last_gemm_plan = p;
    if (p.rows256 > 0 && p.rows128 > 0) {          // the ragged-tail split: rows [0, rows256) on the big tile, the rest on the 128x128 kernel
        const int Mm = p.rows256;
        GemmArgs m = a; m.M = Mm;
        launch_tile256(m, epi, s);
        GemmArgs t = a; t.M = p.rows128; t.C = a.C + (long)Mm * a.ldc;
        if (a.R) t.R = a.R + (long)Mm * a.ldr;
        if (a.q.sca) {
            // int8 GEMM: A is int8 (1 byte per element) and the per-row quantisation data travels with the rows - scales,
            // unquantised activations of the outlier columns, and the row -> group (request) index.  (Leaving them at row 0
            // gave the tail rows the scales and outlier lists of the FIRST rows of the batch: the last request of some batch
            // compositions differed from its solo result, found by tools/find_batch_dependence.py.)
            t.A = (const bf16_t*)((const int8_t*)a.A + (long)Mm * a.lda);
            t.q.sca = a.q.sca + Mm; t.q.x16 = a.q.x16 + (long)Mm * a.q.ldx16; t.q.row_off = a.q.row_off + Mm;
            if (a.q.defer_out) t.q.defer_out = a.q.defer_out + (long)Mm * a.ldc;
        } else {
            t.A = a.A + (long)Mm * a.lda;
        }
        launch_gemm128(t, epi, p.shape128, s);
        return;
    }
    if (p.rows256 > 0) launch_tile256(a, epi, s);
    else launch_gemm128(a, epi, p.shape128, s);
}
template <typename KD, int EPI, int NS, int WM, int WN> static void launch_gemm128_v(const GemmArgs& a, hipStream_t s) {
    constexpr int TBM = 32 * WM, TBN = 32 * WN;
    const size_t lds = (size_t)NS * (TBM + TBN) * BK * 2;
    if (lds > 65536) ensure_dyn_lds((const void*)gemm_kernel<KD, EPI, NS, WM, WN>, (int)lds);
    const int tilesM = (a.M + TBM - 1) / TBM, tilesN = (a.N + TBN - 1) / TBN;
    hipLaunchKernelGGL((gemm_kernel<KD, EPI, NS, WM, WN>), dim3(tilesM * tilesN, 1, a.batch > 0 ? a.batch : 1), dim3(256), lds, s, a);
}
// shape of the launch: gemm128_shape
template <typename KD, int EPI> static void launch_gemm128_e(const GemmArgs& a, int shape, hipStream_t s) {
    if constexpr (EPI == EPI_QKV_VT) launch_gemm128_v<KD, EPI, 2, 4, 4>(a, s);
    else if (shape == 2 && EPI != EPI_SWIGLU) launch_gemm128_v<KD, EPI, 4, 1, EPI == EPI_SWIGLU ? 2 : 1>(a, s);
    else if (shape >= 1) launch_gemm128_v<KD, EPI, 4, 1, 2>(a, s);
    else launch_gemm128_v<KD, EPI, 2, 4, 4>(a, s);
}
static void launch_gemm128(const GemmArgs& a, int epi, int shape, hipStream_t s) {
    KD_SWITCH(a, KD, {
        switch (epi) {
            case EPI_BIAS: launch_gemm128_e<KD, EPI_BIAS>(a, shape, s); break;
            case EPI_BIAS_GELU: launch_gemm128_e<KD, EPI_BIAS_GELU>(a, shape, s); break;
            case EPI_BIAS_RESID: launch_gemm128_e<KD, EPI_BIAS_RESID>(a, shape, s); break;
            case EPI_SWIGLU: launch_gemm128_e<KD, EPI_SWIGLU>(a, shape, s); break;
            case EPI_QKV_VT: if constexpr (!KD::I8) launch_gemm128_e<KD, EPI_QKV_VT>(a, shape, s); break;
        }
    });
}
