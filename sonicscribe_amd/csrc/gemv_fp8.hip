// gemv_fp8.hip: mode fp8 (options fp8_weights / fp8_chain) - the snap of the decoder's matrices onto an e4m3 grid, and the 1 - 4 row token step
// streaming the e4m3 copies: half the weight bytes of the bf16 GEMV chain (gemv.hip), the same bits.
//
// The model.  Every output row n of a packed decoder matrix W[N][K] gets a power-of-two scale s_n (fp8_codec.h: the smallest with amax_n / s_n <= 448), its codes are
// q = RNE_e4m3fn(W / s_n) and the snapped row is W' = s_n q - exact in bf16 (three mantissa bits, a power-of-two scale).  fp8_snap_kernel overwrites the bf16 tiles
// with W' in place, so every kernel that reads them (prefill GEMMs, the MFMA decode chain, scoring, alignment, verification, the bf16 GEMV chain) computes the model
// W', and writes the codes beside them, one byte per weight.
//
// The chain.  gemv_fp8_kernel is gemv_kernel<bf16_t, ...> with another weight operand: the same block / wave / lane ownership of (tile, k), the same staging and
// RMSNorm of the activation rows, the same fdot2 sequence per lane (u ascending, the four e pairs ascending), the same two shfl_xor steps and the same reduction
// over the eight waves in order.  Its fdot2 weight inputs are the codes' values q as bf16 (v_cvt_scalef32_pk_bf16_fp8 at scale 1: exact), NOT s_n q:
//   POST-ACCUMULATION SCALING - a lane's accumulators belong to ONE output row each, and the lane multiplies them by s_n once, behind its k loop and ahead of the
//   shfl_xor steps.  s_n is a power of two, so every partial sum of the unscaled sequence is the scaled sequence's partial sum divided by s_n exactly, rounding
//   included, short of fp32 underflow / overflow (|q| <= 448 and K <= 6144 keep the unscaled sums below 2^22 times the activations' magnitude; s_n >= 2^-117):
//   the outputs are bit-identical to gemv_kernel on the snapped bf16 tiles.  tests/test_gpu_fp8.py holds it to that, without a tolerance.
// The e4m3 tiling is defined in tile_weights.hip's comments beside the others: a lane's 16-byte piece holds its 8 k of two consecutive k-steps.
#include "common.h"
#include "kernels.h"
#include "fp8_codec.h"

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// ------------------------------------------------------------------------------------------ the snap (option time; one block per output row, not tuned)
// wt: a fragment-tiled bf16 matrix [N][K] (either row interleave: a row of the TILED copy is a row of the matrix, whichever it is), K % 64 == 0.
// Row n = (tile t, i): its piece pc (k = 8 pc .. 8 pc + 7) lies at ((t (K/32) + pc/4) 512 + ((pc%4) 16 + i) 8; its eight codes go where the e4m3 tiling puts them (tile_weights.hip)
__global__ __launch_bounds__(256) void fp8_snap_kernel(bf16_t* wt, unsigned char* w8, float* scales, bf16_t* rowmajor, int N, int K) {
    __shared__ float red[256];
    const int n = blockIdx.x, t = n >> 4, i = n & 15, tid = threadIdx.x;
    bf16_t* row = wt + (long)t * (K >> 5) * 512 + i * 8;
    float amax = 0.f;
    for (int pc = tid; pc < (K >> 3); pc += 256) {
        const bf16x8 v = *(const bf16x8*)(row + (long)(pc >> 2) * 512 + (pc & 3) * 128);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf((float)v[e]));
    }
    red[tid] = amax;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]); __syncthreads(); }
    const int ex = fp8_scale_exp(red[0]);
    const float s = fp8_pow2(ex), inv = fp8_pow2(-ex);       // W / s = W * 2^-ex: exact
    if (tid == 0) scales[n] = s;
    for (int pc = tid; pc < (K >> 3); pc += 256) {
        bf16_t* p = row + (long)(pc >> 2) * 512 + (pc & 3) * 128;
        const bf16x8 v = *(const bf16x8*)p;
        bf16x8 o; u32x2 c; c[0] = 0; c[1] = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const unsigned code = fp8_encode((float)v[e] * inv);
            c[e >> 2] |= code << (8 * (e & 3));
            o[e] = (bf16_t)(s * fp8_decode(code));            // exact: 4 significant bits times a power of two
        }
        *(bf16x8*)p = o;
        const int u = pc >> 2, kc = pc & 3;
        *(u32x2*)(w8 + (((long)t * (K >> 6) + (u >> 1)) * 64 + kc * 16 + i) * 16 + (u & 1) * 8) = c;
        if (rowmajor) *(bf16x8*)(rowmajor + (long)n * K + pc * 8) = o;      // the token lookup's row-major embedding: the same W' (plain tiling: tiled row n = row n)
    }
}
void launch_fp8_snap(bf16_t* wt, unsigned char* w8, float* scales, bf16_t* rowmajor, int N, int K, hipStream_t s) {
    hipLaunchKernelGGL(fp8_snap_kernel, dim3(N), dim3(256), 0, s, wt, w8, scales, rowmajor, N, K);
}
// debug read-back: the first `count` elements of the e4m3 copy as fp32 s q, row-major in the tiled copy's row order
__global__ void fp8_read_kernel(const unsigned char* w8, const float* scales, float* out, int K, long count) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= count) return;
    const int n = (int)(idx / K), k = (int)(idx % K), t = n >> 4, i = n & 15, u = k >> 5, kc = (k & 31) >> 3;
    const unsigned code = w8[(((long)t * (K >> 6) + (u >> 1)) * 64 + kc * 16 + i) * 16 + (u & 1) * 8 + (k & 7)];
    out[idx] = scales[n] * fp8_decode(code);
}
void launch_fp8_read(const unsigned char* w8, const float* scales, float* out, int K, long count, hipStream_t s) {
    if (count > 0) hipLaunchKernelGGL(fp8_read_kernel, dim3((count + 255) / 256), dim3(256), 0, s, w8, scales, out, K, count);
}

// ------------------------------------------------------------------------------------------ the chain
// two e4m3 codes (the low or the high half of a 32-bit word) as two bf16, unscaled: exact
static __device__ __forceinline__ bf16x2 cvt2(unsigned w, bool hi) {
    return hi ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false);
}

template <int MODE, int TPB, int KS8>
__global__ __launch_bounds__(512) void gemv_fp8_kernel(GemvFp8Args a8) {
    typedef bf16_t T;
    typedef bf16x8 V8;
    static_assert(KS8 % 2 == 0, "a lane's e4m3 piece holds two consecutive k-steps of one wave");
    const GemvArgs& a = a8.g;
    constexpr int K = KS8 * 256, KE = K / 8, RMAX = GEMV_MAX_ROWS, KP = KS8 / 2;      // KE: elements of a wave's K eighth; KP: its k-step pairs
    constexpr bool NORM = MODE != GEMV_RESID;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs = (T*)smem;                                                     // [R][K] activation rows (NORM: normalised)
    float* red = (float*)(smem + (size_t)RMAX * K * sizeof(T));           // [8][TPB][RMAX][16]
    __shared__ float part[RMAX][8];
    const int tid = threadIdx.x, lane = tid & 63, wk = tid >> 6, R = a.M;
    const u32x4* W = (const u32x4*)a8.W8 + ((long)blockIdx.x * TPB * (K >> 6) + wk * KP) * 64 + lane;
    // weights first: the whole K eighth of every tile of the block in flight at once - half the registers of the bf16 chain's wf
    u32x4 wf[TPB][KP];
#pragma unroll
    for (int j = 0; j < TPB; ++j)
#pragma unroll
        for (int p = 0; p < KP; ++p) wf[j][p] = __builtin_nontemporal_load(W + ((long)j * (K >> 6) + p) * 64);
    float sc[TPB];                                                        // this lane's output row of every tile: its scale
#pragma unroll
    for (int j = 0; j < TPB; ++j) sc[j] = a8.scales[((long)blockIdx.x * TPB + j) * 16 + (lane & 15)];
    // this wave's slice of the activation rows: KE / 8 16-byte pieces per row
    constexpr int PPR = KE / 8, NP = (RMAX * PPR + 63) / 64;
    V8 xv[NP];
    float ss[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) ss[r] = 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int i = p * 64 + lane, row = i / PPR, c = i % PPR;
        if (row < R) {
            xv[p] = *(const V8*)((const T*)a.X + (long)row * a.ldx + wk * KE + c * 8);
            if (NORM) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float f = (float)xv[p][e]; s += f * f; }
#pragma unroll
                for (int r = 0; r < RMAX; ++r) if (r == row) ss[r] += s;
            }
        }
    }
    if (NORM) {
        // row sums of squares: lanes -> wave -> the eight waves' partials in wave order; then w * T(x * rstd) on the staged pieces (modeling_llama.py:60-65)
#pragma unroll
        for (int r = 0; r < RMAX; ++r) { const float t = wave_sum(ss[r]); if (lane == 0) part[r][wk] = t; }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int i = p * 64 + lane, row = i / PPR, c = i % PPR;
            if (row < R) {
                float tot = 0.f;
#pragma unroll
                for (int w8 = 0; w8 < 8; ++w8) tot += part[row][w8];
                const float rs = 1.0f / sqrtf(tot / (float)K + a.eps);
                const float* nw = a.norm_w + wk * KE + c * 8;
                const f32x4 w0 = *(const f32x4*)nw, w1 = *(const f32x4*)(nw + 4);
                V8 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) { o[e] = (T)(w0[e] * rT<T>((float)xv[p][e] * rs)); o[4 + e] = (T)(w1[e] * rT<T>((float)xv[p][4 + e] * rs)); }
                xv[p] = o;
            }
        }
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int i = p * 64 + lane, row = i / PPR, c = i % PPR;
        if (row < R) *(V8*)(xs + (long)row * K + wk * KE + c * 8) = xv[p];
    }
    // (a wave multiplies only the k-steps of its own eighth, i.e. only what it staged itself: no barrier, as in gemv_kernel)
    float acc[TPB][RMAX];
#pragma unroll
    for (int j = 0; j < TPB; ++j)
#pragma unroll
        for (int r = 0; r < RMAX; ++r) acc[j][r] = 0.f;
    const int kc = lane >> 4;                                              // this lane's 8 k of a 32-deep step
#pragma unroll
    for (int u = 0; u < KS8; ++u) {
        // k-step u of every tile: words (u & 1) * 2 and + 1 of the pair's piece -> the four bf16 pairs, e ascending
        bf16x2 wq[TPB][4];
#pragma unroll
        for (int j = 0; j < TPB; ++j) {
            const unsigned w0 = wf[j][u >> 1][(u & 1) * 2], w1 = wf[j][u >> 1][(u & 1) * 2 + 1];
            wq[j][0] = cvt2(w0, false); wq[j][1] = cvt2(w0, true); wq[j][2] = cvt2(w1, false); wq[j][3] = cvt2(w1, true);
        }
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            if (r < R) {
                const V8 xr = *(const V8*)(xs + (long)r * K + wk * KE + u * 32 + kc * 8);
#pragma unroll
                for (int j = 0; j < TPB; ++j) {
                    float s = acc[j][r];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        bf16x2 xa;
                        xa[0] = xr[2 * e]; xa[1] = xr[2 * e + 1];
                        s = __builtin_amdgcn_fdot2_f32_bf16(wq[j][e], xa, s, false);
                    }
                    acc[j][r] = s;
                }
            }
        }
    }
    // the lane's row scale (exact: a power of two), then the four lanes of an output row (k chunks 0 .. 3), then the eight waves, in fixed order
#pragma unroll
    for (int j = 0; j < TPB; ++j)
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            float s = acc[j][r] * sc[j];
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (lane < 16 && r < R) red[((wk * TPB + j) * RMAX + r) * 16 + lane] = s;
        }
    __syncthreads();
    // one thread per output: (tile j, row r, column n of the tile)
    for (int o = tid; o < TPB * RMAX * 16; o += 512) {
        const int j = o / (RMAX * 16), r = (o / 16) % RMAX, n = o % 16;
        if (r >= R) continue;
        float s = 0.f;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) s += red[((w8 * TPB + j) * RMAX + r) * 16 + n];
        const long col = ((long)blockIdx.x * TPB + j) * 16 + n;
        if (MODE == GEMV_SLAB_NORM) a.P[(long)r * a.N + col] = s;
        else if (MODE == GEMV_RESID) {
            T* xp = (T*)a.resid + (long)r * a.ldr + col;
            *xp = (T)((float)*xp + rT<T>(s));
        } else if (n < 8) {
            // gate column n of the tile and its up partner n + 8 (8-row interleave of launch_tile_weights_gu8): read the partner's eight partials as well
            float up = 0.f;
#pragma unroll
            for (int w8 = 0; w8 < 8; ++w8) up += red[((w8 * TPB + j) * RMAX + r) * 16 + n + 8];
            ((T*)a.act)[(long)r * (a.N / 2) + ((long)blockIdx.x * TPB + j) * 8 + n] = (T)(rT<T>(silu_f(rT<T>(s))) * rT<T>(up));
        }
    }
}

template <int MODE, int TPB, int KS8> static void launch_gemv_fp8_v(const GemvFp8Args& a, hipStream_t s) {
    const size_t lds = (size_t)GEMV_MAX_ROWS * KS8 * 256 * sizeof(bf16_t) + (size_t)8 * TPB * GEMV_MAX_ROWS * 16 * 4;
    if (lds > 65536) ensure_dyn_lds((const void*)gemv_fp8_kernel<MODE, TPB, KS8>, (int)lds);
    hipLaunchKernelGGL((gemv_fp8_kernel<MODE, TPB, KS8>), dim3(a.g.N / (16 * TPB)), dim3(512), lds, s, a);
}
// gemv_eligible, and an even number of k-steps per wave (K % 512 == 0: a lane's e4m3 piece is two k-steps of ONE wave): K in {512, 1024, 2048} for every mode,
// K in {1536, 3072, 6144} for the down projection.  bf16 only
bool gemv_fp8_eligible(int M, int N, int K, int mode) { return gemv_eligible(M, N, K, mode) && K % 512 == 0; }
// tiles per block as launch_gemv picks them (one block per CU where the tile count allows): the e4m3 fragments would leave registers for more, but a block's
// tiles are already all the weight bytes it has in flight, and more tiles per block means fewer blocks than CUs on every shape but the lm_head
template <int MODE> static void launch_gemv_fp8_m(const GemvFp8Args& a, hipStream_t s) {
    const int tiles = a.g.N / 16;
#define GV(KS8) do { if (MODE == GEMV_SWIGLU_NORM && tiles % 3 == 0) launch_gemv_fp8_v<MODE, 3, KS8>(a, s); \
                     else if (tiles % 4 == 0 && tiles / 4 >= 512) launch_gemv_fp8_v<MODE, 4, KS8>(a, s);     /* the lm_head: 3704 tiles -> 926 blocks */ \
                     else if (MODE == GEMV_SWIGLU_NORM && tiles % 2 == 0) launch_gemv_fp8_v<MODE, 2, KS8>(a, s); \
                     else launch_gemv_fp8_v<MODE, 1, KS8>(a, s); } while (0)
    switch (a.g.K) {
        case 512: GV(2); break; case 1024: GV(4); break; case 2048: GV(8); break;
        case 1536: if constexpr (MODE == GEMV_RESID) launch_gemv_fp8_v<MODE, 1, 6>(a, s); break;
        case 3072: if constexpr (MODE == GEMV_RESID) launch_gemv_fp8_v<MODE, 1, 12>(a, s); break;
        case 6144: if constexpr (MODE == GEMV_RESID) launch_gemv_fp8_v<MODE, 1, 24>(a, s); break;
    }
#undef GV
}
void launch_gemv_fp8(const GemvFp8Args& a, int mode, hipStream_t s) {
    if (mode == GEMV_SLAB_NORM) launch_gemv_fp8_m<GEMV_SLAB_NORM>(a, s);
    else if (mode == GEMV_RESID) launch_gemv_fp8_m<GEMV_RESID>(a, s);
    else launch_gemv_fp8_m<GEMV_SWIGLU_NORM>(a, s);
}
