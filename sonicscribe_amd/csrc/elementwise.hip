// Memory-bound glue kernels: LayerNorm / RMSNorm with wavefront
// reductions, rotate-half RoPE (partial-32 encoder, full-128 decoder) fused with the KV-cache append,
// the decode-step consumers of the skinny-GEMM partial slabs, embedding gather, fused argmax + greedy
// controller, synthetic weight generator.  All 16-bit traffic is 16 B per lane (8 elements).
//
// Rounding boundaries reproduce torch's op sequence of the reference path: every torch op output is rounded to the
// activation dtype once, arithmetic inside an op is fp32.  Kernels are templated on that dtype T: bf16 (`mode="native"`) or
// IEEE half (`mode="int8"`, asr.py:61,296).  In int8 mode the decode-step consumers read int32 slabs of a quantised skinny
// GEMM (deq4) and producers that own whole rows also emit them quantised for the next Linear8bitLt (quant_emit_row).
#include "common.h"
#include "kernels.h"

#include "int8_util.h"

// A block that owns one whole row (thread c holds its elements [8c, 8c+8) as fp16 values in y, threads with !active hold nothing)
// emits the row quantised: absmax without the elements >= 6.0, int8 = rn(y * 127 / absmax) (0 for outliers), and the ascending
// list of the outlier positions.  Every thread of the block must call it.  s_f: >= 16 floats, s_i: >= 17 ints of LDS scratch.
// FRESH: nobody has touched s_f / s_i in this kernel before (no barrier needed in front of the first write).
template <bool FRESH = false>
__device__ __forceinline__ void quant_emit_row(const float (&y)[8], bool active, int c, int row, const QuantOut& qo, float* s_f, int* s_i) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = (blockDim.x + 63) >> 6;
    float amax = -1.17549435e-38f;
    int cnt = 0;
    if (active) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float a = fabsf(y[j]); if (a < LLM_INT8_THRESHOLD) amax = fmaxf(amax, a); else ++cnt; }
    }
    amax = wave_max(amax);
    int incl = cnt;                                   // inclusive scan of the outlier counts inside the wave (only where the wave holds any)
    if (__ballot(cnt > 0)) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    }
    if constexpr (!FRESH) __syncthreads();           // scratch may still be in use by the caller
    if (lane == 63) s_i[wid] = incl;
    if (lane == 0) s_f[wid] = amax;
    __syncthreads();
    float bm = s_f[0]; int base = 0, total = 0;
    for (int w = 0; w < nw; ++w) { bm = fmaxf(bm, s_f[w]); if (w < wid) base += s_i[w]; total += s_i[w]; }
    const float scale = 127.0f / bm;
    if (tid == 0) { qo.sca[row] = bm; qo.oc_cnt[row] = total; }
    if (active) {
        int pos = base + incl - cnt;
        int pk[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool out = !(fabsf(y[j]) < LLM_INT8_THRESHOLD);
            int qv = (out || !(bm > 0.f)) ? 0 : (int)rintf(y[j] * scale);
            pk[j >> 2] |= (qv & 0xFF) << ((j & 3) * 8);
            if (out) {
                const long at = (long)row * qo.oc_ld + pos++;
                qo.oc_list[at] = c * 8 + j;
                if (qo.oc_val) qo.oc_val[at] = y[j];
            }
        }
        *(int2*)(qo.q + (long)row * qo.ldq + c * 8) = make_int2(pk[0], pk[1]);
    }
}

// ---------------------------------------------------------------- LayerNorm (modeling_glmasr.py:246-247,305)
// one wave per row, d % 8 == 0, d <= 2048; two-pass in registers (mean, then centred variance).
// qa.q != null (int8 mode, the row feeds a Linear8bitLt): the wave that normalised the row also emits what the first two passes of
// launch_quant_act would compute from it - row absmax without the elements >= 6.0, int8 codes (those elements as 0), and their group flags.
template <typename T, bool Q>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* x, const float* w, const float* b, T* y, int rows, int d, float eps, QuantActArgs qa) {
    typedef typename ET<T>::v8 V8;
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const T* xr = x + (long)row * d;
    const int nv = d >> 3;
    float v[4][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            const V8 t = *(const V8*)(xr + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[i][j] = (float)t[j]; s += v[i][j]; }
        }
    }
    const float mean = wave_sum(s) / d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (lane + i * 64 < nv) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float c = v[i][j] - mean; q += c * c; }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / d + eps);
    float amax = -1.17549435e-38f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            V8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                o[j] = (T)(((v[i][j] - mean) * rstd) * w[c * 8 + j] + b[c * 8 + j]);
                if constexpr (Q) {
                    v[i][j] = (float)o[j];
                    const float av = fabsf(v[i][j]);
                    if (av < LLM_INT8_THRESHOLD) amax = fmaxf(amax, av);
                }
            }
            *(V8*)(y + (long)row * d + c * 8) = o;
        }
    }
    if constexpr (!Q) return;
    amax = wave_max(amax);
    if (lane == 0) qa.sca[row] = amax;
    const int g = qa.gmap ? qa.gmap[row / qa.gdiv] : row / qa.gdiv;
    unsigned char* fl = qa.flags + (long)g * qa.K;
    const float scale = 127.0f / amax;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            int pk[2] = {0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool out = !(fabsf(v[i][j]) < LLM_INT8_THRESHOLD);
                if (out) fl[c * 8 + j] = 1;                       // (benign race: every writer stores the same value)
                const int qv = (out || !(amax > 0.f)) ? 0 : (int)rintf(v[i][j] * scale);
                pk[j >> 2] |= (qv & 0xFF) << ((j & 3) * 8);
            }
            *(int2*)(qa.q + (long)row * qa.K + c * 8) = make_int2(pk[0], pk[1]);
        }
    }
}

// ---------------------------------------------------------------- RMSNorm (modeling_llama.py:60-65)
template <typename T, bool Q>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const T* x, const float* w, T* y, int rows, int d, float eps,
                                                      const int* row_map /* optional gather: y[r] = norm(x[row_map[r]]) */, QuantActArgs qa) {
    typedef typename ET<T>::v8 V8;
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const T* xr = x + (long)(row_map ? row_map[row] : row) * d;
    const int nv = d >> 3;
    float v[4][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            const V8 t = *(const V8*)(xr + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) { v[i][j] = (float)t[j]; s += v[i][j] * v[i][j]; }
        }
    }
    const float r = 1.0f / sqrtf(wave_sum(s) / d + eps);
    T* yr = y + (long)row * d;
    float amax = -1.17549435e-38f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            V8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                o[j] = (T)(w[c * 8 + j] * rT<T>(v[i][j] * r));
                if constexpr (Q) {
                    v[i][j] = (float)o[j];
                    const float av = fabsf(v[i][j]);
                    if (av < LLM_INT8_THRESHOLD) amax = fmaxf(amax, av);
                }
            }
            *(V8*)(yr + c * 8) = o;
        }
    }
    if constexpr (!Q) return;
    // int8 mode, the row feeds a Linear8bitLt: absmax, codes and group flags in the same pass (as layernorm_kernel)
    amax = wave_max(amax);
    if (lane == 0) qa.sca[row] = amax;
    const int g = qa.gmap ? qa.gmap[row / qa.gdiv] : row / qa.gdiv;
    unsigned char* fl = qa.flags + (long)g * qa.K;
    const float scale = 127.0f / amax;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            int pk[2] = {0, 0};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool out = !(fabsf(v[i][j]) < LLM_INT8_THRESHOLD);
                if (out) fl[c * 8 + j] = 1;
                const int qv = (out || !(amax > 0.f)) ? 0 : (int)rintf(v[i][j] * scale);
                pk[j >> 2] |= (qv & 0xFF) << ((j & 3) * 8);
            }
            *(int2*)(qa.q + (long)row * qa.K + c * 8) = make_int2(pk[0], pk[1]);
        }
    }
}

// decode: x[r] = T(x[r] + T(sum_ks P[ks][r][:])); y[r] = rmsnorm(x[r]) (o_proj / down_proj consumer).
// one block of d/8 threads per row (the step has only <= 64 rows: parallelism comes from the row width).
// int8 mode (dq.sca != null): P holds the int32 slabs of the quantised projection; the normalised row is also emitted quantised (qo.q).
template <typename T>
__global__ __launch_bounds__(256) void add_rmsnorm_kernel(T* x, const float* P, int ksplit, int mpad, const float* w, T* y,
                                                          int rows, int d, float eps, DeqInfo dq, QuantOut qo, PrefetchRange pf) {
    typedef typename ET<T>::v8 V8;
    if ((int)blockIdx.x >= rows) {                    // idle-CU prefetch blocks (experiment, option decode_prefetch bit 2): stream the next q|k|v's weights and leave
        prefetch_share(pf, blockIdx.x - rows, gridDim.x - rows);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }
    __shared__ float part[16], qpart[16];             // (qpart / qparti: the re-quantisation's own scratch - no barrier before its first write)
    __shared__ int parti[17], qparti[17];
    __shared__ int s_ok[OUTL_CAP];
    __shared__ float s_ox[OUTL_CAP];
    const int row = blockIdx.x, c = threadIdx.x, lane = c & 63, wid = c >> 6;
    const int nv = d >> 3;
    float v[8];
    float s = 0.f;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    T* xr = x + (long)row * d + (c < nv ? c : 0) * 8;
    // the norm weight is requested FIRST: it is cold every step (8 KiB per layer, read once per token) and used only behind the block's
    // reduction - loaded where it is used, it was a second HBM round trip of the kernel's critical path
    f32x4 nw0 = *(const f32x4*)(w + (c < nv ? c : 0) * 8), nw1 = *(const f32x4*)(w + (c < nv ? c : 0) * 8 + 4);
    const V8 t = *(const V8*)xr;                      // (requested before the slabs: one round trip for both)
    if (dq.sca) {
        // int8: the row's outlier pairs and this thread's slabs are requested together, the pairs go through LDS (int8_util.h)
        const int col[1] = {c < nv ? c * 8 : 0};
        float a[1][8];
        if (dq.dbg & 1) {
            const Slab8<1, 8> sl = slab8_load<1, 8>(dq, P, ksplit, mpad, row, col, d);
            OutlStage os{}; os.n = 0;
            slab8_finish<1, 8>(dq, P, ksplit, mpad, row, col, d, sl, os, s_ok, s_ox, a);
        } else if (dq.scan) {
            // the projection quantised its input on the fly: this block lists the input row's outliers itself (K <= 4 * 8 * blockDim.x)
            // (the producers' per-block counts say whether there is anything to find: usually not, and then the block scan and its barriers
            //  are skipped; the row itself is requested either way, before the verdict is known)
            i32x4 nb4 = {1, 0, 0, 0};
            if (dq.scan_cnt) nb4 = *(const i32x4*)(dq.scan_cnt + row * 4);
            const OutlScan<4> sc = outl_scan_issue<4>(dq, row);
            const Slab8<1, 8> sl = slab8_load<1, 8>(dq, P, ksplit, mpad, row, col, d);
            OutlStage os{}; os.n = 0;
            if ((nb4[0] | nb4[1] | nb4[2] | nb4[3]) != 0) os = outl_scan_commit<4>(dq, row, sc, s_ok, s_ox, parti);     // (block-uniform)
            slab8_finish<1, 8>(dq, P, ksplit, mpad, row, col, d, sl, os, s_ok, s_ox, a);
        } else {
            const OutlStage os = outl_issue(dq, row);
            const Slab8<1, 8> sl = slab8_load<1, 8>(dq, P, ksplit, mpad, row, col, d);
            outl_commit(dq, row, os, s_ok, s_ox);
            slab8_finish<1, 8>(dq, P, ksplit, mpad, row, col, d, sl, os, s_ok, s_ox, a);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = a[0][j];
    }
    if (c < nv) {
        if (!dq.sca) {
            // every slab load is issued before the first add (a rolled ksplit loop costs one L2 round trip per slab); the sum keeps its
            // fixed order ks = 0, 1, ...
            f32x4 a0[8], a1[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const float* p = P + ((long)(ks < ksplit ? ks : 0) * mpad + row) * d + c * 8;
                a0[ks] = *(const f32x4*)p; a1[ks] = *(const f32x4*)(p + 4);
            }
#pragma unroll
            for (int ks = 0; ks < 8; ++ks)
                if (ks < ksplit) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { acc[j] += a0[ks][j]; acc[4 + j] += a1[ks][j]; }
                }
            for (int ks = 8; ks < ksplit; ++ks) {                         // (not reached by the current tilings: ksplit <= 8)
                const float* p = P + ((long)ks * mpad + row) * d + c * 8;
                const f32x4 b0 = *(const f32x4*)p, b1 = *(const f32x4*)(p + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc[j] += b0[j]; acc[4 + j] += b1[j]; }
            }
        }
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) { o[j] = (T)((float)t[j] + rT<T>(acc[j])); v[j] = (float)o[j]; s += v[j] * v[j]; }
        *(V8*)xr = o;
    }
    asm volatile("" : "+v"(nw0), "+v"(nw1));          // (keeps the weight loads above the barrier)
    s = wave_sum(s);
    if (lane == 0) part[wid] = s;
    __syncthreads();
    const int nw = (blockDim.x + 63) >> 6;
    float tot = 0.f;
    for (int i = 0; i < nw; ++i) tot += part[i];
    const float r = 1.0f / sqrtf(tot / d + eps);
    float yo[8];
    if (c < nv) {
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) { o[j] = (T)((j < 4 ? nw0[j & 3] : nw1[j & 3]) * rT<T>(v[j] * r)); yo[j] = (float)o[j]; }
        *(V8*)(y + (long)row * d + c * 8) = o;
    }
    if (qo.q && !(dq.dbg & 2)) quant_emit_row<true>(yo, c < nv, c, row, qo, qpart, qparti);
}

// decode, 33 .. 64 rows: RMSNorm of the residual rows from the fused o_proj kernel's sum-of-squares partials - the arithmetic skinny_gu_kernel<NORM> does while it
// stages X (same association of the partials: lane half h adds groups 16 h .. 16 h + 15 of a 2048-wide row in ascending order, then the halves are
// added; same two roundings per element), once per row instead of once per gate/up block: at 64 rows that normalisation was ~9 us of VALU time on every
// SIMD of 256 CUs.  One block per row, D / 8 threads.  SS: [region = row / 32][D / 64 groups][32 rows][4].
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_ss_kernel(const T* x, const float* SS, const float* w, T* y, int rows, int d, float eps) {
    typedef typename ET<T>::v8 V8;
    __shared__ float s_half[2], s_scale;
    const int row = blockIdx.x, c = threadIdx.x, nv = d >> 3, ng = d >> 6, ssn = ng >> 1;
    V8 t;
    f32x4 w0, w1;
    if (c < nv) { t = *(const V8*)(x + (long)row * d + c * 8); w0 = *(const f32x4*)(w + c * 8); w1 = *(const f32x4*)(w + c * 8 + 4); }
    if (c < 2) {
        const float* sp = SS + ((long)(row >> 5) * ng * 32 + (long)c * ssn * 32 + (row & 31)) * 4;
        float th = 0.f;
        for (int i = 0; i < ssn; ++i) { const f32x4 v = *(const f32x4*)(sp + (long)i * 128); th += v[0]; th += v[1]; th += v[2]; th += v[3]; }
        s_half[c] = th;
    }
    __syncthreads();
    if (c == 0) { const float tt = s_half[0] + s_half[1]; s_scale = 1.0f / sqrtf(tt / (float)d + eps); }
    __syncthreads();
    if (c < nv) {
        const float rr = s_scale;
        V8 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[j] = (T)(w0[j] * rT<T>((float)t[j] * rr)); o[4 + j] = (T)(w1[j] * rT<T>((float)t[4 + j] * rr)); }
        *(V8*)(y + (long)row * d + c * 8) = o;
    }
}
void launch_rmsnorm_ss(const bf16_t* x, const float* SS, const float* w, bf16_t* y, int rows, int d, float eps, hipStream_t s, int dt) {
    DT_SWITCH(dt, T, hipLaunchKernelGGL(rmsnorm_ss_kernel<T>, dim3(rows), dim3(((d >> 3) + 63) / 64 * 64), 0, s, (const T*)x, SS, w, (T*)y, rows, d, eps));
}

// decode: act[r][c] = T(T(silu(T g)) * T u), gate/up rows interleaved in 16-row groups (as EPI_SWIGLU) or, gu8, in 8-row groups (the fused
// gate/up kernel's weight copy, launch_tile_weights_gu8: the one decode copy of the projection since round 5)
template <typename T>
__global__ void swiglu_slab_kernel(const float* P, int ksplit, int mpad, int n2 /* 2*ff */, T* act, int rows, int gu8) {
    typedef typename ET<T>::v4 V4;
    const int ff = n2 >> 1;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;  // one thread per 4 outputs
    if (idx >= (long)rows * (ff >> 2)) return;
    const int row = idx / (ff >> 2), c4 = (idx % (ff >> 2)) * 4;
    const int ng = gu8 ? (c4 >> 3) * 16 + (c4 & 7) : (c4 >> 4) * 32 + (c4 & 15), nu = ng + (gu8 ? 8 : 16);
    f32x4 g = {0.f, 0.f, 0.f, 0.f}, u = {0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < ksplit; ++ks) {
        const float* p = P + ((long)ks * mpad + row) * n2;
        g += *(const f32x4*)(p + ng);
        u += *(const f32x4*)(p + nu);
    }
    V4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (T)(rT<T>(silu_f(rT<T>(g[j]))) * rT<T>(u[j]));
    *(V4*)(act + (long)row * ff + c4) = o;
}

// int8 decode: one block (1024 threads) per row; slabs hold the int32 products of the quantised gate and up projections, weight rows
// interleaved in 16-row groups like the prefill GEMM's SwiGLU layout (one int8 copy serves both).  act = fp16(fp16(silu(g)) * u) and,
// in the same pass, the row quantised for down_proj's Linear8bitLt.  ff <= 8192.
__global__ __launch_bounds__(1024) void swiglu_quant_kernel(const float* P, int ksplit, int mpad, int ff, f16_t* act, DeqInfo dq, QuantOut qo) {
    __shared__ float part[16];
    __shared__ int parti[17];
    __shared__ int s_ok[OUTL_CAP];
    __shared__ float s_ox[OUTL_CAP];
    const int row = blockIdx.x, c = threadIdx.x;
    const bool active = c * 8 < ff;
    // act columns [8c, 8c + 8) = gate columns [base, base + 8) and up columns [base + 16, base + 24) of the interleaved projection
    const int base = active ? (c >> 1) * 32 + (c & 1) * 8 : 0;
    const int col[2] = {base, base + 16};
    const OutlStage os = outl_issue(dq, row);
    const Slab8<2, 2> sl = slab8_load<2, 2>(dq, P, ksplit, mpad, row, col, 2 * ff);
    outl_commit(dq, row, os, s_ok, s_ox);
    float gu[2][8];
    slab8_finish<2, 2>(dq, P, ksplit, mpad, row, col, 2 * ff, sl, os, s_ok, s_ox, gu);
    float y[8];
    if (active) {
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) { o[j] = (f16_t)(rT<f16_t>(silu_f(gu[0][j])) * gu[1][j]); y[j] = (float)o[j]; }
        *(f16x8*)(act + (long)row * ff + c * 8) = o;
    }
    quant_emit_row<true>(y, active, c, row, qo, part, parti);
}

// decode flavour of the activation quantiser: one block per row of an fp16 matrix (K <= 8192)
__global__ __launch_bounds__(1024) void quant_rows_kernel(const f16_t* X, long ld, int K, QuantOut qo) {
    __shared__ float part[16];
    __shared__ int parti[17];
    const int row = blockIdx.x, c = threadIdx.x;
    const bool active = c * 8 < K;
    float y[8];
    if (active) {
        const f16x8 t = *(const f16x8*)(X + (long)row * ld + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = (float)t[j];
    }
    quant_emit_row<true>(y, active, c, row, qo, part, parti);
}

// ---------------------------------------------------------------- encoder RoPE (modeling_glmasr.py:153-168)
// in place on the fused q|k buffer [M][ld]; first `rd` dims of each 64-dim head, pairs (i, i + rd/2);
// cs table [T][rd] = cos[0..rd/2) | sin[0..rd/2) (T-rounded fp32).  one thread = 8 pairs.
template <typename T>
__global__ void rope_enc_kernel(T* qk, long ld, int M, int Tn, int heads2 /* q heads + k heads */, int hd, int rd, const float* cs) {
    typedef typename ET<T>::v8 V8;
    const int half = rd >> 1, per_head = half >> 3;  // threads per head
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)M * heads2 * per_head) return;
    const int u = idx % per_head, hh = (idx / per_head) % heads2;
    const int m = idx / ((long)per_head * heads2), t = m % Tn;
    T* p = qk + (long)m * ld + hh * hd + u * 8;
    const V8 a = *(const V8*)p, bb = *(const V8*)(p + half);
    const float* c = cs + (long)t * rd + u * 8;
    const float* s = c + half;
    V8 o1, o2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float x1 = (float)a[j], x2 = (float)bb[j];
        o1[j] = (T)(rT<T>(x1 * c[j]) + rT<T>(-x2 * s[j]));
        o2[j] = (T)(rT<T>(x2 * c[j]) + rT<T>(x1 * s[j]));
    }
    *(V8*)p = o1;
    *(V8*)(p + half) = o2;
}

// ---------------------------------------------------------------- decoder RoPE + KV append (modeling_llama.py:121-143,261-262)
// Source is either the 16-bit QKV matrix of the prefill GEMM or the fp32 slabs of the decode skinny GEMM.
// Writes roped q ([tok][Hq*128]), roped k -> K cache, v -> V cache, and (prefill) v^T -> Vt scratch.
template <typename T, bool SLAB>
__global__ __launch_bounds__(256) void rope_append_kernel(RopeAppendArgs a) {
    typedef typename ET<T>::v8 V8;
    constexpr int HD = 128, HALF = 64;
    const int tok = blockIdx.x;
    const int heads = a.Hq + 2 * a.Hkv;
    const int N = heads * HD;
    const int b = a.tok_seq[tok], pos = a.tok_pos[tok];
    for (int w = threadIdx.x; w < heads * 8; w += blockDim.x) {
        const int hh = w >> 3, u = w & 7;   // head, 8-wide chunk of the first half
        float x1[8], x2[8];
        if (SLAB) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { x1[j] = 0.f; x2[j] = 0.f; }
            for (int ks = 0; ks < a.ksplit; ++ks) {
                const float* p = a.P + ((long)ks * a.mpad + tok) * N + hh * HD + u * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) { x1[j] += p[j]; x2[j] += p[HALF + j]; }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { x1[j] = rT<T>(x1[j]); x2[j] = rT<T>(x2[j]); }
        } else {
            const T* p = (const T*)a.qkv + (long)tok * a.ld + hh * HD + u * 8;
            const V8 t1 = *(const V8*)p, t2 = *(const V8*)(p + HALF);
#pragma unroll
            for (int j = 0; j < 8; ++j) { x1[j] = (float)t1[j]; x2[j] = (float)t2[j]; }
        }
        V8 o1, o2;
        if (hh < a.Hq + a.Hkv) {
            const float* c = a.cs + (long)pos * HD + u * 8;
            const float* s = c + HALF;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                o1[j] = (T)(rT<T>(x1[j] * c[j]) + rT<T>(-x2[j] * s[j]));
                o2[j] = (T)(rT<T>(x2[j] * c[j]) + rT<T>(x1[j] * s[j]));
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) { o1[j] = (T)x1[j]; o2[j] = (T)x2[j]; }
        }
        if (hh < a.Hq) {
            T* q = (T*)a.q_out + (long)tok * a.Hq * HD + hh * HD + u * 8;
            *(V8*)q = o1; *(V8*)(q + HALF) = o2;
        } else if (hh < a.Hq + a.Hkv) {
            T* k = (T*)a.Kc + (((long)b * a.Hkv + (hh - a.Hq)) * a.ctx_max + pos) * HD + u * 8;
            *(V8*)k = o1; *(V8*)(k + HALF) = o2;
        } else {
            const int kvh = hh - a.Hq - a.Hkv;
            T* v = (T*)a.Vc + (((long)b * a.Hkv + kvh) * a.ctx_max + pos) * HD + u * 8;
            *(V8*)v = o1; *(V8*)(v + HALF) = o2;
            if (a.Vt) {
                T* vt = (T*)a.Vt + ((long)b * a.Hkv + kvh) * HD * a.vt_ld + pos;
#pragma unroll
                for (int j = 0; j < 8; ++j) { vt[(long)(u * 8 + j) * a.vt_ld] = o1[j]; vt[(long)(HALF + u * 8 + j) * a.vt_ld] = o2[j]; }
            }
        }
    }
}

// Prefill form (round 5): one block per (tile of 16 positions, sequence).  Same arithmetic per element as rope_append_kernel<T, false>; what changes
// is the V^T scratch: the tile's V rows go through LDS and leave as [hd][16 positions] = two 16-byte stores per row, where the per-token kernel
// wrote every V element with its own 2-byte store (8448 tokens x 512 elements: 103 us per layer, 2.9 ms of a 24 ms prefill).
template <typename T>
__global__ __launch_bounds__(256) void rope_append_pf_kernel(RopeAppendArgs a) {
    typedef typename ET<T>::v8 V8;
    constexpr int HD = 128, HALF = 64, TT = 16;
    extern __shared__ __attribute__((aligned(16))) char smem_ra[];            // [TT][Hkv * HD] V values of the tile
    T* sv = (T*)smem_ra;
    const int b = blockIdx.y, p0 = blockIdx.x * TT;
    const int P = a.q_len[b];
    if (p0 >= P) return;
    const int nt = min(TT, P - p0), tok0 = a.q_off[b] + p0;
    const int heads = a.Hq + 2 * a.Hkv, VW = a.Hkv * HD;
    for (int w = threadIdx.x; w < nt * heads * 8; w += blockDim.x) {
        const int t = w / (heads * 8), r = w - t * heads * 8, hh = r >> 3, u = r & 7;
        const int tok = tok0 + t, pos = a.tok_pos[tok];
        const T* p = (const T*)a.qkv + (long)tok * a.ld + hh * HD + u * 8;
        const V8 t1 = *(const V8*)p, t2 = *(const V8*)(p + HALF);
        V8 o1, o2;
        if (hh < a.Hq + a.Hkv) {
            const float* c = a.cs + (long)pos * HD + u * 8;
            const float* s = c + HALF;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float x1 = (float)t1[j], x2 = (float)t2[j];
                o1[j] = (T)(rT<T>(x1 * c[j]) + rT<T>(-x2 * s[j]));
                o2[j] = (T)(rT<T>(x2 * c[j]) + rT<T>(x1 * s[j]));
            }
        } else { o1 = t1; o2 = t2; }
        if (hh < a.Hq) {
            T* q = (T*)a.q_out + (long)tok * a.Hq * HD + hh * HD + u * 8;
            *(V8*)q = o1; *(V8*)(q + HALF) = o2;
        } else if (hh < a.Hq + a.Hkv) {
            T* k = (T*)a.Kc + (((long)b * a.Hkv + (hh - a.Hq)) * a.ctx_max + pos) * HD + u * 8;
            *(V8*)k = o1; *(V8*)(k + HALF) = o2;
        } else {
            const int kvh = hh - a.Hq - a.Hkv;
            T* v = (T*)a.Vc + (((long)b * a.Hkv + kvh) * a.ctx_max + pos) * HD + u * 8;
            *(V8*)v = o1; *(V8*)(v + HALF) = o2;
            if (a.Vt) { *(V8*)(sv + t * VW + kvh * HD + u * 8) = o1; *(V8*)(sv + t * VW + kvh * HD + HALF + u * 8) = o2; }
        }
    }
    if (!a.Vt) return;
    __syncthreads();
    // V^T[b][kvh][hd][pos]: row (kvh, hd) of the tile = TT consecutive positions starting at the tile's first position (prompt positions are 0 .. P-1,
    // so p0 is a multiple of 16: the row piece is 32 bytes, 16-byte aligned whenever vt_ld is a multiple of 8)
    const int pos0 = a.tok_pos[tok0];
    for (int rr = threadIdx.x; rr < VW; rr += blockDim.x) {
        T* vt = (T*)a.Vt + ((long)b * a.Hkv * HD + rr) * a.vt_ld + pos0;
        if (nt == TT && (pos0 & 7) == 0 && (a.vt_ld & 7) == 0) {
            V8 lo, hi;
#pragma unroll
            for (int j = 0; j < 8; ++j) { lo[j] = sv[j * VW + rr]; hi[j] = sv[(8 + j) * VW + rr]; }
            *(V8*)vt = lo; *(V8*)(vt + 8) = hi;
        } else {
            for (int j = 0; j < nt; ++j) vt[j] = sv[j * VW + rr];
        }
    }
}

// ---------------------------------------------------------------- embedding gather / audio scatter (modeling_glmasr.py:452-465)
// src[tok] >= 0: row of the embedding table; src[tok] < 0: audio row -(src+1) of `audio`.  (2-byte copies: dtype-agnostic)
__global__ void assemble_embeds_kernel(const int* src, const bf16_t* table, const bf16_t* audio, bf16_t* x, int n_tok, int d) {
    const int tok = blockIdx.x;
    const int s = src[tok];
    const bf16_t* from = s >= 0 ? table + (long)s * d : audio + (long)(-(s + 1)) * d;
    for (int c = threadIdx.x; c < (d >> 3); c += blockDim.x) *(bf16x8*)(x + (long)tok * d + c * 8) = *(const bf16x8*)(from + c * 8);
}

// ---------------------------------------------------------------- argmax + greedy controller (generation/utils.py:2894-2936)
// LP (option token_logprobs): the block also returns log_softmax(l)[tok] of the token it emits.  Every thread keeps the sum lp_s of
// exp(r - lp_m) over the values it visits, lp_m being its running maximum `best`: one rescale per trip of the unrolled loop, then the trip's (up to
// 16) terms.  Threads are brought to their wave's maximum and added by the xor butterfly, waves to the block's maximum and added as a fixed tree by
// thread 0: one block, one order, whatever the grid.  exp is v_exp_f32 of the argument times log2(e); the closing log and subtraction are fp64.
// LP = false is the kernel as it was: everything below that belongs to the sum sits behind `if constexpr (LP)`.
// GUARD (sonic_set_generation): HF's repetition_penalty, no_repeat_ngram_size and suppress_tokens on the fp32 scores the argmax compares.
// The block first builds two vocabulary bitmaps in LDS from the row's history hist[b][0 .. kv_len[b]) (prompt ids, then every id emitted): "seen" (ids of
// the history) and "banned" (continuations of earlier occurrences of the last n - 1 ids, and the suppress list).  Integer ORs: no order in them.  The
// loop then reads the 4 bits of each map that belong to its f32x4 group: a seen score becomes s < 0 ? s * p : s / p (fp32 multiply, correctly rounded
// fp32 divide), a banned one -inf, in that order, behind the dump (raw logits) and ahead of the compare and the LP sum.  Thread 0 appends the emitted
// id at hist[b][kv_len[b]].  A row whose scores are all -inf emits token 0 (torch.argmax of equal values).  GUARD = false is the kernel as it was.
// BIAS (option request_bias; implies GUARD): HF's SequenceBiasLogitsProcessor, with NoBadWordsLogitsProcessor folded in as entries of bias -inf
// (generation/logits_process.py; the reference's hotwords, backend/asr.py:303-333, are what it serves), on the row's own table GreedyArgs.bias_tab.  Thread e of the
// prologue decides whether entry e applies to the history (L = 1: always; else L <= len and the last L - 1 ids equal its prefix) and leaves a flag in LDS; the first
// entry of every last-id group then adds the group's flagged biases to +0.0 in stored order - HF's order: the length-1 value, then the longer sequences in list
// order - and leaves (id, sum) in the LDS list and the id's bit in a third bitmap, "biased".  The loop reads that map's 4 bits with the others; a set bit scans the
// list (every lane reads the same word: a broadcast) and adds the sum, once, ahead of guard_score: the bias is HF's first processor.  An unset bit adds nothing
// (HF adds +0.0 there, which changes no compare and no exponential).  BIAS = false is the kernel as it was, GUARD or not.
// SAMPLE (option sampling; LP only): temperature sampling by the Gumbel-max identity.  Row b reads GreedyArgs.samp[3b ..]: the bits of its
// temperature t, its seed's low and high word.  t == 0: no division, no noise - the row's token and out_lp are the bits of the LP kernel.  t > 0: the compare runs
// on y_i = fdiv_rn(s_i, t) + g_i, s the fully processed score (bias, penalty, bans: HF's order, then TemperatureLogitsWarper), g_i = -ln(-ln(u_i)) Gumbel noise
// from Philox4x32-10 with key = the seed, counter = (i >> 2, n_new[b], 0, 0), word i & 3: one call per f32x4 group; u = ((word >> 9) + 0.5) * 2^-23 lies
// strictly inside (0, 1).  The first maximum of y is an exact draw from softmax(s / t); it depends on (scores, t, seed, step) alone - not on batch, row or
// slot.  The log-probability sum still runs over s, against its own running maximum (`rmax`; without SAMPLE that maximum is `best`), and out_lp is
// log_softmax(s)[tok] at temperature 1 - openai-whisper's convention, the one its fallback thresholds are calibrated on; the emitted token's s is recomputed
// from the slabs as the forced id's is.  Teacher forcing wins over sampling; step_logits stay raw.  The two logs are logf - v_log_f32 (1 ulp) times ln 2 in extended precision, a relative error
// of at most 1.5 * 2^-23 each: |g - exact| <= (1 + 16.64) * 1.5 * 2^-23 < 3.2e-6.
extern __shared__ unsigned g_bits[];
__device__ __forceinline__ float guard_score(float r, unsigned seen, unsigned banned, float p) {
    if (seen & 1u) r = r < 0.f ? r * p : __fdiv_rn(r, p);
    return (banned & 1u) ? -INFINITY : r;
}
__device__ __forceinline__ void guard_set(unsigned* map, int id, int V) {
    if ((unsigned)id < (unsigned)V) atomicOr(&map[id >> 5], 1u << (id & 31));
}
__device__ __forceinline__ float bias_of(const int* ids, const float* sums, int n, int id) {
    float b = 0.f;
    for (int k = 0; k < n; ++k) if (ids[k] == id) b = sums[k];      // (ids are unique: one group per last id)
    return b;
}
__device__ __forceinline__ float lp_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between them
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned* out) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// 23 bits, centred: every value is exact in fp32 and inside (0, 1).  logf is the library's: relatively accurate also at u next to 1, where -ln(u) is tiny (the
// hardware logarithm's 1 ulp is of ITS result): no 1 - u form needed
__device__ __forceinline__ float gumbel_of(unsigned word) {
    const float u = ((float)(word >> 9) + 0.5f) * 1.1920928955078125e-7f;
    return -logf(-logf(u));
}
#define LPB (SAMPLE ? rmax : best)      // what the LP sum is taken against: the running maximum of s
template <typename T, bool LP, bool GUARD = false, bool BIAS = false, bool SAMPLE = false>
__global__ __launch_bounds__(1024) void greedy_kernel(GreedyArgs a) {
    static_assert(GUARD || !BIAS, "the request bias lives in the guard instantiations (it needs their history)");
    static_assert(LP || !SAMPLE, "sampling lives in the log-probability instantiations (the fallback ladder reads them)");
    typedef typename ET<T>::v8 V8;
    __shared__ float sv[16];
    __shared__ int si[17];
    __shared__ int s_tok;
    __shared__ float ss_lp[LP ? (SAMPLE ? 32 : 16) : 1];
    [[maybe_unused]] float* const ss_m = ss_lp + (SAMPLE ? 16 : 0);      // SAMPLE: the waves' maxima of the unperturbed scores (sv holds those of y)
    float lp_m = -INFINITY, lp_s = 0.f;      // LP: the thread's sum is lp_s * exp(lp_m); a thread that saw nothing holds (-inf, 0)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* lg = a.logits + (long)b * a.V;
    const long ks_stride = (long)a.mpad * a.V;
    float* dump = a.logits_dump ? a.logits_dump + (long)a.step_counter[b] * a.dump_stride_step + (long)b * a.V : nullptr;
    float best = -INFINITY; int bi = 0x7fffffff;
    // SAMPLE: the row's temperature, seed and step (block-uniform); rmax = the running maximum of s, which `best` (now over y) no longer is
    [[maybe_unused]] float temp = 0.f, rmax = -INFINITY; [[maybe_unused]] unsigned k0 = 0u, k1 = 0u, step_n = 0u; [[maybe_unused]] bool noisy = false;
    [[maybe_unused]] float* noise = nullptr;
    if constexpr (SAMPLE) {
        temp = __uint_as_float(a.samp[3 * b]); k0 = a.samp[3 * b + 1]; k1 = a.samp[3 * b + 2]; step_n = (unsigned)a.n_new[b];
        noisy = temp > 0.f;
        if (a.noise_out) noise = a.noise_out + (long)b * a.V;
    }
    // the first layer's norm weight for the tail of this kernel, requested before anything else (cold every step; behind the token's
    // embedding row it was one more dependent round trip)
    f32x4 gw0 = {0.f, 0.f, 0.f, 0.f}, gw1 = {0.f, 0.f, 0.f, 0.f};
    if (a.y && (a.d >> 3) <= 1024 && tid < (a.d >> 3)) { gw0 = *(const f32x4*)(a.norm_w + tid * 8); gw1 = *(const f32x4*)(a.norm_w + tid * 8 + 4); }
    [[maybe_unused]] unsigned* g_seen = nullptr; [[maybe_unused]] unsigned* g_ban = nullptr;
    [[maybe_unused]] unsigned* g_bia = nullptr; [[maybe_unused]] int* q_id = nullptr; [[maybe_unused]] float* q_sum = nullptr; [[maybe_unused]] int q_n = 0;
    if constexpr (GUARD) {
        const int nw = (a.V + 31) >> 5;
        g_seen = g_bits; g_ban = g_bits + nw;
        for (int w = tid; w < (BIAS ? 3 : 2) * nw; w += 1024) g_bits[w] = 0u;
        __syncthreads();
        const int* h = a.hist + (long)b * a.hist_ld;
        const int len = min(max(a.kv_len[b], 0), a.hist_ld), n = a.ngram;
        if constexpr (BIAS) {
            // dynamic LDS behind the three maps: the group sums' ids [256], the sums [256], the entries' flags [256] (greedy_guard_lds)
            g_bia = g_bits + 2 * nw; q_id = (int*)(g_bits + 3 * nw); q_sum = (float*)(q_id + BIAS_MAX_ENTRIES);
            int* q_flag = q_id + 2 * BIAS_MAX_ENTRIES;
            const int* tab = a.bias_tab + 64 + (long)b * BIAS_ROW_WORDS;
            q_n = min(max(a.bias_tab[b], 0), BIAS_MAX_ENTRIES);
            const int* en = tab + tid * BIAS_ENTRY_WORDS;
            int last = -1;
            if (tid < q_n) {
                last = en[0];
                const int L = en[1];
                bool m = L >= 1 && L <= BIAS_MAX_LEN && L <= len;          // (L == len + 1 would fit its prefix; HF ignores it, so does this)
                if (m) { const int* tail = h + len - (L - 1); for (int k = 0; k < L - 1; ++k) m = m && tail[k] == en[3 + k]; }
                q_flag[tid] = (L == 1 || m) ? 1 : 0;                       // a single id has no prefix to match: it applies whatever the history holds
                q_id[tid] = -1;
            }
            __syncthreads();
            if (tid < q_n && (unsigned)last < (unsigned)a.V && (tid == 0 || en[-BIAS_ENTRY_WORDS] != last)) {      // the first entry of its last-id group
                float acc = 0.f; bool any = false;
                for (int k = tid; k < q_n && tab[k * BIAS_ENTRY_WORDS] == last; ++k)
                    if (q_flag[k]) { acc += __int_as_float(tab[k * BIAS_ENTRY_WORDS + 2]); any = true; }
                if (any) { q_id[tid] = last; q_sum[tid] = acc; guard_set(g_bia, last, a.V); }
            }
        }
        for (int j = tid; j < len; j += 1024) guard_set(g_seen, h[j], a.V);
        if (n > 0) {                              // every n-gram h[j .. j + n) of the history whose first n - 1 ids are the history's last n - 1 bans its last id
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
    // four strides per trip with all their slab loads issued first (the rolled form paid one L2 round trip per stride)
    constexpr int U = 4;
    for (int i0 = tid * 4; i0 < a.V; i0 += 1024 * 4 * U) {
        f32x4 v[U], w[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 4096, ic = i < a.V ? i : 0;
            v[u] = *(const f32x4*)(lg + ic);
            w[u] = *(const f32x4*)(lg + (a.ksplit > 1 ? ks_stride : 0) + ic);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 4096;
            if (i >= a.V) break;
            f32x4 t = v[u];
            if (a.ksplit > 1) t += w[u];
            for (int ks = 2; ks < a.ksplit; ++ks) t += *(const f32x4*)(lg + ks * ks_stride + i);
            [[maybe_unused]] unsigned sb = 0u, bb = 0u;      // GUARD: the group's 4 bits of each map (i is a multiple of 4)
            if constexpr (GUARD) { sb = g_seen[i >> 5] >> (i & 31); bb = g_ban[i >> 5] >> (i & 31); }
            [[maybe_unused]] unsigned qb = 0u;               // BIAS: the group's 4 bits of the "biased" map
            if constexpr (BIAS) qb = (g_bia[i >> 5] >> (i & 31)) & 15u;
            [[maybe_unused]] float gz[4] = {0.f, 0.f, 0.f, 0.f};      // SAMPLE: the group's Gumbel values, one Philox call
            if constexpr (SAMPLE) if (noisy) {
                unsigned pw[4];
                philox4x32_10((unsigned)i >> 2, step_n, 0u, 0u, k0, k1, pw);
#pragma unroll
                for (int j = 0; j < 4; ++j) { gz[j] = gumbel_of(pw[j]); if (noise) noise[i + j] = gz[j]; }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float r = rT<T>(t[j]);              // logits are T in the reference, compared as fp32
                if (dump) dump[i + j] = r;
                if constexpr (BIAS) if ((qb >> j) & 1u) r += bias_of(q_id, q_sum, q_n, i + j);      // HF's order: the bias first, the penalty sees the biased score
                if constexpr (GUARD) r = guard_score(r, sb >> j, bb >> j, a.rep_penalty);
                if constexpr (SAMPLE) {
                    const float y = noisy ? __fdiv_rn(r, temp) + gz[j] : r;      // (-inf stays -inf: g is finite)
                    if (y > best) { best = y; bi = i + j; }
                    rmax = fmaxf(rmax, r);                                       // (t == 0: rmax == best, bit for bit)
                } else {
                    if (r > best) { best = r; bi = i + j; }   // strict > keeps the first maximum within a thread
                }
                if constexpr (LP) v[u][j] = r;
            }
        }
        if constexpr (LP) {
            // the trip's values against the maximum so far (`best` covers them): the old sum is rescaled once (exp2(0) = 1 and s * 1 are exact when
            // the maximum did not move), then the terms are added in visiting order.  While nothing finite has been seen (the first trip, or trips
            // of -inf logits only) the sum stays 0: -inf - -inf is not formed, here or in the terms (exp(-inf - finite) = 0 is fine)
            lp_s = lp_m > -INFINITY ? lp_s * lp_exp(lp_m - LPB) : 0.f; lp_m = LPB;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (i0 + u * 4096 >= a.V) break;
#pragma unroll
                for (int j = 0; j < 4; ++j) lp_s += LPB > -INFINITY ? lp_exp(v[u][j] - LPB) : 0.f;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if constexpr (SAMPLE) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, o, 64));
        if (lane == 0) ss_m[wid] = rmax;
    }
    if constexpr (LP) {
        // every lane now holds the wave's maximum: bring the lane's sum to it (an empty lane is the identity: 0, not 0 * exp(-inf + inf)) and add
        // across the wave; the butterfly gives every lane the same tree, and a + b = b + a bit for bit
        lp_s = lp_m > -INFINITY ? lp_s * lp_exp(lp_m - LPB) : 0.f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) lp_s += __shfl_xor(lp_s, o, 64);
        if (lane == 0) ss_lp[wid] = lp_s;
    }
    if (lane == 0) { sv[wid] = best; si[wid] = bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
        float lp_sum = 0.f;
        if constexpr (LP) {
            float q[16];                          // the 16 waves at the block's maximum (an empty wave: 0), added as a fixed binary tree
            const float* wm = SAMPLE ? ss_m : sv; // the waves' maxima of the scores the sum ran over
            if constexpr (SAMPLE) for (int w = 1; w < 16; ++w) rmax = fmaxf(rmax, ss_m[w]);
#pragma unroll
            for (int w = 0; w < 16; ++w) q[w] = wm[w] > -INFINITY ? ss_lp[w] * lp_exp(wm[w] - LPB) : 0.f;
#pragma unroll
            for (int h = 8; h > 0; h >>= 1)
#pragma unroll
                for (int w = 0; w < h; ++w) q[w] = q[2 * w] + q[2 * w + 1];
            lp_sum = q[0];
        }
        if constexpr (GUARD || SAMPLE) if (bi == 0x7fffffff) bi = 0;      // every score -inf: the first of equal values
        int tok = bi;
        const int fin = a.finished[b];
        bool running = false;
        if (fin) tok = a.pad_id;                 // finished rows emit the pad token (:2928-2929)
        else {
            if (a.force_ids) tok = a.force_ids[(long)b * a.force_ld + a.n_new[b]];   // teacher forcing (parity tests): feed this id instead
            a.out_ids[(long)b * a.out_ld + a.n_new[b]] = tok;
            if constexpr (LP) {
                float lt = LPB;                   // the emitted token's logit: the maximum, or under teacher forcing the forced id's value, summed
                // from the slabs in the main loop's order (v + w, then ks = 2 ...): the bits of the dumped logit.  SAMPLE: a sampled token is rarely the maximum of s
                if (SAMPLE ? (a.force_ids || noisy) && (unsigned)tok < (unsigned)a.V : a.force_ids != nullptr) {
                    float f = lg[tok];
                    if (a.ksplit > 1) f += lg[ks_stride + tok];
                    for (int ks = 2; ks < a.ksplit; ++ks) f += lg[ks * ks_stride + tok];
                    lt = rT<T>(f);
                    if constexpr (BIAS) if ((g_bia[tok >> 5] >> (tok & 31)) & 1u) lt += bias_of(q_id, q_sum, q_n, tok);
                    if constexpr (GUARD) lt = guard_score(lt, g_seen[tok >> 5] >> (tok & 31), g_ban[tok >> 5] >> (tok & 31), a.rep_penalty);
                }
                a.out_lp[(long)b * a.out_ld + a.n_new[b]] = (float)(((double)lt - (double)LPB) - log((double)lp_sum));
            }
            if constexpr (GUARD) { const int pos = a.kv_len[b]; if (pos >= 0 && pos < a.hist_ld) a.hist[(long)b * a.hist_ld + pos] = tok; }   // the token's position
            const int nn = a.n_new[b] + 1;
            a.n_new[b] = nn;
            bool stop = nn >= a.max_new[b];
            for (int e = 0; e < a.n_eos; ++e) stop |= (tok == a.eos[e]);
            if (stop) { a.finished[b] = 1; atomicSub(a.n_active, 1); } else running = true;
        }
        // device error word (SkinnyArgs.err = n_active[1]): a kernel of this step gave up on an in-kernel wait, its outputs are garbage.  The count of
        // running rows goes (and stays) far below zero: the loop stops at its next check and the host fails the batch (DEV_ERR_ACTIVE in engine_internal.h)
        if (a.dev_err && b == 0 && *a.dev_err) atomicMin(a.n_active, -(1 << 24));
        // Only a row that keeps running advances its context.  A finished row stays where it is (its later steps rewrite the same
        // cache slot and are discarded), so kv_len never exceeds prompt + max_new - 1 < max_ctx whatever the other rows' budgets are:
        // before, a [long prompt, small budget] row riding a [short prompt, large budget] batch walked past its cache region.
        if (running) {
            a.tok_pos[b] = a.kv_len[b];          // the new token sits right after the current context
            a.kv_len[b] += 1;
        }
        s_tok = tok;
        if (a.step_counter) a.step_counter[b] += 1;
    }
    __syncthreads();
    const T* row = (const T*)a.table + (long)s_tok * a.d;
    T* xo = (T*)a.x;
    if (!a.y || (a.d >> 3) > 1024) {
        for (int c = tid; c < (a.d >> 3); c += 1024) *(V8*)(xo + (long)b * a.d + c * 8) = *(const V8*)(row + c * 8);
        return;
    }
    // next step's input row and, in the same pass, the first decoder layer's input RMSNorm of it (modeling_llama.py:60-65, :306):
    // one launch less per token step
    const int c = tid, nv = a.d >> 3;
    V8 xv;
    float ss = 0.f;
    if (c < nv) {
        xv = *(const V8*)(row + c * 8);
        *(V8*)(xo + (long)b * a.d + c * 8) = xv;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = (float)xv[j]; ss += f * f; }
    }
    ss = wave_sum(ss);
    __syncthreads();                         // sv is reused below
    if (lane == 0) sv[wid] = ss;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += sv[w];
    const float r = 1.0f / sqrtf(tot / a.d + a.norm_eps);
    float yo[8];
    if (c < nv) {
        V8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) { o[j] = (T)((j < 4 ? gw0[j & 3] : gw1[j & 3]) * rT<T>((float)xv[j] * r)); yo[j] = (float)o[j]; }
        *(V8*)((T*)a.y + (long)b * a.d + c * 8) = o;
    }
    if (a.qo.q) quant_emit_row(yo, c < nv, c, b, a.qo, sv, si);
}
#undef LPB

// ---------------------------------------------------------------- misc
// In-stream fill of small control words.  hipMemsetAsync of a few bytes was observed not to be reliably ordered against
// the neighbouring kernels of a non-blocking stream (a stale per-segment log-mel maximum survived a reset on some runs);
// a kernel on the stream is.
__global__ void fill_i32_kernel(int* p, int value, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = value;
}
void launch_fill_i32(int* p, int value, int n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(fill_i32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p, value, n);
}
template <typename T> __global__ void f32_to_t_kernel(const float* in, T* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (T)in[i];
}
template <typename T> __global__ void t_to_f32_kernel(const T* in, float* out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
__global__ void bf16_to_f16_kernel(const bf16_t* in, f16_t* out, long n) {   // a bf16 checkpoint loaded with torch_dtype=float16 (asr.py:156)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (f16_t)(float)in[i];
}

// sonicscribe_amd/synth.py restated for the device: writes bf16 and/or fp32
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__global__ void synth_fill_kernel(unsigned long long key, long n, float scale, float offset, bf16_t* out_bf, float* out_f32, int round_f32) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long z = mix64(key + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ULL);
    const int bits = (int)(z >> 40);
    const float r = __fsub_rn(__fmul_rn((float)bits, 0x1p-23f), 1.0f);
    const float v = __fadd_rn(offset, __fmul_rn(r, scale));
    if (out_bf) out_bf[i] = f2bf(v);
    if (out_f32) out_f32[i] = (out_bf || round_f32) ? rbf(v) : v;      // fp32 alone: the generator's exact value (synth.synth_fill(..., bf16=False)) unless round_f32
}

// ---------------------------------------------------------------- launchers
void launch_layernorm(const bf16_t* x, const float* w, const float* b, bf16_t* y, int rows, int d, float eps, hipStream_t s, int dt, const QuantActArgs* qa) {
    const QuantActArgs q = qa ? *qa : QuantActArgs{};
    if (q.q) { DT_SWITCH(dt, T, hipLaunchKernelGGL((layernorm_kernel<T, true>), dim3((rows + 3) / 4), dim3(256), 0, s, (const T*)x, w, b, (T*)y, rows, d, eps, q)); }
    else { DT_SWITCH(dt, T, hipLaunchKernelGGL((layernorm_kernel<T, false>), dim3((rows + 3) / 4), dim3(256), 0, s, (const T*)x, w, b, (T*)y, rows, d, eps, q)); }
}
void launch_rmsnorm(const bf16_t* x, const float* w, bf16_t* y, int rows, int d, float eps, const int* row_map, hipStream_t s, int dt, const QuantActArgs* qa) {
    const QuantActArgs q = qa ? *qa : QuantActArgs{};
    if (q.q) { DT_SWITCH(dt, T, hipLaunchKernelGGL((rmsnorm_kernel<T, true>), dim3((rows + 3) / 4), dim3(256), 0, s, (const T*)x, w, (T*)y, rows, d, eps, row_map, q)); }
    else { DT_SWITCH(dt, T, hipLaunchKernelGGL((rmsnorm_kernel<T, false>), dim3((rows + 3) / 4), dim3(256), 0, s, (const T*)x, w, (T*)y, rows, d, eps, row_map, q)); }
}
void launch_add_rmsnorm(bf16_t* x, const float* P, int ksplit, int mpad, const float* w, bf16_t* y, int rows, int d, float eps, hipStream_t s,
                        int dt, const DeqInfo* dq, const QuantOut* qo, const PrefetchRange* pf, int pf_blocks) {
    const int threads = ((d >> 3) + 63) / 64 * 64;   // d <= 2048 -> <= 256 threads
    const DeqInfo q = dq ? *dq : DeqInfo{};
    const QuantOut o = qo ? *qo : QuantOut{};
    const PrefetchRange r = pf ? *pf : PrefetchRange{nullptr, 0};
    const int extra = pf && pf->p && pf_blocks > 0 ? pf_blocks : 0;
    DT_SWITCH(dt, T, hipLaunchKernelGGL(add_rmsnorm_kernel<T>, dim3(rows + extra), dim3(threads), 0, s, (T*)x, P, ksplit, mpad, w, (T*)y, rows, d, eps, q, o, r));
}
void launch_swiglu_slab(const float* P, int ksplit, int mpad, int n2, bf16_t* act, int rows, hipStream_t s, int dt, int gu8) {
    const long n = (long)rows * (n2 >> 3);
    DT_SWITCH(dt, T, hipLaunchKernelGGL(swiglu_slab_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, s, P, ksplit, mpad, n2, (T*)act, rows, gu8));
}
void launch_swiglu_quant(const float* P, int ksplit, int mpad, int ff, bf16_t* act, int rows, const DeqInfo& dq, const QuantOut& qo, hipStream_t s) {
    hipLaunchKernelGGL(swiglu_quant_kernel, dim3(rows), dim3(1024), 0, s, P, ksplit, mpad, ff, (f16_t*)act, dq, qo);
}
void launch_quant_rows(const bf16_t* X, long ld, int M, int K, const QuantOut& qo, hipStream_t s) {
    hipLaunchKernelGGL(quant_rows_kernel, dim3(M), dim3(1024), 0, s, (const f16_t*)X, ld, K, qo);
}
void launch_rope_enc(bf16_t* qk, long ld, int M, int T, int heads2, int hd, int rd, const float* cs, hipStream_t s, int dt) {
    const long n = (long)M * heads2 * (rd >> 4);
    DT_SWITCH(dt, E, hipLaunchKernelGGL(rope_enc_kernel<E>, dim3((n + 255) / 256), dim3(256), 0, s, (E*)qk, ld, M, T, heads2, hd, rd, cs));
}
void launch_rope_append(const RopeAppendArgs& a, bool slab, hipStream_t s) {
    if (a.n_tok <= 0) return;
    if (!slab && a.q_off && a.q_len && a.n_seq > 0 && a.max_p > 0 && a.Hkv * 128 * 16 * 2 <= 65536) {      // prefill: tiles of 16 positions per sequence
        DT_SWITCH(a.dt, T, hipLaunchKernelGGL((rope_append_pf_kernel<T>), dim3((a.max_p + 15) / 16, a.n_seq), dim3(256), (size_t)a.Hkv * 128 * 16 * 2, s, a));
        return;
    }
    DT_SWITCH(a.dt, T, {
        if (slab) hipLaunchKernelGGL((rope_append_kernel<T, true>), dim3(a.n_tok), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((rope_append_kernel<T, false>), dim3(a.n_tok), dim3(256), 0, s, a);
    });
}
void launch_assemble_embeds(const int* src, const bf16_t* table, const bf16_t* audio, bf16_t* x, int n_tok, int d, hipStream_t s) {
    if (n_tok > 0) hipLaunchKernelGGL(assemble_embeds_kernel, dim3(n_tok), dim3(256), 0, s, src, table, audio, x, n_tok, d);
}
// a request's prompt ids into its history row (option generation guards): token t of the packed prompt plan is position tok_pos[t] of request
// tok_seq[t]; audio positions (src < 0) hold the placeholder id, as in HF's input_ids
__global__ void hist_prompt_kernel(const int* src, const int* tok_seq, const int* tok_pos, int n_tok, int audio_id, int* hist, int hist_ld) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tok) return;
    const int s = src[t], r = tok_seq[t], p = tok_pos[t];
    if (r >= 0 && r < 64 && p >= 0 && p < hist_ld) hist[(long)r * hist_ld + p] = s >= 0 ? s : audio_id;
}
void launch_hist_prompt(const int* src, const int* tok_seq, const int* tok_pos, int n_tok, int audio_id, int* hist, int hist_ld, hipStream_t s) {
    if (n_tok > 0) hipLaunchKernelGGL(hist_prompt_kernel, dim3((n_tok + 255) / 256), dim3(256), 0, s, src, tok_seq, tok_pos, n_tok, audio_id, hist, hist_ld);
}
size_t greedy_guard_lds(int V, bool bias) { return (size_t)(bias ? 3 : 2) * ((V + 31) / 32) * 4 + (bias ? (size_t)3 * BIAS_MAX_ENTRIES * 4 : 0); }
void launch_greedy(const GreedyArgs& a, hipStream_t s) {
    if (a.samp && a.out_lp) {                                                                                    // option sampling: the SAMPLE instantiations of the three LP families
        if (a.hist && a.bias_tab) {
            const size_t lds = greedy_guard_lds(a.V, true);
            if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, true, true, true, true>), dim3(a.B), dim3(1024), lds, s, a); return; }
            DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, true, true, true, true>), dim3(a.B), dim3(1024), lds, s, a));
            return;
        }
        if (a.hist) {
            const size_t lds = greedy_guard_lds(a.V);
            if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, true, true, false, true>), dim3(a.B), dim3(1024), lds, s, a); return; }
            DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, true, true, false, true>), dim3(a.B), dim3(1024), lds, s, a));
            return;
        }
        if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, true, false, false, true>), dim3(a.B), dim3(1024), 0, s, a); return; }
        DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, true, false, false, true>), dim3(a.B), dim3(1024), 0, s, a));
        return;
    }
    if (a.hist && a.bias_tab) {                                                                                  // request bias: the BIAS instantiations (a third bitmap and the matched list)
        const size_t lds = greedy_guard_lds(a.V, true);
        if (a.out_lp) {
            if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, true, true, true>), dim3(a.B), dim3(1024), lds, s, a); return; }
            DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, true, true, true>), dim3(a.B), dim3(1024), lds, s, a));
            return;
        }
        if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, false, true, true>), dim3(a.B), dim3(1024), lds, s, a); return; }
        DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, false, true, true>), dim3(a.B), dim3(1024), lds, s, a));
        return;
    }
    if (a.hist) {                                                                                                // generation guards: the GUARD instantiations, two bitmaps of dynamic LDS
        const size_t lds = greedy_guard_lds(a.V);
        if (a.out_lp) {
            if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, true, true>), dim3(a.B), dim3(1024), lds, s, a); return; }
            DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, true, true>), dim3(a.B), dim3(1024), lds, s, a));
            return;
        }
        if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, false, true>), dim3(a.B), dim3(1024), lds, s, a); return; }
        DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, false, true>), dim3(a.B), dim3(1024), lds, s, a));
        return;
    }
    if (a.out_lp) {                                                                                              // token_logprobs: the LP instantiation
        if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, true>), dim3(a.B), dim3(1024), 0, s, a); return; }
        DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, true>), dim3(a.B), dim3(1024), 0, s, a));
        return;
    }
    if (a.dt == DT_F32) { hipLaunchKernelGGL((greedy_kernel<float, false>), dim3(a.B), dim3(1024), 0, s, a); return; }   // SONIC_MODE_F32: fp32 logits, table and rows
    DT_SWITCH(a.dt, T, hipLaunchKernelGGL((greedy_kernel<T, false>), dim3(a.B), dim3(1024), 0, s, a));
}
void launch_f32_to_bf16(const float* in, bf16_t* out, long n, hipStream_t s, int dt) {
    if (n > 0) DT_SWITCH(dt, T, hipLaunchKernelGGL(f32_to_t_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, s, in, (T*)out, n));
}
void launch_bf16_to_f32(const bf16_t* in, float* out, long n, hipStream_t s, int dt) {
    if (n > 0) DT_SWITCH(dt, T, hipLaunchKernelGGL(t_to_f32_kernel<T>, dim3((n + 255) / 256), dim3(256), 0, s, (const T*)in, out, n));
}
void launch_bf16_to_f16(const bf16_t* in, bf16_t* out, long n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(bf16_to_f16_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, (f16_t*)out, n);
}
void launch_synth_fill(unsigned long long key, long n, float scale, float offset, bf16_t* out_bf, float* out_f32, hipStream_t s, int round_f32) {
    if (n > 0) hipLaunchKernelGGL(synth_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, s, key, n, scale, offset, out_bf, out_f32, round_f32);
}
