// Word timestamps on the parallel forced run (option forced_align): openai-whisper's find_alignment on the decoder's self-attention onto the audio
// placeholder run.  Three kernels, all fp32 behind the 16-bit q / k:
//   align_probs_kernel<T>   per (score row, selected head): s[a] = scale * (q . k_{a0+a}) over 128 dims, p = softmax over the A audio keys of the row's sequence
//   align_reduce_kernel     per (sequence, 58-column tile, head): mean / population std of p[.][a] over the sequence's L rows, z = (p - mean) / std (std = 0: z = 0),
//                           median of 7 along a with reflect padding (A <= 3: unchanged) -> Z; align_accum_kernel then adds M[n][a] += z_f / H_total, the launch's
//                           heads in ascending order
//   align_dtw_kernel        per sequence: whisper/timing.py::dtw_cpu on -M as an anti-diagonal wavefront, three live diagonals in LDS, int8 trace in global
//                           scratch, thread 0 walks the trace back; t_n = the audio index of the first path step whose text index is n
// One order everywhere: a thread owns its keys / columns / cells and visits them in ascending order, sums across threads are the xor butterfly and a fixed tree, every
// M element is added to by exactly one thread, launch after launch in stream order - no floating-point atomics.  Nothing a (row, head) produces depends on the
// launch's other sequences, on the row's index, on the strides of the buffers or on the handle.
#include "common.h"
#include "kernels.h"

#define ALIGN_TILE 58      // columns per block of align_reduce_kernel: with 3 either side for the median, one wave of 64 columns

// numpy / torch "reflect" (no edge repeat), one fold: enough for |overhang| <= 3 < A
__device__ __forceinline__ int align_reflect(int i, int A) { return i < 0 ? -i : (i >= A ? 2 * (A - 1) - i : i); }

template <typename T>
__global__ __launch_bounds__(256) void align_probs_kernel(AlignArgs a) {
    typedef typename ET<T>::v8 V8;
    __shared__ float qs[128];
    __shared__ float red[4];
    const int s = blockIdx.x, hi = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int h = a.heads[hi], r = a.rseq[s];
    const int a0 = a.seqp[4 * r + 2], A = a.seqp[4 * r + 3];
    const T* q = (const T*)a.Q + (long)a.qrow[s] * a.q_ld + (long)h * 128;
    if (tid < 128) qs[tid] = (float)q[tid];
    __syncthreads();
    const T* kb = (const T*)a.K + (long)r * a.k_seq_stride + (long)(h / a.grp) * a.k_head_stride + (long)a0 * a.k_ld;
    float* prow = a.P + ((long)hi * a.S + s) * a.A_max;
    float mx = -INFINITY;
    for (int c = tid; c < A; c += 256) {
        const T* k = kb + (long)c * a.k_ld;
        float acc = 0.f;
#pragma unroll 4
        for (int d = 0; d < 128; d += 8) {
            const V8 x = *(const V8*)(k + d);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf(qs[d + j], (float)x[j], acc);
        }
        const float sc = acc * a.scale;
        prow[c] = sc;
        mx = fmaxf(mx, sc);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wid] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int c = tid; c < A; c += 256) {      // (a thread reads back what it wrote itself)
        const float ex = expf(prow[c] - mx);
        prow[c] = ex;
        sum += ex;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    sum = (red[0] + red[1]) + (red[2] + red[3]);
    for (int c = tid; c < A; c += 256) prow[c] = prow[c] / sum;
}

__device__ __forceinline__ void align_cswap(float& x, float& y) { const float lo = fminf(x, y), hi = fmaxf(x, y); x = lo; y = hi; }

__global__ __launch_bounds__(256) void align_reduce_kernel(AlignArgs a) {
    __shared__ float part_s[4][64];
    __shared__ float mean_s[64];
    __shared__ float sd_s[64];
    const int r = blockIdx.y, c0 = blockIdx.x * ALIGN_TILE, hi = blockIdx.z, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row0 = a.seqp[4 * r], L = a.seqp[4 * r + 1], A = a.seqp[4 * r + 3];
    if (c0 >= A) return;
    const bool filt = A > 3;
    const float fl = (float)L;
    const float* P = a.P + ((long)hi * a.S + row0) * a.A_max;
    float* Z = a.Z + ((long)hi * a.S + row0) * a.A_max;
    // the tile's 58 columns and 3 either side (reflected): lane = column, wave w takes rows w, w + 4, ... in ascending order; the four partial sums are added as
    // (w0 + w1) + (w2 + w3)
    const int raw = c0 - 3 + lane;
    const bool valid = raw <= A + 2 && (filt || (raw >= 0 && raw < A));
    const int col = valid ? (filt ? align_reflect(raw, A) : raw) : 0;
    float sum = 0.f;
    if (valid) for (int n = w; n < L; n += 4) sum += P[(long)n * a.A_max + col];
    part_s[w][lane] = sum;
    __syncthreads();
    const float mean = ((part_s[0][lane] + part_s[1][lane]) + (part_s[2][lane] + part_s[3][lane])) / fl;
    __syncthreads();
    float var = 0.f;
    if (valid) for (int n = w; n < L; n += 4) { const float dlt = P[(long)n * a.A_max + col] - mean; var = fmaf(dlt, dlt, var); }
    part_s[w][lane] = var;
    __syncthreads();
    if (w == 0) { mean_s[lane] = mean; sd_s[lane] = sqrtf(((part_s[0][lane] + part_s[1][lane]) + (part_s[2][lane] + part_s[3][lane])) / fl); }
    __syncthreads();
    for (int idx = tid; idx < L * ALIGN_TILE; idx += 256) {
        const int n = idx / ALIGN_TILE, cc = idx % ALIGN_TILE, c = c0 + cc;
        if (c >= A) continue;
        const float* prow = P + (long)n * a.A_max;
        float med;
        if (filt) {
            float z[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const float sd = sd_s[cc + j];
                z[j] = sd > 0.f ? (prow[align_reflect(c - 3 + j, A)] - mean_s[cc + j]) / sd : 0.f;
            }
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int j = 0; j < 6 - p; ++j) align_cswap(z[j], z[j + 1]);
            med = z[3];
        } else {
            const float sd = sd_s[cc + 3];
            med = sd > 0.f ? (prow[c] - mean_s[cc + 3]) / sd : 0.f;
        }
        Z[(long)n * a.A_max + c] = med;
    }
}

// M[n][a] += z_f / H_total, the launch's heads in ascending order: one thread per element, so the order is the same on every run
__global__ __launch_bounds__(256) void align_accum_kernel(AlignArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.S * a.A_max) return;
    const int s = (int)(idx / a.A_max), c = (int)(idx % a.A_max);
    if (c >= a.seqp[4 * a.rseq[s] + 3]) return;
    float m = a.M[idx];
    for (int hi = 0; hi < a.n_heads; ++hi) m += a.Z[((long)hi * a.S + s) * a.A_max + c] / a.h_total;
    a.M[idx] = m;
}

__global__ __launch_bounds__(256) void align_dtw_kernel(AlignArgs a) {
    extern __shared__ float dg[];                    // three diagonals, each indexed by the text index i in 0 .. L
    const int r = blockIdx.x, tid = threadIdx.x;
    const int row0 = a.seqp[4 * r], L = a.seqp[4 * r + 1], A = a.seqp[4 * r + 3];
    const int ld = a.L_max + 1;
    if (tid == 0) { dg[0] = 0.f; dg[ld] = INFINITY; dg[ld + 1] = INFINITY; }      // cost[0][0]; cost[0][1], cost[1][0]
    __syncthreads();
    for (int d = 2; d <= L + A; ++d) {
        float* cur = dg + (d % 3) * ld;
        const float* p1 = dg + ((d - 1) % 3) * ld;
        const float* p2 = dg + ((d - 2) % 3) * ld;
        const int lo = d - A > 0 ? d - A : 0, hi = d < L ? d : L;
        for (int i = lo + tid; i <= hi; i += 256) {
            const int j = d - i;
            if (i == 0 || j == 0) { cur[i] = INFINITY; continue; }
            const float c0 = p2[i - 1], c1 = p1[i - 1], c2 = p1[i];
            float c; signed char t;
            if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
            else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
            else { c = c2; t = 2; }
            const long at = (long)(row0 + i - 1) * a.A_max + (j - 1);
            cur[i] = -a.M[at] + c;
            a.trace[at] = t;
        }
        __syncthreads();
    }
    if (tid != 0) return;
    int i = L, j = A;
    while (i > 0 && j > 0) {                         // (the path reaches (0, 0) through (1, 1): a border cell's cost is infinite)
        const signed char t = a.trace[(long)(row0 + i - 1) * a.A_max + (j - 1)];
        if (t != 2) {                                // the walk leaves text index i - 1 here: j - 1 is its first audio index on the path
            a.t_out[a.rec[row0 + i - 1]] = (float)(j - 1);
            --i;
        }
        if (t != 1) --j;
    }
}

void launch_align_probs(const AlignArgs& a, hipStream_t s) {
    if (a.S < 1 || a.n_heads < 1) return;
    DT_SWITCH(a.dt, T, hipLaunchKernelGGL(align_probs_kernel<T>, dim3(a.S, a.n_heads), dim3(256), 0, s, a));
}
void launch_align_reduce(const AlignArgs& a, hipStream_t s) {
    if (a.S < 1 || a.n_heads < 1) return;
    hipLaunchKernelGGL(align_reduce_kernel, dim3((a.A_max + ALIGN_TILE - 1) / ALIGN_TILE, a.n_seq, a.n_heads), dim3(256), 0, s, a);
    hipLaunchKernelGGL(align_accum_kernel, dim3((unsigned)(((long)a.S * a.A_max + 255) / 256)), dim3(256), 0, s, a);
}
void launch_align_dtw(const AlignArgs& a, hipStream_t s) {
    if (a.S < 1) return;
    hipLaunchKernelGGL(align_dtw_kernel, dim3(a.n_seq), dim3(256), (size_t)3 * (a.L_max + 1) * sizeof(float), s, a);
}
