// Polyphase windowed-sinc resampler (replaces torchaudio.transforms.Resample at backend/asr.py:255-261,
// backend/vad.py:63-67 / :108-112 and pydub's set_frame_rate(16000) at backend/utils.py:18).  The algorithm is the one
// sonicscribe_amd/frontend.py resample_sinc_hann restates (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99):
//     of = in_rate / g, nf = out_rate / g, g = gcd;  base = min(of, nf) * 0.99;  width = ceil(6 * of / base);  K = 2 * width + of
//     y[i * nf + p] = sum_{k = 0 .. K-1} bank[p][k] * x[i * of - width + k]          (x = 0 outside the stream)
// One thread owns one output and accumulates with fmaf in ascending k from +0, zero-padded taps included, so an output's bits depend on
// the stream's samples alone: not on the grid, the tile, the k chunking, the piece of the stream a launch covers or the ring position.
// The bank lies k-major on the device ([K][nf]): the lanes of a wave are consecutive phases p and read consecutive words at a given k
// (nf == 1: one word, broadcast).  A block stages the input span of its tile of outputs in LDS as fp32 (int16 input: s * 2^-15, exact);
// the lanes of one frame read the same LDS word (broadcast), lanes of neighbouring frames words `of` apart.
// fp32 VALU work, at most 475 MACs per output (44.1 kHz): 152 MMAC per 20 s of audio.
#include "common.h"
#include "kernels.h"

template <typename T> __device__ __forceinline__ float rs_load(const void* src, long s);
template <> __device__ __forceinline__ float rs_load<short>(const void* src, long s) { return (float)((const short*)src)[s] * (1.0f / 32768.0f); }
template <> __device__ __forceinline__ float rs_load<float>(const void* src, long s) { return ((const float*)src)[s]; }

template <typename T> __global__ __launch_bounds__(256) void resample_kernel(ResampleArgs a) {
    __shared__ float xs[RS_LDS_FLOATS];
    const int of = a.of, nf = a.nf, K = a.K;
    const long j_end = a.j0 + a.n_out;
    const long jt = a.j0 + (long)blockIdx.x * a.tile;                 // first output of this block's tile
    const long jl = jt + a.tile < j_end ? jt + a.tile : j_end;        // one past its last
    const long i_lo = jt / nf;                                        // first frame of the tile
    const int span = (int)((jl - 1) / nf - i_lo) * of;                // input samples between the tile's first and last frame (host: span + kc <= LDS)
    const long j = jt + threadIdx.x;
    const bool active = (int)threadIdx.x < a.tile && j < jl;
    const long i = active ? j / nf : i_lo;
    const int p = active ? (int)(j - i * nf) : 0;
    const float* xp = xs + (int)(i - i_lo) * of;
    float acc = 0.0f;
    for (int k0 = 0; k0 < K; k0 += a.kc) {
        const int kn = K - k0 < a.kc ? K - k0 : a.kc;
        const long s0 = i_lo * of - a.width + k0 - a.src_base;        // index in src of xs[0] (may be negative: zeros before the stream)
        const int len = span + kn;
        for (int t = threadIdx.x; t < len; t += 256) {
            const long s = s0 + t;
            xs[t] = (s >= 0 && s < a.src_n) ? rs_load<T>(a.src, s) : 0.0f;
        }
        __syncthreads();
        if (active) {
            const float* bp = a.bank + (long)k0 * nf + p;
            for (int k = 0; k < kn; ++k) acc = fmaf(bp[(long)k * nf], xp[k], acc);
        }
        __syncthreads();
    }
    if (!active) return;
    const long o = j - a.j0;
    if (a.out_f32) a.out_f32[o] = acc;
    if (a.ring) {
        // the ring's int16 content: round-half-even as ring_stage_kernel, no contraction; sinc overshoot of full-scale input exceeds 1
        const float q = rintf(__fmul_rn(acc, 32768.0f));
        long pos = a.ring_pos + o;                                    // n_out <= ring_cap (host)
        pos = pos >= a.ring_cap ? pos - a.ring_cap : pos;
        a.ring[pos] = (short)fminf(fmaxf(q, -32768.0f), 32767.0f);
    }
}

// buf[dst .. dst + n) = buf[src .. src + n) with dst < src, ranges may overlap (the carry of a rate ring moves to the front of its
// linear buffer).  One block; a batch is read whole before it is written, and a later batch only reads above what was written.
__global__ __launch_bounds__(256) void resample_carry_kernel(short* buf, long dst, long src, long n) {
    for (long b = 0; b < n; b += 256) {
        const long t = b + threadIdx.x;
        const short v = t < n ? buf[src + t] : (short)0;
        __syncthreads();
        if (t < n) buf[dst + t] = v;
        __syncthreads();
    }
}

void resample_plan(int of, int nf, int K, int* tile, int* kc) {
    // the largest tile of outputs whose input span leaves room for at least min(K, 1024) taps per pass
    int t = 256;
    const int want = K < 1024 ? K : 1024;
    while (t > 1 && (long)((t - 1 + nf - 1) / nf) * of + want > RS_LDS_FLOATS) t >>= 1;
    long span = (long)((t - 1 + nf - 1) / nf) * of;
    if (t == 1) span = 0;
    long c = RS_LDS_FLOATS - span;
    *tile = t;
    *kc = (int)(c < K ? c : K);
}

void launch_resample(const ResampleArgs& a, bool src_f32, hipStream_t s) {
    for (long done = 0; done < a.n_out;) {                            // at most 2^20 blocks per launch
        ResampleArgs b = a;
        b.n_out = a.n_out - done < ((long)a.tile << 20) ? a.n_out - done : ((long)a.tile << 20);
        b.j0 = a.j0 + done;
        if (b.out_f32) b.out_f32 += done;
        if (b.ring) b.ring_pos = (a.ring_pos + done) % a.ring_cap;
        const unsigned blocks = (unsigned)((b.n_out + a.tile - 1) / a.tile);
        if (src_f32) hipLaunchKernelGGL(resample_kernel<float>, dim3(blocks), dim3(256), 0, s, b);
        else hipLaunchKernelGGL(resample_kernel<short>, dim3(blocks), dim3(256), 0, s, b);
        done += b.n_out;
    }
}

void launch_resample_carry(short* buf, long dst, long src, long n, hipStream_t s) {
    if (n < 1 || dst == src) return;
    hipLaunchKernelGGL(resample_carry_kernel, dim3(1), dim3(256), 0, s, buf, dst, src, n);
}
