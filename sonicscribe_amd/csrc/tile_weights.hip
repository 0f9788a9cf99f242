// Weight layout kernels (weight load only): row-major W[N][K] -> the fragment-tiled copies that the decode-step kernels
// (skinny.hip, skinny_fused.hip, gemv.hip) and gemm_kernel's w_tiled path read.  The comments here define those layouts.
#include "common.h"

// W[N][K] row-major -> fragment-tiled: element (n, k) goes to ((n/16)*(K/32) + k/32)*512 + (((k%32)/8)*16 + n%16)*8 + k%8,
// i.e. the 64 lanes of the MFMA A-operand of (row tile, k-step) read 64 consecutive 16-byte pieces.
__global__ void tile_weights_kernel(const bf16_t* w, bf16_t* wt, int N, int K) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;   // one 8-element piece per thread
    if (e >= (long)N * (K >> 3)) return;
    const int n = e / (K >> 3), kc = e % (K >> 3), k = kc * 8;
    const long dst = ((long)(n >> 4) * (K >> 5) + (k >> 5)) * 512 + ((((k & 31) >> 3) * 16) + (n & 15)) * 8;
    *(bf16x8*)(wt + dst) = *(const bf16x8*)(w + (long)n * K + k);
}
// gate/up variant: the source has gate and up rows interleaved in groups of 16 (the prefill GEMM's SwiGLU epilogue layout); the tiled
// copy interleaves them in groups of 8, so tile t = gate rows [8t, 8t+8) followed by up rows [8t, 8t+8)
__global__ void tile_weights_gu8_kernel(const bf16_t* w, bf16_t* wt, int N, int K) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)N * (K >> 3)) return;
    const int n = e / (K >> 3), kc = e % (K >> 3), k = kc * 8;       // n = destination row
    const int t = n >> 4, i = n & 15, q = t * 8 + (i & 7);           // q = gate/up row index
    const int src = (q >> 4) * 32 + (i >> 3) * 16 + (q & 15);
    const long dst = ((long)t * (K >> 5) + (k >> 5)) * 512 + ((((k & 31) >> 3) * 16) + i) * 8;
    *(bf16x8*)(wt + dst) = *(const bf16x8*)(w + (long)src * K + k);
}
void launch_tile_weights_gu8(const bf16_t* w, bf16_t* wt, int N, int K, hipStream_t s) {
    const long n = (long)N * (K >> 3);
    hipLaunchKernelGGL(tile_weights_gu8_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w, wt, N, K);
}
void launch_tile_weights(const bf16_t* w, bf16_t* wt, int N, int K, hipStream_t s) {
    const long n = (long)N * (K >> 3);
    hipLaunchKernelGGL(tile_weights_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w, wt, N, K);
}

// e4m3 variant (mode fp8; written by fp8_snap_kernel in gemv_fp8.hip from a bf16 tiled copy, whose row order - plain or the gate/up 8-row interleave - it keeps):
// one byte per weight, a (16-row, 64-k) tile is 1 KiB = 64 lanes x 16 bytes.  Lane (kc, n%16) of the bf16 tiling owns k = u*32 + kc*8 + e of k-step u; its e4m3
// piece holds those 8 k of the TWO consecutive k-steps u = 2p (bytes 0 .. 7) and u = 2p + 1 (bytes 8 .. 15), so a lane still issues 16-byte loads: element (n, k)
// goes to (((n/16)*(K/64) + k/64)*64 + ((k%32)/8)*16 + n%16)*16 + ((k/32)%2)*8 + k%8.  K % 64 == 0.

// int8 variant: a (16-row, 64-k) MFMA A-operand tile of v_mfma_i32_16x16x64_i8 is 1 KiB; element (n, k) goes to
// ((n/16)*(K/64) + k/64)*1024 + (((k%64)/16)*16 + n%16)*16 + k%16
__global__ void tile_weights_i8_kernel(const int8_t* w, int8_t* wt, int N, int K) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;   // one 16-byte piece per thread
    if (e >= (long)N * (K >> 4)) return;
    const int n = e / (K >> 4), kc = e % (K >> 4), k = kc * 16;
    const long dst = ((long)(n >> 4) * (K >> 6) + (k >> 6)) * 1024 + ((((k & 63) >> 4) * 16) + (n & 15)) * 16;
    *(i32x4*)(wt + dst) = *(const i32x4*)(w + (long)n * K + k);
}
void launch_tile_weights_i8(const int8_t* w, int8_t* wt, int N, int K, hipStream_t s) {
    const long n = (long)N * (K >> 4);
    hipLaunchKernelGGL(tile_weights_i8_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w, wt, N, K);
}
