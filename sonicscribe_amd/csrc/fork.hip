// Row forks (sonic_load_tensor "request_forks"): behind the prefill's last decoder layer, the K and V a forked request left in its cache row - and,
// where the rows' histories are kept, its input_ids - are copied to the rows of its forks.  From then on a fork is an ordinary row.
// fork_kv_kernel: a pure copy, read once and written cnt times - every 16-byte piece of the source is loaded by one thread, which then stores it to each of the
// source's forks (a splice_kv_kernel launch per fork would read the source cnt times).  The copy of one (source, layer, kv head) is kv_len * hd 16-bit elements:
// with one audio at full width that is 28 x 4 such ranges, fewer blocks than the chip has CUs, so the range is split over the grid's third axis - slice z takes the
// pieces j with j / 256 % Z == z, the 256 threads of a block always 4 KiB of consecutive bytes.  No LDS, no atomics; the loads of a trip are issued ahead of its stores.
#include "common.h"
#include "kernels.h"

__global__ __launch_bounds__(256) void fork_kv_kernel(ForkArgs a) {
    const int i = blockIdx.x, lh = blockIdx.y, s = a.src[i], d0 = a.first[i], cnt = a.cnt[i];
    const int len = min(max(a.kv_len[s], 0), a.ctx);
    const long blk = (long)a.ctx * a.hd;                                        // elements of one (row, head) range of the cache
    const long row = (long)a.Hkv * blk;                                         // ... of one row of a layer
    const long so = ((long)(lh / a.Hkv) * a.Bm + s) * row + (long)(lh % a.Hkv) * blk;
    const long dd = ((long)(lh / a.Hkv) * a.Bm + d0) * row + (long)(lh % a.Hkv) * blk;
    const uint4* ks = (const uint4*)(a.Kc + so); const uint4* vs = (const uint4*)(a.Vc + so);
    uint4* kd = (uint4*)(a.Kc + dd); uint4* vd = (uint4*)(a.Vc + dd);
    const long step = row / 8;                                                   // 16-byte pieces from one row's range to the next row's
    const int n16 = len * (a.hd / 8);
    for (int j = blockIdx.z * 256 + threadIdx.x; j < n16; j += gridDim.z * 256) {
        const uint4 k = ks[j], v = vs[j];
        for (int f = 0; f < cnt; ++f) { kd[f * step + j] = k; vd[f * step + j] = v; }
    }
    if (a.hist && lh == 0)                                                       // the rows' input_ids ride along: kv_len ints, whatever their count's alignment
        for (int j = blockIdx.z * 256 + threadIdx.x; j < len; j += gridDim.z * 256) {
            const int t = a.hist[(long)s * a.ctx + j];
            for (int f = 0; f < cnt; ++f) a.hist[(long)(d0 + f) * a.ctx + j] = t;
        }
}

// the grid: (sources, layers x kv heads, Z), Z slices so that a launch with few sources still brings about eight blocks per CU, never more slices than a
// range has 4 KiB trips
void launch_fork_kv(const ForkArgs& a, int max_len, hipStream_t s) {
    if (a.n_src < 1 || max_len < 1) return;
    const int ranges = a.n_src * a.layers * a.Hkv;
    const int trips = (max_len * (a.hd / 8) + 255) / 256;
    int Z = (2048 + ranges - 1) / ranges;
    if (Z > trips) Z = trips;
    if (Z < 1) Z = 1;
    hipLaunchKernelGGL(fork_kv_kernel, dim3(a.n_src, a.layers * a.Hkv, Z), dim3(256), 0, s, a);
}
