// Shallow fusion with a token n-gram language model (option lm): lm_step_kernel turns a row's LM state into the fp32 vector the greedy kernel adds to
// that row's scores, once per token step, right ahead of it.  The automaton (kernels.h LmArgs; sonicscribe_amd/ngram.py is its host twin and the numpy reference) is a
// backoff model in CSR form: node 0 the empty context, bo_next / bo_w the backoff link and weight of every other node, a node's edges ascending by token id.
// Contract, all in fp32 with separately rounded operations (__fadd_rn / __fmul_rn: nothing is contracted), L the handle's weight:
//   chain     c_0 = the row's node, c_{j+1} = bo_next[c_j] down to c_k = 0;  A_0 = +0, A_{j+1} = A_j + bo_w[c_j]
//   dense     add[w] = L * (A_k + uni[w]) for every id
//   levels    for j = k - 1 down to 0 and every edge e of c_j: add[edge_tok[e]] = L * (A_j + edge_w[e]) - the longest context that lists an id wins, so the passes are
//             separated by barriers (their stores have been acknowledged when a wave arrives: __syncthreads waits for them)
//   step      a pending token t (lm_tok >= 0) is consumed first: t is searched among the node's edges; found, the state is the edge's `next`; else the search repeats at
//             bo_next, and ends at the root - as does a token outside [0, V)
// Wave 0 makes the transition and walks the chain.  The search is 64-ary: the 64 lanes probe an evenly spaced sample of the range, one ballot narrows it to one
// stride, and a range of at most 64 edges is matched by one probe per lane - two dependent loads for a node of 2 000 edges where a bisection on one thread needs 11.
#include "common.h"
#include "kernels.h"

// the index of `t` among edge_tok[lo .. hi), or -1; every lane of the wave returns the same value
__device__ __forceinline__ int lm_find(const int* edge_tok, int lo, int hi, int t, int lane) {
    while (hi - lo > 64) {
        const int step = (hi - lo + 63) >> 6, i = lo + lane * step;
        const bool le = i < hi && edge_tok[i] <= t;               // (ascending tokens: the lanes that see a token <= t are a prefix of the wave)
        const int n = __popcll(__ballot(le));
        if (n == 0) return -1;                                     // t lies below the range's first token
        lo += (n - 1) * step;
        hi = min(lo + step, hi);
    }
    const bool eq = lo + lane < hi && edge_tok[lo + lane] == t;
    const unsigned long long m = __ballot(eq);
    return m ? lo + (int)__ffsll((long long)m) - 1 : -1;
}

__global__ __launch_bounds__(1024) void lm_step_kernel(LmArgs a) {
    __shared__ int s_c[LM_MAX_ORDER + 1];
    __shared__ float s_A[LM_MAX_ORDER + 1];
    __shared__ int s_k;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (a.finished[b]) return;                                     // block-uniform
    const int V = a.blob[0], N = a.blob[1], E = a.blob[2];
    const float* uni = (const float*)(a.blob + LM_HEAD);
    const int* node_off = a.blob + LM_HEAD + V;
    const int* bo_next = node_off + N + 1;
    const float* bo_w = (const float*)(bo_next + N);
    const int* edge_tok = bo_next + 2 * (long)N;
    const int* edge_next = edge_tok + E;
    const float* edge_w = (const float*)(edge_next + E);
    if (tid < 64) {
        int n = a.state[b];
        if (n < 0 || n >= N) n = 0;                                // (a state the blob does not hold - never written by the engine - counts as the root)
        const int t = a.tok[b];
        if (t >= 0) {
            if (t >= V) n = 0;
            else for (int it = 0; it < LM_MAX_ORDER; ++it) {       // (a validated chain has at most order - 1 <= 7 links)
                const int e = lm_find(edge_tok, node_off[n], node_off[n + 1], t, lane);
                if (e >= 0) { n = edge_next[e]; break; }
                if (n == 0) break;
                n = bo_next[n];
            }
            if (n < 0 || n >= N) n = 0;
            if (lane == 0) { a.state[b] = n; a.tok[b] = -1; }
        }
        if (lane == 0) {
            int k = 0; float A = 0.f;
            s_c[0] = n; s_A[0] = A;
            while (n != 0 && k < LM_MAX_ORDER) { A = __fadd_rn(A, bo_w[n]); n = bo_next[n]; ++k; s_c[k] = n; s_A[k] = A; }
            s_k = k;
        }
    }
    __syncthreads();
    const int k = s_k;
    const float L = a.weight, Ak = s_A[k];
    float* add = a.add + (long)b * V;
    if ((V & 3) == 0) {
        for (int i = tid * 4; i < V; i += 4096) {
            const f32x4 u = *(const f32x4*)(uni + i);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = __fmul_rn(L, __fadd_rn(Ak, u[j]));
            *(f32x4*)(add + i) = o;
        }
    } else
        for (int i = tid; i < V; i += 1024) add[i] = __fmul_rn(L, __fadd_rn(Ak, uni[i]));
    for (int j = k - 1; j >= 0; --j) {
        __syncthreads();
        const int c = s_c[j], hi = min(node_off[c + 1], E);
        const float Aj = s_A[j];
        for (int e = max(node_off[c], 0) + tid; e < hi; e += 1024) {
            const int w = edge_tok[e];
            if ((unsigned)w < (unsigned)V) add[w] = __fmul_rn(L, __fadd_rn(Aj, edge_w[e]));
        }
    }
}

void launch_lm_step(const LmArgs& a, hipStream_t s) {
    if (a.B > 0) hipLaunchKernelGGL(lm_step_kernel, dim3(a.B), dim3(1024), 0, s, a);
}
