// sonic_hip engine: the kernel test hooks (sonic_test_*) and bench hooks (sonic_bench_*) of the C ABI, and the temporary device buffers they work in.
#include "engine_internal.h"

static void fill_words(int* p, int value, size_t n, hipStream_t st) {      // n words of `value`, in launches of at most 2^30 words
    while (n > 0) { const int c = n > (1u << 30) ? (1 << 30) : (int)n; launch_fill_i32(p, value, c, st); p += c; n -= c; }
}
// The device buffers of one hook call, freed when it returns.  bad(): an allocation (get) or an upload (up_bf16 / up_f32) of this call has failed; every hook asks
// once, before its first launch on the buffers, instead of testing each pointer.
struct TmpBuf {
    std::vector<void*> v;
    hipStream_t st;
    bool failed = false; bool bad() const { return failed; }
    explicit TmpBuf(hipStream_t s) : st(s) {}
    ~TmpBuf() { for (void* p : v) (void)hipFree(p); }
    // Zero-fill with a KERNEL on the engine stream.  hipMemsetAsync on this non-blocking stream was seen not to be reliably ordered
    // against its neighbours (a stale log-mel maximum survived one in round 1); here a late zero fill would wipe a buffer that a
    // conversion kernel or a GEMM has already written - the signature of the intermittent test_gemm256_path failures (gross errors on
    // a few tiles, clean on an immediate rerun, never in the engine's own long-lived buffers).
    template <typename Tt> Tt* get(size_t n) {
        void* p = nullptr;
        const size_t bytes = (((n ? n : 1) * sizeof(Tt)) + 3) / 4 * 4;
        if (hipMalloc(&p, bytes) != hipSuccess) { failed = true; return nullptr; }
        fill_words((int*)p, 0, bytes / 4, st);
        (void)hipStreamSynchronize(st);
        v.push_back(p);
        return (Tt*)p;
    }
};
static bf16_t* up_bf16(sonic_engine* e, TmpBuf& tb, const float* h, size_t n, size_t pad = 0) {
    float* f = tb.get<float>(n); bf16_t* b = tb.get<bf16_t>(n + pad);
    if (!f || !b) return nullptr;
    if (h2d(e, f, h, n * 4) != hipSuccess) { tb.failed = true; return nullptr; }
    launch_f32_to_bf16(f, b, (long)n, e->st, e->dt);     // the engine's element type: bf16, or fp16 on an int8-mode engine
    return b;
}
static float* up_f32(sonic_engine* e, TmpBuf& tb, const float* h, size_t n) {
    float* f = tb.get<float>(n);
    if (f && h2d(e, f, h, n * 4) != hipSuccess) { tb.failed = true; return nullptr; }
    return f;
}
static int down_bf16(sonic_engine* e, TmpBuf& tb, const bf16_t* d, float* h, size_t n) {
    float* f = tb.get<float>(n);
    if (!f) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    launch_bf16_to_f32(d, f, (long)n, e->st, e->dt);
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    HIPC(e, d2h(e, h, f, n * 4));
    return SONIC_OK;
}
int read_back_16(sonic_engine* e, const bf16_t* d, float* h, size_t n) { TmpBuf tb(e->st); return down_bf16(e, tb, d, h, n); }

// ------------------------------------------------------------------------------------------ C ABI: kernel test hooks
extern "C" int sonic_test_gemm(sonic_engine* e, const float* A, const float* W, const float* bias, const float* resid, float* C,
                               int M, int N, int K, int epi) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    if (K % 64 || N % 4) return fail(e, SONIC_ERR_INVALID, "K must be a multiple of 64 and N of 4");
    TmpBuf tb(e->st);
    const int Nout = (epi == EPI_SWIGLU) ? N / 2 : N;
    bf16_t* dA = up_bf16(e, tb, A, (size_t)M * K); bf16_t* dW = up_bf16(e, tb, W, (size_t)N * K);
    float* db = bias ? up_f32(e, tb, bias, N) : nullptr;
    bf16_t* dR = resid ? up_bf16(e, tb, resid, (size_t)M * Nout) : nullptr;
    bf16_t* dC = tb.get<bf16_t>((size_t)M * Nout);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    gemm(e, epi, dA, K, dW, db, dC, Nout, M, N, K, dR, Nout);
    return down_bf16(e, tb, dC, C, (size_t)M * Nout);
}

extern "C" int sonic_test_skinny(sonic_engine* e, const float* X, const float* W, float* C, int M, int N, int K) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    if (M < 1 || M > 64 || N % 16 || K % 256 || skinny_pick_ksplit(N, K) < 1) return fail(e, SONIC_ERR_INVALID, "skinny: M<=64, N%%16==0, K%%256==0");
    TmpBuf tb(e->st);
    bf16_t* dX = up_bf16(e, tb, X, (size_t)M * K); bf16_t* dW = up_bf16(e, tb, W, (size_t)N * K);
    bf16_t* dWt = tb.get<bf16_t>((size_t)N * K);
    const int ks = skinny_pick_ksplit(N, K), mpad = ((M + 15) / 16) * 16;
    float* P = tb.get<float>((size_t)ks * mpad * N);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    launch_tile_weights(dW, dWt, N, K, e->st);
    launch_skinny(skinny_args(dX, K, dWt, P, M, N, K, ks, e->dt), e->st);
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    std::vector<float> h((size_t)ks * mpad * N);
    HIPC(e, d2h(e, h.data(), P, h.size() * 4));
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) {
            float s = 0;
            for (int k = 0; k < ks; ++k) s += h[((size_t)k * mpad + m) * N + n];
            C[(size_t)m * N + n] = s;
        }
    return SONIC_OK;
}

__global__ void test_transpose_v_kernel(const bf16_t* v, bf16_t* vt, int B, int Tk, int Hkv, int hd, int ld_t) {
    // v [B][Tk][Hkv*hd] -> vt [B][Hkv][hd][ld_t]
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)B * Tk * Hkv * hd) return;
    const int c = e % (Hkv * hd), t = (e / (Hkv * hd)) % Tk, b = e / ((long)Hkv * hd * Tk);
    vt[(((long)b * Hkv + c / hd) * hd + c % hd) * ld_t + t] = v[e];
}

// sonic_test_attention on an align handle (option forced_align): the three word-timestamp kernels on caller data through production's descriptor
// (align_probs_args).  q [B][Tq][Hq * 128], k [B][Tk][Hkv * 128]; every one of the Hq heads takes part, the audio run is all Tk keys of a sequence, its rows are its
// Tq queries.  out [B][Tq][Tk + 1]: M's row, then t_n.  The caller holds the lock
static int test_align(sonic_engine* e, const float* q, const float* k, float* out, int B, int Tq, int Tk, int Hq, int Hkv, int hd, int causal) {
    if (!q || !k || !out) return fail(e, SONIC_ERR_INVALID, "align hook: q, k and out are needed");
    if (hd != 128 || causal) return fail(e, SONIC_ERR_INVALID, "align hook: hd = 128 and causal = 0 (every audio key lies before every row)");
    if (B < 1 || B > 64 || Tq < 1 || Tq > ALIGN_MAX_ROWS || Tk < 1 || Hkv < 1 || Hq % Hkv || Hq > ALIGN_MAX_HEADS || (long)B * Tq > e->tok_cap)
        return fail(e, SONIC_ERR_INVALID, "align hook: bad shape (B <= 64, Tq <= %d, B * Tq <= tok_cap = %d, Hq <= %d a multiple of Hkv)", ALIGN_MAX_ROWS, e->tok_cap, ALIGN_MAX_HEADS);
    const int S = B * Tq;
    TRY(align_alloc(e, S, Tk, Hq));
    TmpBuf tb(e->st);
    bf16_t* dq = up_bf16(e, tb, q, (size_t)S * Hq * 128);
    bf16_t* dk = up_bf16(e, tb, k, (size_t)B * Tk * Hkv * 128);
    float* dt_out = tb.get<float>(S); int* rec = tb.get<int>(S);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    std::vector<int> plan(AlignPlan::words(e->tok_cap), 0), iota(S);
    const AlignPlan ap(plan.data(), e->tok_cap);
    for (int b = 0, s = 0; b < B; ++b) {
        int* sp = ap.seq + 4 * b;
        sp[0] = s; sp[1] = Tq; sp[2] = 0; sp[3] = Tk;
        for (int n = 0; n < Tq; ++n, ++s) { ap.qrow[s] = s; ap.rseq[s] = b; iota[s] = s; }
    }
    for (int h = 0; h < Hq; ++h) ap.heads[h] = h;
    HIPC(e, h2d(e, e->align_plan_d, plan.data(), plan.size() * 4));
    HIPC(e, h2d(e, rec, iota.data(), (size_t)S * 4));
    e->align_S = S; e->align_nseq = B; e->align_Amax = Tk; e->align_Lmax = Tq; e->align_Htot = Hq; e->align_last_heads = Hq; e->align_last = false;
    fill_words((int*)e->align_M, 0, (size_t)S * Tk, e->st);
    AlignArgs a = align_probs_args(e, dq, dk, Hkv * 128L, 128, (long)Tk * Hkv * 128, AlignPlan(e->align_plan_d, e->tok_cap).heads, Hq, Hq, Hkv, rec);
    a.t_out = dt_out;
    launch_align_probs(a, e->st);
    launch_align_reduce(a, e->st);
    launch_align_dtw(a, e->st);
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    std::vector<float> m((size_t)S * Tk), t(S);
    HIPC(e, d2h(e, m.data(), e->align_M, m.size() * 4));
    HIPC(e, d2h(e, t.data(), dt_out, (size_t)S * 4));
    for (int s = 0; s < S; ++s) { memcpy(out + (size_t)s * (Tk + 1), m.data() + (size_t)s * Tk, (size_t)Tk * 4); out[(size_t)s * (Tk + 1) + Tk] = t[s]; }
    return SONIC_OK;
}

extern "C" int sonic_test_attention(sonic_engine* e, const float* q, const float* k, const float* v, float* out,
                                    int B, int Tq, int Tk, int Hq, int Hkv, int hd, int causal) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    if (e->opt_forced_align) return test_align(e, q, k, out, B, Tq, Tk, Hq, Hkv, hd, causal);
    if (hd != 64 && hd != 128) return fail(e, SONIC_ERR_INVALID, "hd must be 64 or 128");
    TmpBuf tb(e->st);
    const int Tkp = (Tk + 63) / 64 * 64;
    bf16_t* dq = up_bf16(e, tb, q, (size_t)B * Tq * Hq * hd);
    bf16_t* dk = up_bf16(e, tb, k, (size_t)B * Tk * Hkv * hd, (size_t)64 * Hkv * hd);
    bf16_t* dv = up_bf16(e, tb, v, (size_t)B * Tk * Hkv * hd);
    bf16_t* dvt = tb.get<bf16_t>((size_t)B * Hkv * hd * Tkp);
    bf16_t* dO = tb.get<bf16_t>((size_t)B * Tq * Hq * hd);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    const long nv = (long)B * Tk * Hkv * hd;
    hipLaunchKernelGGL(test_transpose_v_kernel, dim3((nv + 255) / 256), dim3(256), 0, e->st, dv, dvt, B, Tk, Hkv, hd, Tkp);
    FlashArgs f{};
    f.Q = dq; f.q_ld = (long)Hq * hd; f.K = dk; f.k_ld = (long)Hkv * hd; f.Vt = dvt; f.vt_ld = Tkp; f.O = dO; f.o_ld = (long)Hq * hd;
    f.q_seq_stride = (long)Tq * Hq * hd; f.k_seq_stride = (long)Tk * Hkv * hd; f.k_head_stride = hd;
    f.vt_seq_stride = (long)Hkv * hd * Tkp; f.vt_head_stride = (long)hd * Tkp; f.T = Tq; f.Hq = Hq; f.Hkv = Hkv; f.scale = 1.0f / sqrtf((float)hd); f.dt = e->dt;
    int *ql = nullptr, *kl = nullptr;
    if (Tq != Tk) {   // per-sequence lengths (decode-style offset: query t sits at position Tk - Tq + t)
        ql = tb.get<int>(B); kl = tb.get<int>(B);
        std::vector<int> a(B, Tq), b2(B, Tk);
        HIPC(e, h2d(e, ql, a.data(), B * 4)); HIPC(e, h2d(e, kl, b2.data(), B * 4));
        f.q_len = ql; f.kv_len = kl;
    }
    launch_flash(f, hd, causal != 0, B, Tq, e->st);
    return down_bf16(e, tb, dO, out, (size_t)B * Tq * Hq * hd);
}

extern "C" int sonic_test_decode_attention(sonic_engine* e, const float* q, const float* k, const float* v, float* out, int B, int Tk, int Hq, int Hkv) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    const int hd = 128, ctx = (Tk + 63) / 64 * 64;
    if (Hq % Hkv || Hq / Hkv > 4) return fail(e, SONIC_ERR_INVALID, "bad GQA group");
    TmpBuf tb(e->st);
    // k, v given as [B][Tk][Hkv*hd]; cache layout is [B][Hkv][ctx][hd]
    std::vector<float> kc((size_t)B * Hkv * ctx * hd, 0.f), vc(kc.size(), 0.f);
    for (int b = 0; b < B; ++b) for (int t = 0; t < Tk; ++t) for (int h = 0; h < Hkv; ++h) for (int i = 0; i < hd; ++i) {
        const size_t s = (((size_t)b * Tk + t) * Hkv + h) * hd + i, dd = (((size_t)b * Hkv + h) * ctx + t) * hd + i;
        kc[dd] = k[s]; vc[dd] = v[s];
    }
    bf16_t* dq = up_bf16(e, tb, q, (size_t)B * Hq * hd); bf16_t* dk = up_bf16(e, tb, kc.data(), kc.size()); bf16_t* dv = up_bf16(e, tb, vc.data(), vc.size());
    bf16_t* dO = tb.get<bf16_t>((size_t)B * Hq * hd); int* kl = tb.get<int>(B);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    std::vector<int> l(B, Tk); HIPC(e, h2d(e, kl, l.data(), B * 4));
    launch_decode_attn(decode_attn_args(dk, dv, nullptr, dq, 0, 0, nullptr, dO, kl, Hq, Hkv, ctx, e->dt), B, e->st);
    return down_bf16(e, tb, dO, out, (size_t)B * Hq * hd);
}

// The decode attention through decode_step()'s own descriptor builder (decode_attn_args) - fused mode (slabs != null: slab sum, RoPE at kv_len - 1, K/V append, kv_len - 1 cached keys + the new one
// from LDS) - or with a given q (slabs == null), over caller-filled caches and per-row kv_len.  The caches are read back after the launch.
extern "C" int sonic_test_decode_attention_cache(sonic_engine* e, const float* q, const float* slabs, int ksplit, int mpad, const float* rope_cs,
                                                 const float* kcache, const float* vcache, const int32_t* kv_len, float* out, float* kcache_out, float* vcache_out,
                                                 int B, int Hq, int Hkv, int ctx_max) {
    if (!e || !kcache || !vcache || !kv_len || !out || (q == nullptr) == (slabs == nullptr)) return SONIC_ERR_INVALID;
    ENTER(e);
    const int hd = 128;
    if (e->f32) return fail(e, SONIC_ERR_INVALID, "decode attention hook needs a 16-bit engine");
    if (B < 1 || B > 4096 || Hkv < 1 || Hq < Hkv || Hq % Hkv || Hq / Hkv > 4 || ctx_max < 1) return fail(e, SONIC_ERR_INVALID, "bad decode attention test shape");
    if (slabs && (!rope_cs || ksplit < 1 || ksplit > 8 || mpad < B)) return fail(e, SONIC_ERR_INVALID, "fused decode attention: rope table, 1 <= ksplit <= 8, mpad >= B");
    for (int b = 0; b < B; ++b)
        if (kv_len[b] < 1 || kv_len[b] > ctx_max) return fail(e, SONIC_ERR_INVALID, "kv_len[%d] = %d outside 1..%d", b, kv_len[b], ctx_max);
    TmpBuf tb(e->st);
    const size_t nc = (size_t)B * Hkv * ctx_max * hd, no = (size_t)B * Hq * hd, N = (size_t)(Hq + 2 * Hkv) * hd;
    bf16_t* dk = up_bf16(e, tb, kcache, nc); bf16_t* dv = up_bf16(e, tb, vcache, nc);
    bf16_t* dq = q ? up_bf16(e, tb, q, no) : nullptr;
    float* dP = slabs ? up_f32(e, tb, slabs, (size_t)ksplit * mpad * N) : nullptr;
    float* dcs = slabs ? up_f32(e, tb, rope_cs, (size_t)ctx_max * hd) : nullptr;
    bf16_t* dO = tb.get<bf16_t>(no); int* kl = tb.get<int>(B);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    HIPC(e, h2d(e, kl, kv_len, (size_t)B * 4));
    launch_decode_attn(decode_attn_args(dk, dv, dP, dq, ksplit, mpad, dcs, dO, kl, Hq, Hkv, ctx_max, e->dt), B, e->st);
    TRY(down_bf16(e, tb, dO, out, no));
    if (kcache_out) TRY(down_bf16(e, tb, dk, kcache_out, nc));
    if (vcache_out) TRY(down_bf16(e, tb, dv, vcache_out, nc));
    return SONIC_OK;
}

// sonic_load_tensor "share_prompt.hook": int32 [2][B] = pre_row | pre_len, armed until the next sonic_test_prefill_attention takes it (that call checks it against its shapes)
int share_hook_arm(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (dtype != SONIC_DTYPE_I32 || ndim != 2 || shape[0] != 2 || shape[1] < 1 || shape[1] > 4096)
        return fail(nullptr, SONIC_ERR_INVALID, "share_prompt.hook: int32 [2][B] (pre_row | pre_len), 1 <= B <= 4096");
    std::lock_guard<std::mutex> lk(e->mu);
    e->hook_share.assign((const int*)data, (const int*)data + 2 * shape[1]);
    return SONIC_OK;
}
// The causal attention of the prefill through run_prefill()'s own descriptor builder (prefill_flash_args): packed ragged queries (q_off / q_len / kv_len), K in cache layout, V^T with the
// context as its leading dimension, head dim 128.  `out` [n_tok][Hq * 128] is uploaded first, so rows the kernel leaves alone keep the caller's values.  An armed
// "share_prompt.hook" is consumed: sequence b's keys [0, pre_len[b]) are then those of cache row pre_row[b] (the shared-prefix kernel of option forced_share_prompt)
extern "C" int sonic_test_prefill_attention(sonic_engine* e, const float* q, const float* kcache, const float* vt, const int32_t* q_off, const int32_t* q_len,
                                            const int32_t* kv_len, float* out, int n_tok, int B, int Hq, int Hkv, int ctx_max) {
    if (!e || !q || !kcache || !vt || !q_off || !q_len || !kv_len || !out) return SONIC_ERR_INVALID;
    ENTER(e);
    std::vector<int> share; share.swap(e->hook_share);      // (an armed "share_prompt.hook" is consumed whatever becomes of the call)
    const int hd = 128;
    if (e->f32) return fail(e, SONIC_ERR_INVALID, "prefill attention hook needs a 16-bit engine");
    if (B < 1 || B > 4096 || n_tok < 1 || Hkv < 1 || Hq < Hkv || Hq % Hkv || ctx_max < 64 || ctx_max % 64) return fail(e, SONIC_ERR_INVALID, "bad prefill attention test shape");
    int max_p = 0;
    for (int b = 0; b < B; ++b) {
        if (q_len[b] < 1 || kv_len[b] < q_len[b] || kv_len[b] > ctx_max || q_off[b] < 0 || (long)q_off[b] + q_len[b] > n_tok)
            return fail(e, SONIC_ERR_INVALID, "sequence %d: q_off %d, q_len %d, kv_len %d do not fit %d tokens / a context of %d", b, q_off[b], q_len[b], kv_len[b], n_tok, ctx_max);
        max_p = q_len[b] > max_p ? q_len[b] : max_p;
    }
    if (!share.empty() && share.size() != (size_t)2 * B) return fail(e, SONIC_ERR_INVALID, "share_prompt.hook: armed for %zu sequences, the launch has %d", share.size() / 2, B);
    for (int b = 0; b < B && !share.empty(); ++b)
        if (share[b] < 0 || share[b] >= B || share[B + b] < 0 || share[B + b] > kv_len[b] - q_len[b])
            return fail(e, SONIC_ERR_INVALID, "share_prompt.hook: sequence %d: pre_row %d outside 0 .. %d or pre_len %d outside 0 .. kv_len - q_len = %d", b, share[b], B - 1, share[B + b], kv_len[b] - q_len[b]);
    TmpBuf tb(e->st);
    const size_t nq = (size_t)n_tok * Hq * hd, nc = (size_t)B * Hkv * ctx_max * hd;
    bf16_t* dq = up_bf16(e, tb, q, nq); bf16_t* dk = up_bf16(e, tb, kcache, nc); bf16_t* dvt = up_bf16(e, tb, vt, nc); bf16_t* dO = up_bf16(e, tb, out, nq);
    int* di = tb.get<int>((size_t)5 * B);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    HIPC(e, h2d(e, di, q_off, (size_t)B * 4)); HIPC(e, h2d(e, di + B, q_len, (size_t)B * 4)); HIPC(e, h2d(e, di + 2 * B, kv_len, (size_t)B * 4));
    if (!share.empty()) HIPC(e, h2d(e, di + 3 * B, share.data(), (size_t)2 * B * 4));
    launch_flash(prefill_flash_args(dq, dk, dvt, dO, di, di + B, di + 2 * B, Hq, Hkv, ctx_max, e->dt, share.empty() ? nullptr : di + 3 * B, di + 4 * B), hd, true, B, max_p, e->st);
    return down_bf16(e, tb, dO, out, nq);
}

extern "C" int sonic_test_layernorm(sonic_engine* e, const float* x, const float* w, const float* b, float* y, int rows, int d, float eps, int rms) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    if (d % 8 || d > 2048) return fail(e, SONIC_ERR_INVALID, "d must be a multiple of 8 and <= 2048");
    TmpBuf tb(e->st);
    bf16_t* dx = up_bf16(e, tb, x, (size_t)rows * d); float* dw = up_f32(e, tb, w, d); float* db = b ? up_f32(e, tb, b, d) : nullptr;
    bf16_t* dy = tb.get<bf16_t>((size_t)rows * d);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    if (rms) launch_rmsnorm(dx, dw, dy, rows, d, eps, nullptr, e->st, e->dt);
    else launch_layernorm(dx, dw, db, dy, rows, d, eps, e->st, e->dt);
    return down_bf16(e, tb, dy, y, (size_t)rows * d);
}

// `iters` launches between two events -> *ms for all of them.  g_opts goes back to the engine's own before the checks: sonic_bench_skinny runs a variant of its own
template <typename F> static int time_launches(sonic_engine* e, int iters, F launch, float* ms) {
    hipEvent_t ea, eb; HIPC(e, hipEventCreate(&ea)); HIPC(e, hipEventCreate(&eb));
    (void)hipEventRecord(ea, e->st);
    for (int i = 0; i < iters; ++i) launch(i);
    (void)hipEventRecord(eb, e->st);
    hipError_t r = stream_sync(e);
    *ms = 0; (void)hipEventElapsedTime(ms, ea, eb);
    (void)hipEventDestroy(ea); (void)hipEventDestroy(eb);
    g_opts = e->opts;
    HIPC(e, r); HIPC(e, hipGetLastError());
    return SONIC_OK;
}

extern "C" int sonic_bench_gemm(sonic_engine* e, int M, int N, int K, int epi, int iters, float* ms_per_launch) {
    if (!e || !ms_per_launch) return SONIC_ERR_INVALID;
    ENTER(e);
    if (K % 64 || N % 4 || iters < 1) return fail(e, SONIC_ERR_INVALID, "bad gemm bench shape");
    TmpBuf tb(e->st);
    const int Nout = (epi == EPI_SWIGLU) ? N / 2 : N;
    bf16_t* dA = tb.get<bf16_t>((size_t)M * K + 1024); bf16_t* dW = tb.get<bf16_t>((size_t)N * K); bf16_t* dC = tb.get<bf16_t>((size_t)M * Nout);
    float* db = tb.get<float>(N);
    bf16_t* dVt = nullptr;
    GemmArgs a{};
    if (epi == EPI_QKV_VT) {   // encoder QKV shape: last third of the columns is V, written transposed per 1500-frame segment
        if (N % 3 || M % 1500) return fail(e, SONIC_ERR_INVALID, "QKV bench needs N % 3 == 0 and M % 1500 == 0");
        dVt = tb.get<bf16_t>((size_t)(M / 1500) * (N / 3) * 1536);
        a.Vt = dVt; a.n_split = 2 * N / 3; a.seg_T = 1500; a.vt_ld = 1536; a.vt_seg_stride = (long)(N / 3) * 1536;
    }
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in gemm bench");
    // random (not zero) operands: zero data reads high on this chip (cdna_hip_programming.md rule 25)
    launch_synth_fill(0x1234, (long)M * K, 1.0f, 0.f, dA, nullptr, e->st);
    launch_synth_fill(0x5678, (long)N * K, 0.05f, 0.f, dW, nullptr, e->st);
    a.A = dA; a.lda = K; a.W = dW; a.C = dC; a.ldc = (epi == EPI_QKV_VT) ? 2 * N / 3 : Nout; a.bias = db; a.R = dC; a.ldr = Nout; a.M = M; a.N = N; a.K = K; a.batch = 1; a.dt = e->dt;
    a.gelu_lut = e->opt_no_gelu_lut ? nullptr : e->gelu_lut;          // as the encoder's fc1 (round 5: the bench used to time the arithmetic GELU)
    for (int i = 0; i < 2; ++i) launch_gemm(a, epi, e->st);
    if (e->opt_gemm_trace) {
        // diagnostics: where a 256x256 tile's time goes (in-kernel 100 MHz stamps of every block of ONE launch) and how long a CU waits between two blocks
        const int nblk = ((M + 255) / 256) * ((N + 255) / 256);
        long long* dbg = tb.get<long long>((size_t)nblk * 8);
        if (dbg) {
            (void)hipMemsetAsync(dbg, 0, (size_t)nblk * 64, e->st);
            GemmArgs t = a; t.dbg = dbg;
            launch_gemm(t, epi, e->st);
            std::vector<long long> h((size_t)nblk * 8);
            if (d2h(e, h.data(), dbg, (size_t)nblk * 64) == hipSuccess) {
                std::map<long long, std::vector<std::pair<long long, long long>>> per_cu;     // hw id -> (entry, exit)
                double s01 = 0, s12 = 0, s23 = 0; int n = 0;
                for (int b = 0; b < nblk; ++b) {
                    const long long* r = &h[(size_t)b * 8];
                    if (!r[0] || !r[3]) continue;
                    s01 += (r[1] - r[0]) * 0.01; s12 += (r[2] - r[1]) * 0.01; s23 += (r[3] - r[2]) * 0.01; ++n;
                    per_cu[r[4] & 0x0000000F0000FF00ll].push_back({r[0], r[3]});            // XCC_ID[3:0] | HW_ID: se_id[15:13] sh_id[12] cu_id[11:8]
                }
                double gap = 0; int ng = 0; long long t_first = 0, t_last = 0;
                for (auto& kv : per_cu) {
                    auto& v = kv.second; std::sort(v.begin(), v.end());
                    for (size_t i = 1; i < v.size(); ++i) { gap += (v[i].first - v[i - 1].second) * 0.01; ++ng; }
                    for (auto& x : v) { if (!t_first || x.first < t_first) t_first = x.first; if (x.second > t_last) t_last = x.second; }
                }
                fprintf(stderr, "[gemm_trace] M=%d N=%d K=%d epi=%d: %d blocks on %zu CUs; per block: entry -> first K tile landed %.2f us, K loop %.2f us, epilogue %.2f us; "
                                "gap between consecutive blocks of a CU %.2f us (n=%d); first entry -> last exit %.1f us\n",
                        M, N, K, epi, n, per_cu.size(), s01 / n, s12 / n, s23 / n, ng ? gap / ng : 0.0, ng, (t_last - t_first) * 0.01);
            }
        }
    }
    float ms;
    TRY(time_launches(e, iters, [&](int) { launch_gemm(a, epi, e->st); }, &ms));
    *ms_per_launch = ms / iters;
    return SONIC_OK;
}

extern "C" int sonic_bench_skinny(sonic_engine* e, int M, int N, int K, int variant, int iters, float* us_per_launch) {
    if (!e || !us_per_launch) return SONIC_ERR_INVALID;
    ENTER(e);
    if (M < 1 || M > 64 || N % 16 || K % 256 || skinny_pick_ksplit(N, K) < 1 || iters < 1) return fail(e, SONIC_ERR_INVALID, "bad skinny bench shape");
    TmpBuf tb(e->st);
    g_opts.skinny_variant = variant;   // this call only (ENTER() reloads the engine's own knobs on the next entry); before the ksplit pick: the slab count depends on the kernel family
    // 8 distinct weight copies so consecutive launches do not re-read an Infinity-Cache-resident matrix
    const int copies = 8;
    bf16_t* dW = tb.get<bf16_t>((size_t)copies * N * K); bf16_t* dX = tb.get<bf16_t>((size_t)64 * K);
    const int ks = skinny_pick_ksplit(N, K), mpad = ((M + 15) / 16) * 16;
    float* P = tb.get<float>((size_t)ks * mpad * N);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in skinny bench");
    launch_synth_fill(0x77, (long)copies * N * K, 0.05f, 0.f, dW, nullptr, e->st);
    launch_synth_fill(0x78, (long)64 * K, 1.0f, 0.f, dX, nullptr, e->st);
    SkinnyArgs a = skinny_args(dX, K, nullptr, P, M, N, K, ks, e->dt);
    for (int i = 0; i < copies; ++i) { a.W = dW + (size_t)(i % copies) * N * K; launch_skinny(a, e->st); }
    float ms;
    TRY(time_launches(e, iters, [&](int i) { a.W = dW + (size_t)(i % copies) * N * K; launch_skinny(a, e->st); }, &ms));
    *us_per_launch = ms * 1e3f / iters;
    return SONIC_OK;
}
// The engine's own quantisation scratch is sized for its model, not for a test: buffers of the test's shape (M rows of K, at most 64 groups) stand in for the call
struct I8Scratch {
    sonic_engine* e; int8_t* s_qa; float* s_sca; unsigned char* s_fl; int *s_occ, *s_ocl; int s_k;
    I8Scratch(sonic_engine* e_, TmpBuf& tb, int M, int K) : e(e_), s_qa(e_->qa), s_sca(e_->q_sca), s_fl(e_->q_flags), s_occ(e_->q_oc_cnt), s_ocl(e_->q_oc_list), s_k(e_->q_kmax) {
        e->qa = tb.get<int8_t>((size_t)M * K + 4096); e->q_sca = tb.get<float>(M);
        e->q_flags = tb.get<unsigned char>((size_t)64 * K + 64); e->q_oc_cnt = tb.get<int>(64); e->q_oc_list = tb.get<int>((size_t)64 * K); e->q_kmax = K;
    }
    ~I8Scratch() { e->qa = s_qa; e->q_sca = s_sca; e->q_flags = s_fl; e->q_oc_cnt = s_occ; e->q_oc_list = s_ocl; e->q_kmax = s_k; }
    I8Scratch(const I8Scratch&) = delete; I8Scratch& operator=(const I8Scratch&) = delete;
};
// W [N][K] (fp16) quantised row-wise on the device; tiled: only the fragment-tiled copy is handed on, as a decoder projection's since round 5
static QW i8_quant_weights(sonic_engine* e, TmpBuf& tb, const bf16_t* dW, int N, int K, bool tiled) {
    QW q;
    int8_t* cb = tb.get<int8_t>((size_t)N * K); q.scb = tb.get<float>(N);
    int8_t* cbt = tiled ? tb.get<int8_t>((size_t)N * K) : nullptr;
    if (tb.bad()) return q;
    launch_quant_weights(dW, cb, q.scb, N, K, e->st);
    if (tiled) { launch_tile_weights_i8(cb, cbt, N, K, e->st); q.cbt = cbt; q.cb_rowmajor_kept = false; }
    else q.cb = cb;
    return q;
}
// One Linear8bitLt (LLM.int8, threshold 6.0) through the engine's kernels: W [N][K] is quantised row-wise on the device, X [M][K] is
// cut into groups of `group_rows` rows (one group = one reference call: its outlier columns are found over its rows), then the int8
// MFMA GEMM with the dequantising epilogue `epi` (EPI_BIAS / _GELU / _RESID / _SWIGLU).  Inputs are fp32 holding fp16 values.
extern "C" int sonic_test_linear_int8(sonic_engine* e, const float* X, const float* W, const float* bias, const float* resid, float* out,
                                      int M, int N, int K, int group_rows, int epi) {
    if (!e || !X || !W || !out) return SONIC_ERR_INVALID;
    ENTER(e);
    if (!e->i8) return fail(e, SONIC_ERR_INVALID, "sonic_test_linear_int8 needs an engine created with mode int8");
    if (K % 128 || N % 16 || M < 1 || group_rows < 1 || (M + group_rows - 1) / group_rows > 64)
        return fail(e, SONIC_ERR_INVALID, "bad int8 linear test shape");
    TmpBuf tb(e->st);
    const int Nout = (epi == EPI_SWIGLU) ? N / 2 : N;
    bf16_t* dX = up_bf16(e, tb, X, (size_t)M * K); bf16_t* dW = up_bf16(e, tb, W, (size_t)N * K);
    float* db = bias ? up_f32(e, tb, bias, N) : nullptr;
    bf16_t* dR = resid ? up_bf16(e, tb, resid, (size_t)M * Nout) : nullptr;
    bf16_t* dC = tb.get<bf16_t>((size_t)M * Nout);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    I8Scratch sc(e, tb, M, K);
    const QW q = i8_quant_weights(e, tb, dW, N, K, false);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    qlinear(e, epi, dX, K, nullptr, q, db, dC, Nout, M, N, K, dR, Nout, QGroup{nullptr, group_rows, (M + group_rows - 1) / group_rows});
    return down_bf16(e, tb, dC, out, (size_t)M * Nout);
}

// One GEMM in a production launch form (include/sonic_hip.h has the record and the buffers): what sonic_test_gemm cannot express - pitched and overlapping rows, the
// batched conv-stem forms, the fragment-tiled weight copies, R == C, the q|k|v epilogue with its V^T and fused RoPE - on the engine's own type.
static int gemm_form_check(sonic_engine* e, const sonic_gemm_form& f, const float* resid, const float* rope, const float* Vt) {
    const char* bad = nullptr;
    const bool qkv = f.epi == EPI_QKV_VT;
    const int Nout = f.epi == EPI_SWIGLU ? f.N / 2 : qkv ? f.n_split : f.N;
    const int lda = f.lda ? f.lda : f.K, ldc = f.ldc ? f.ldc : Nout, ldr = f.ldr ? f.ldr : Nout, batch = f.batch > 0 ? f.batch : 1;
    if (f.size != (int32_t)sizeof(sonic_gemm_form)) bad = "size is not sizeof(sonic_gemm_form)";
    else if (e->f32) bad = "needs a 16-bit or int8 engine";
    else if (f.M < 1 || f.N < 16 || f.N % 16 || f.K < 64 || f.K % (e->i8 ? 128 : 64)) bad = "M >= 1, N a multiple of 16, K a multiple of 64 (int8: 128)";
    else if (f.epi < EPI_BIAS || f.epi > EPI_QKV_VT) bad = "epi is none of 0 .. 4";
    else if (f.epi == EPI_SWIGLU && f.N % 32) bad = "EPI_SWIGLU needs N % 32 == 0";
    else if (lda < 8 || lda % 8 || ldc < Nout || ldc % 4 || f.c_row_offset < 0) bad = "lda a multiple of 8, ldc >= the output width and a multiple of 4, c_row_offset >= 0";
    else if (f.batch < 0 || (batch > 1 && (f.strideA < 1 || f.strideC < (long)(f.c_row_offset + f.M) * ldc || f.strideA % 8 || f.strideC % 8))) bad = "batch > 1 needs strideA >= 1 and strideC >= (c_row_offset + M) * ldc, multiples of 8";
    else if (batch <= 1 && (f.strideA || f.strideC)) bad = "strideA / strideC without batch > 1";
    else if (batch > 1 && (f.epi == EPI_BIAS_RESID || qkv || e->i8)) bad = "batch > 1 with a residual, the q|k|v epilogue or an int8 engine";
    else if (f.gu8 && !(f.w_tiled && f.epi == EPI_SWIGLU)) bad = "gu8 without w_tiled and EPI_SWIGLU";
    else if (f.gu8 && e->i8) bad = "gu8 on an int8 engine";
    else if (f.gelu_arith && (f.epi != EPI_BIAS_GELU || e->i8)) bad = "gelu_arith without a 16-bit EPI_BIAS_GELU";
    else if (f.w_tiled && e->i8 && f.epi == EPI_BIAS_GELU) bad = "int8 EPI_BIAS_GELU from the tiled copy (gemm_lin compiles the tiled outlier gather out of the GELU epilogue: no decoder linear has one)";
    else if (f.epi == EPI_BIAS_RESID ? (f.resid_in_place ? resid != nullptr : resid == nullptr) : (f.resid_in_place || resid)) bad = "EPI_BIAS_RESID takes exactly one of resid and resid_in_place, the other epilogues neither";
    else if (f.epi == EPI_BIAS_RESID && !f.resid_in_place && (ldr < Nout || ldr % 4)) bad = "ldr >= N and a multiple of 4";
    else if (f.ldr && (f.epi != EPI_BIAS_RESID || f.resid_in_place)) bad = "ldr without a separate residual";
    else if (!qkv && (f.n_split || f.seg_T || f.vt_ld || f.rope_ncols || rope || Vt)) bad = "q|k|v fields without EPI_QKV_VT";
    else if (qkv && (!Vt || f.n_split < 128 || f.n_split % 128 || f.n_split >= f.N || f.seg_T < 4 || f.seg_T % 4 || f.M % 4 || f.vt_ld < f.seg_T || f.vt_ld % 8))
        bad = "EPI_QKV_VT needs Vt, 0 < n_split < N a multiple of 128, seg_T and M multiples of 4, vt_ld >= seg_T a multiple of 8";
    else if (qkv && (rope ? (f.rope_ncols < 64 || f.rope_ncols % 64 || f.rope_ncols > f.n_split) : f.rope_ncols != 0)) bad = "rope needs 64 <= rope_ncols <= n_split, a multiple of 64 (and rope_ncols needs rope)";
    else if (qkv && e->i8 && (!rope || f.ldc)) bad = "int8 q|k|v needs rope and the dense ldc";
    else if (e->i8 ? (f.group_rows < 0 || (f.M + (f.group_rows ? f.group_rows : f.M) - 1) / (f.group_rows ? f.group_rows : f.M) > 64) : f.group_rows != 0) bad = "group_rows: int8 engines only, at most 64 groups";
    return bad ? fail(e, SONIC_ERR_INVALID, "gemm.form.run: %s", bad) : SONIC_OK;
}
struct FormSizes { size_t a, c, vt, r; };
static FormSizes gemm_form_sizes(const sonic_engine* e, const sonic_gemm_form& f) {      // (of a record gemm_form_check accepts, but for the buffers it cannot see yet)
    const bool qkv = f.epi == EPI_QKV_VT;
    const int Nout = f.epi == EPI_SWIGLU ? f.N / 2 : qkv ? f.n_split : f.N, batch = f.batch > 0 ? f.batch : 1;
    const long lda = f.lda ? f.lda : f.K, ldr = f.ldr ? f.ldr : Nout, ldc = (qkv && e->i8) ? f.N : f.ldc ? f.ldc : Nout;
    FormSizes z;
    z.a = (size_t)(batch - 1) * f.strideA + (size_t)(f.M - 1) * lda + f.K;
    z.c = (size_t)f.c_row_offset * ldc + (size_t)(batch - 1) * f.strideC + (size_t)(f.M + 8) * ldc;
    z.vt = qkv ? (size_t)((f.M + f.seg_T - 1) / f.seg_T) * (f.N - f.n_split) * f.vt_ld : 0;
    z.r = (size_t)f.M * ldr;
    return z;
}
// the launch itself, under the caller's lock: buffers as the header lays them out, C and Vt in-out
static int gemm_form_launch(sonic_engine* e, const sonic_gemm_form& f, const float* A, const float* W, const float* bias, const float* resid, const float* rope,
                            float* C, float* Vt) {
    TRY(gemm_form_check(e, f, resid, rope, Vt));
    const int M = f.M, N = f.N, K = f.K, epi = f.epi, batch = f.batch > 0 ? f.batch : 1;
    const bool qkv = epi == EPI_QKV_VT;
    const int Nout = epi == EPI_SWIGLU ? N / 2 : qkv ? f.n_split : N;
    const long lda = f.lda ? f.lda : K, ldr = f.ldr ? f.ldr : Nout;
    long ldc = f.ldc ? f.ldc : Nout;
    if (qkv && e->i8) ldc = N;                               // room for the un-fused [M][N] form; the fused one is asked to write it at the pitch it then uses
    const size_t a_elems = (size_t)(batch - 1) * f.strideA + (size_t)(M - 1) * lda + K;
    const size_t c_elems = (size_t)f.c_row_offset * ldc + (size_t)(batch - 1) * f.strideC + (size_t)(M + 8) * ldc;
    const int n_seg = qkv ? (M + f.seg_T - 1) / f.seg_T : 0;
    const size_t vt_elems = qkv ? (size_t)n_seg * (N - f.n_split) * f.vt_ld : 0;
    TmpBuf tb(e->st);
    bf16_t* dA = up_bf16(e, tb, A, a_elems, 4096); bf16_t* dW = up_bf16(e, tb, W, (size_t)N * K);
    float* db = bias ? up_f32(e, tb, bias, N) : nullptr;
    bf16_t* dR = resid ? up_bf16(e, tb, resid, (size_t)M * ldr) : nullptr;
    bf16_t* dC = up_bf16(e, tb, C, c_elems);
    bf16_t* dVt = qkv ? up_bf16(e, tb, Vt, vt_elems) : nullptr;
    float* dcs = rope ? up_f32(e, tb, rope, (size_t)f.seg_T * 32) : nullptr;
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    bf16_t* c0 = dC + (size_t)f.c_row_offset * ldc;
    const bf16_t* R = f.resid_in_place ? c0 : dR;
    const long ldR = f.resid_in_place ? ldc : ldr;
    if (e->i8) {
        I8Scratch sc(e, tb, M, K);
        const QW q = i8_quant_weights(e, tb, dW, N, K, f.w_tiled != 0);
        if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
        const int gr = f.group_rows ? f.group_rows : M;
        const QGroup grp{nullptr, gr, (M + gr - 1) / gr};
        if (qkv) {
            const QkvVt vt{dVt, f.n_split, f.seg_T, f.vt_ld, (long)(N - f.n_split) * f.vt_ld};
            // as run_encoder: the linear is asked for [M][N] row-major; when the engine fuses, q | k land rotated in its first n_split columns and V in Vt
            qlinear(e, EPI_BIAS, dA, lda, nullptr, q, db, c0, ldc, M, N, K, nullptr, 0, grp, dcs, f.seg_T, f.rope_ncols, false, &vt);
        } else {
            qlinear(e, epi, dA, lda, nullptr, q, db, c0, ldc, M, N, K, R, ldR, grp);
        }
    } else {
        bf16_t* dWt = f.w_tiled ? tb.get<bf16_t>((size_t)N * K) : nullptr;
        if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
        if (f.gu8) launch_tile_weights_gu8(dW, dWt, N, K, e->st);
        else if (f.w_tiled) launch_tile_weights(dW, dWt, N, K, e->st);
        GemmArgs a{};
        a.A = dA; a.lda = lda; a.W = f.w_tiled ? dWt : dW; a.C = c0; a.ldc = ldc; a.bias = db; a.R = R; a.ldr = ldR; a.M = M; a.N = N; a.K = K; a.dt = e->dt;
        a.batch = batch; a.strideA = f.strideA; a.strideC = f.strideC;
        a.w_tiled = f.w_tiled != 0; a.gu8 = f.gu8 != 0;
        a.gelu_lut = (e->opt_no_gelu_lut || f.gelu_arith) ? nullptr : e->gelu_lut;      // (the conv stem launches without the table)
        if (qkv) {
            a.Vt = dVt; a.n_split = f.n_split; a.seg_T = f.seg_T; a.vt_ld = f.vt_ld; a.vt_seg_stride = (long)(N - f.n_split) * f.vt_ld;
            if (dcs && enc_qkv_fuses_rope(e, a)) { a.rope_cs = dcs; a.rope_T = f.seg_T; a.rope_ncols = f.rope_ncols; }
        }
        launch_gemm(a, epi, e->st);
    }
    TRY(down_bf16(e, tb, dC, C, c_elems));
    if (qkv) TRY(down_bf16(e, tb, dVt, Vt, vt_elems));
    return SONIC_OK;
}
// sonic_load_tensor "gemm.form:<buffer>": one of the hook's seven host buffers (fp32, ndim 1; shape {0} drops it)
static const char* const FORM_BUFS[7] = {"A", "W", "bias", "resid", "rope", "C", "Vt"};
int gemm_form_stage(sonic_engine* e, const char* which, const void* data, int dtype, const int64_t* shape, int ndim) {
    std::lock_guard<std::mutex> lk(e->mu);
    if (dtype != SONIC_DTYPE_F32 || ndim != 1 || shape[0] < 0) return fail(e, SONIC_ERR_INVALID, "gemm.form:%s: a buffer is one row of fp32 values (SONIC_DTYPE_F32, ndim 1)", which);
    for (int i = 0; i < 7; ++i)
        if (!strcmp(which, FORM_BUFS[i])) { e->hook_form[i].assign((const float*)data, (const float*)data + shape[0]); return SONIC_OK; }
    return fail(e, SONIC_ERR_INVALID, "gemm.form:%s: the buffers are A, W, bias, resid, rope, C, Vt", which);
}
// sonic_load_tensor "gemm.form.run": the record's words; the staged inputs are consumed whatever way the call leaves, C and Vt keep what the launch left
int gemm_form_run(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim) {
    ENTER(e);
    struct Drop { sonic_engine* e; ~Drop() { for (int i = 0; i < 5; ++i) std::vector<float>().swap(e->hook_form[i]); } } drop{e};
    sonic_gemm_form f;
    if (dtype != SONIC_DTYPE_I32 || ndim != 1 || shape[0] != (int64_t)(sizeof f / 4)) return fail(e, SONIC_ERR_INVALID, "gemm.form.run: the record is %d int32 words (SONIC_DTYPE_I32, ndim 1)", (int)(sizeof f / 4));
    memcpy(&f, data, sizeof f);
    std::vector<float>* b = e->hook_form;
    if (b[0].empty() || b[1].empty()) return fail(e, SONIC_ERR_INVALID, "gemm.form.run: stage A and W first (sonic_load_tensor \"gemm.form:A\", \"gemm.form:W\")");
    const bool qkv = f.epi == EPI_QKV_VT;
    TRY(gemm_form_check(e, f, b[3].empty() ? nullptr : b[3].data(), b[4].empty() ? nullptr : b[4].data(), b[6].empty() ? nullptr : b[6].data()));
    const FormSizes z = gemm_form_sizes(e, f);
    if (b[5].empty()) b[5].assign(z.c, 0.f);
    if (b[0].size() < z.a || b[1].size() != (size_t)f.N * f.K || (!b[2].empty() && b[2].size() != (size_t)f.N) || (!b[3].empty() && b[3].size() != z.r) ||
        (!b[4].empty() && b[4].size() != (size_t)f.seg_T * 32) || b[5].size() != z.c || b[6].size() != z.vt)
        return fail(e, SONIC_ERR_INVALID, "gemm.form.run: a staged buffer has another size than the record asks for (A >= %zu, W %zu, bias %d, resid %zu, rope %d, C %zu, Vt %zu)",
                    z.a, (size_t)f.N * f.K, f.N, z.r, f.seg_T * 32, z.c, z.vt);
    return gemm_form_launch(e, f, b[0].data(), b[1].data(), b[2].empty() ? nullptr : b[2].data(), b[3].empty() ? nullptr : b[3].data(), b[4].empty() ? nullptr : b[4].data(),
                            b[5].data(), qkv ? b[6].data() : nullptr);
}
// sonic_debug_read "gemm_form_c" / "gemm_form_vt" / "gemm_route" (under the caller's lock); returns -1 for any other name
int gemm_form_read(sonic_engine* e, const char* name, float* out, int64_t n) {
    if (!strcmp(name, "gemm_route")) {          // the calling thread's last launch_gemm (host only; exact in fp32: row counts below 2^24)
        if (n != 4 && n != 5) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        const GemmPlan p = g_last_gemm_plan;
        out[0] = (float)p.rows256; out[1] = (float)p.rows128; out[2] = (float)p.shape128; out[3] = (float)p.cus;
        if (n == 5) out[4] = (float)g_last_qlinear_defer;      // the last int8 linear of this thread armed the deferral (rows with long outlier lists left to the side product)
        return SONIC_OK;
    }
    const int i = !strcmp(name, "gemm_form_c") ? 5 : !strcmp(name, "gemm_form_vt") ? 6 : -1;
    if (i < 0) return -1;
    if (n < 0 || (size_t)n > e->hook_form[i].size()) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
    if (n > 0) memcpy(out, e->hook_form[i].data(), (size_t)n * 4);
    return SONIC_OK;
}

// greedy_kernel on caller-provided lm_head partial slabs [ksplit][mpad][V] (fp32): returns the token each row picks (first maximum of
// the bf16-rounded slab sum, HF:generation/utils.py:2925 / torch.argmax semantics) and, optionally, the bf16 logits it compared.
// sonic_test_greedy_lp: the same launch through greedy_kernel<T, true>, optionally under teacher forcing (force_ids[B]: the token every row emits
// instead of its argmax); lp_out[B] = the emitted token's log-probability.
// sonic_test_greedy_guard: the launch through greedy_kernel<T, LP, true> (LP when lp_out is given): row b's history is hist[b * hist_ld .. + hist_len[b]), the three
// parameters are sonic_set_generation's; logits_out stays the raw logits.
// With option top_logprobs = K on the handle the four hooks that take lp_out launch the TOPK kernel of their family and return row b's whole record at
// lp_out[b * (1 + 2K)]: the emitted token's log-probability, the K alternatives', their ids as fp32.
// sonic_test_greedy_bias: the launch through greedy_kernel<T, LP, true, true>: the guard test plus row b's table (sonic_set_request_bias's packed form, B requests).
struct GuardTest { const int32_t* hist; int hist_ld; const int32_t* hist_len; float penalty; int ngram; const int32_t* suppress; int n_suppress;
                   bool bias = false; const int32_t* seq_ids = nullptr; const int32_t* seq_off = nullptr; const float* seq_bias = nullptr; const int32_t* req_off = nullptr; };
// sonic_test_greedy_sample: the launch through greedy_kernel<T, true, GUARD, BIAS, true> in the handle's own type (bf16, fp16, the fp32 kind's float): row b draws at
// temperature[b] with seed[b] as its step[b]-th token (n_new = step: ids, log-probabilities and forced ids sit at that column); noise_out[B][V] = the Gumbel values used.
struct SampTest { const float* temperature; const uint64_t* seed; const int32_t* step; float* noise_out; };
// The grammar instantiations (greedy_kernel<T, true, true, BIAS, SAMPLE, TOPK, true>) ride on the guard / bias / sample hooks: an automaton armed on the
// handle (sonic_load_tensor "grammar.hook:<V>", validated against V as a grammar is against its model; options hook_grammar_state = row << 20 | state + 2 and
// hook_grammar_eos) is taken by the next launch that has histories and log-probabilities, in the handle's own type: row b enters at its state (-1: a free row, -2: it has
// left), eos: the ids a row at -2 may still emit (they also end a row, as the handle's do); the states out are read with sonic_debug_read "hook_grammar_state"
struct GramTest { const int32_t* state_in; const int32_t* eos; int n_eos; int32_t* state_out; };
// The language-model hooks (lm_step_kernel, lm.hip, and greedy_kernel<T, true, true, BIAS, SAMPLE, TOPK, false, ., true>).  sonic_load_tensor "lm.hook:<V>" arms an
// automaton, validated against V as a model's is against its vocabulary: every row at the start node, no token pending, weight 0; options hook_lm_state / hook_lm_tok /
// hook_lm_weight set the rows' words and the weight.  sonic_load_tensor "lm.hook.step" (one finished flag per row) launches lm_step_kernel alone over those rows; the
// states, pending tokens and vectors it left are read with sonic_debug_read "hook_lm_state" / "hook_lm_tok" / "hook_lm_add".  While a vector stands, the greedy hooks
// that have histories and log-probabilities and the vector's shape (V, at most its rows) launch their family's LM instantiation on it, in the handle's own type, and
// leave the emitted ids in the rows' pending tokens.  One launch takes the vector: the next one needs a step of its own.  Arming again (shape {0}: disarming) drops it
int lm_hook_arm(sonic_engine* e, int V, const int* words, int64_t n) {
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipGetLastError();
    HIPC(e, hipSetDevice(e->device));
    e->hook_lm_rows = 0; e->hook_lm_V = 0; e->hook_lm_N = 0;
    if (n == 0) { if (e->hook_lm) TRY(dfree(e, &e->hook_lm, e->hook_lm_cap)); e->hook_lm = nullptr; e->hook_lm_cap = 0; return SONIC_OK; }
    if (V < 4 || V % 4 || V > (1 << 24)) return fail(e, SONIC_ERR_INVALID, "lm.hook: vocabulary %d (a multiple of 4 in 4 .. 2^24)", V);
    TRY(lm_check("lm.hook", words, n, V));
    std::vector<int> w; lm_to_device_words(words, w);
    if (e->hook_lm && e->hook_lm_cap < w.size()) { TRY(dfree(e, &e->hook_lm, e->hook_lm_cap)); e->hook_lm = nullptr; }
    if (!e->hook_lm) { TRY(dalloc(e, &e->hook_lm, w.size(), false)); e->hook_lm_cap = w.size(); }
    if (!e->hook_lm_words) TRY(dalloc(e, &e->hook_lm_words, (size_t)128));
    HIPC(e, h2d(e, e->hook_lm, w.data(), w.size() * 4));
    HIPC(e, stream_sync(e));
    e->hook_lm_V = V; e->hook_lm_N = words[1]; e->hook_lm_weight = 0.f;
    for (int b = 0; b < 64; ++b) { e->hook_lm_in[b] = words[4]; e->hook_lm_in[64 + b] = -1; }
    return SONIC_OK;
}
int lm_hook_step(sonic_engine* e, const int* finished, int64_t B) {
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipGetLastError();
    HIPC(e, hipSetDevice(e->device));
    if (!e->hook_lm || !e->hook_lm_V) return fail(e, SONIC_ERR_INVALID, "lm.hook.step: arm a hook language model first (sonic_load_tensor \"lm.hook:<V>\")");
    if (B < 1 || B > 64) return fail(e, SONIC_ERR_INVALID, "lm.hook.step: %lld rows (1 .. 64)", (long long)B);
    const size_t need = (size_t)64 * e->hook_lm_V;
    if (e->hook_lm_add && e->hook_lm_add_cap < need) { TRY(dfree(e, &e->hook_lm_add, e->hook_lm_add_cap)); e->hook_lm_add = nullptr; }
    if (!e->hook_lm_add) { TRY(dalloc(e, &e->hook_lm_add, need)); e->hook_lm_add_cap = need; }
    TmpBuf tb(e->st);
    int* fin = tb.get<int>(64);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    HIPC(e, hipMemsetAsync(e->hook_lm_add, 0, (size_t)B * e->hook_lm_V * 4, e->st));      // (a finished row's vector reads as zeros: "nothing written")
    HIPC(e, h2d(e, fin, finished, (size_t)B * 4));
    HIPC(e, h2d(e, e->hook_lm_words, e->hook_lm_in, sizeof e->hook_lm_in));
    launch_lm_step(LmArgs{e->hook_lm, e->hook_lm_words, e->hook_lm_words + 64, fin, e->hook_lm_add, e->hook_lm_weight, (int)B}, e->st);
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    e->hook_lm_rows = (int)B;
    return SONIC_OK;
}
static int test_greedy(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* force_ids, int32_t* tok_out, float* logits_out, float* lp_out,
                       const GuardTest* gt = nullptr, const SampTest* sp = nullptr) {
    if (ksplit < 1 || ksplit > 8 || B < 1 || B > 64 || mpad < B || V < 4 || V % 4) return fail(e, SONIC_ERR_INVALID, "bad greedy test shape");
    if (force_ids) for (int b = 0; b < B; ++b) if (force_ids[b] < 0 || force_ids[b] >= V) return fail(e, SONIC_ERR_INVALID, "forced id %d out of vocabulary", force_ids[b]);
    const int lw_ = lp_out ? lp_width(e) : 1;                                     // floats of a token's log-probability record (option top_logprobs)
    int old = 1;                                                                  // columns of ids / lp / forced ids: one, or up to the largest step of a sampling test
    if (sp) {
        if (!sp->temperature || !sp->seed || !sp->step || !lp_out) return fail(e, SONIC_ERR_INVALID, "bad greedy sample test arguments");
        TRY(samp_check(e, "sonic_test_greedy_sample", sp->temperature, B));
        for (int b = 0; b < B; ++b) { if (sp->step[b] < 0 || sp->step[b] > 65535) return fail(e, SONIC_ERR_INVALID, "step %d outside 0 .. 65535", sp->step[b]); old = std::max(old, sp->step[b] + 1); }
    }
    std::vector<int> gblob; std::vector<int> geos;
    GramTest gtest{}; const GramTest* gr = nullptr;
    if (!e->hook_gram.empty() && gt && lp_out) {      // an armed hook grammar: this launch takes it
        gblob.swap(e->hook_gram); geos.swap(e->hook_eos);
        for (int k = 0; k < gblob[1]; ++k) if (gblob[GRAM_HEAD + gblob[0] + 1 + k] >= V) return fail(e, SONIC_ERR_INVALID, "hook grammar: token id %d does not fit this launch's vocabulary %d", gblob[GRAM_HEAD + gblob[0] + 1 + k], V);
        for (int id : geos) if (id >= V) return fail(e, SONIC_ERR_INVALID, "hook grammar: EOS id %d out of vocabulary", id);
        gtest = GramTest{e->hook_state_in, geos.data(), (int)geos.size(), e->hook_state_out};
        gr = &gtest;
    }
    const bool lmh = !gr && gt && lp_out && e->hook_lm_add && e->hook_lm_words && e->hook_lm_V == V && e->hook_lm_rows >= B;      // a standing hook vector of this shape: this launch takes it
    if (lmh) e->hook_lm_rows = 0;
    TmpBuf tb(e->st);
    const size_t n = (size_t)ksplit * mpad * V;
    float* dl = up_f32(e, tb, slabs, n);
    bf16_t* table = tb.get<bf16_t>((size_t)V * 8 * (sp || gr || lmh ? 2 : 1)); bf16_t* x = tb.get<bf16_t>((size_t)64 * 8 * (sp || gr || lmh ? 2 : 1));      // (sp, gr, lmh: rows of 8 floats in the fp32 kind)
    int* st = tb.get<int>(64 * 8 + 4); int* ids = tb.get<int>((size_t)64 * old);
    float* dump = logits_out ? tb.get<float>((size_t)B * V) : nullptr;
    float* lp = lp_out ? tb.get<float>((size_t)64 * old * lw_) : nullptr;
    int* fd = force_ids ? tb.get<int>((size_t)64 * old) : nullptr;
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    std::vector<int> h(64 * 8 + 4, 0);
    for (int b = 0; b < 64; ++b) { h[64 * 2 + b] = 1; h[64 * 4 + b] = 4; }       // kv_len = 1, max_new = 4
    h[64 * 8] = B;
    int *ghist = nullptr, *gsup = nullptr; int gld = 0;
    if (gt) {                                                                     // the history rows with room for the appended id; kv_len = the history's length
        if (gt->hist_ld < 0 || gt->hist_ld > (1 << 20) || !gt->hist_len || (gt->hist_ld > 0 && !gt->hist) || !(gt->penalty > 0.f) || !std::isfinite(gt->penalty) || gt->ngram < 0 || gt->ngram > 64 ||
            gt->n_suppress < 0 || gt->n_suppress > 256 || (gt->n_suppress > 0 && !gt->suppress) || greedy_guard_lds(V) > 60000)
            return fail(e, SONIC_ERR_INVALID, "bad greedy guard test arguments");
        gld = gt->hist_ld + 1;
        std::vector<int> hh((size_t)B * gld, 0);
        for (int b = 0; b < B; ++b) {
            if (gt->hist_len[b] < 0 || gt->hist_len[b] > gt->hist_ld) return fail(e, SONIC_ERR_INVALID, "history length %d outside 0 .. %d", gt->hist_len[b], gt->hist_ld);
            for (int j = 0; j < gt->hist_len[b]; ++j) {
                const int id = gt->hist[(size_t)b * gt->hist_ld + j];
                if (id < 0 || id >= V) return fail(e, SONIC_ERR_INVALID, "history id %d out of vocabulary", id);
                hh[(size_t)b * gld + j] = id;
            }
            h[64 * 2 + b] = gt->hist_len[b];
        }
        for (int i = 0; i < gt->n_suppress; ++i) if (gt->suppress[i] < 0 || gt->suppress[i] >= V) return fail(e, SONIC_ERR_INVALID, "suppressed id %d out of vocabulary", gt->suppress[i]);
        ghist = tb.get<int>(hh.size()); gsup = tb.get<int>(256);
        if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
        HIPC(e, h2d(e, ghist, hh.data(), hh.size() * 4));
        if (gt->n_suppress > 0) HIPC(e, h2d(e, gsup, gt->suppress, (size_t)gt->n_suppress * 4));
    }
    int* gbias = nullptr;
    if (gt && gt->bias) {
        if (!gt->req_off || gt->req_off[0] != 0 || greedy_guard_lds(V, true) > 60000) return fail(e, SONIC_ERR_INVALID, "bad greedy bias test arguments");
        std::vector<int> tab((size_t)BIAS_TAB_WORDS, 0);
        for (int b = 0; b < B; ++b) {
            const int a = gt->req_off[b], n = gt->req_off[b + 1] - a;
            if (n < 0) return fail(e, SONIC_ERR_INVALID, "bad greedy bias test arguments");
            if (n > 0 && (!gt->seq_off || !gt->seq_bias)) return fail(e, SONIC_ERR_INVALID, "bad greedy bias test arguments");
            if (n > 0) TRY(bias_pack(e, "sonic_test_greedy_bias", gt->seq_ids, gt->seq_off + a, gt->seq_bias + a, n, V, tab.data() + 64 + (size_t)b * BIAS_ROW_WORDS, &tab[b]));
        }
        gbias = tb.get<int>(tab.size());
        if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
        HIPC(e, h2d(e, gbias, tab.data(), tab.size() * 4));
    }
    unsigned* gsamp = nullptr; float* gnoise = nullptr;
    if (sp) {
        std::vector<unsigned> w((size_t)SAMP_WORDS, 0u);
        for (int b = 0; b < B; ++b) {
            samp_pack(&w[3 * b], sp->temperature[b], sp->seed[b]);
            h[b] = sp->step[b]; h[64 * 4 + b] = sp->step[b] + 4;                 // n_new = step, max_new beyond it
        }
        gsamp = tb.get<unsigned>(w.size());
        if (sp->noise_out) gnoise = tb.get<float>((size_t)B * V);
        if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
        HIPC(e, h2d(e, gsamp, w.data(), w.size() * 4));
    }
    unsigned* gtrunc = nullptr;                                                   // an armed hook truncation (sonic_load_tensor "truncation.hook"): this sampling launch takes it
    if (sp && !e->hook_trunc.empty()) {
        std::vector<unsigned> w; w.swap(e->hook_trunc);
        if (greedy_guard_lds(V, gt && gt->bias) + greedy_trunc_lds() > 60000) return fail(e, SONIC_ERR_INVALID, "truncation.hook: a vocabulary of %d ids does not fit the select's histogram beside the bitmaps", V);
        gtrunc = tb.get<unsigned>(2 * (size_t)TRUNC_STAGE_WORDS);                 // the rows' words, then their records
        if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
        HIPC(e, h2d(e, gtrunc, w.data(), w.size() * 4));
    }
    int* gdev = nullptr; unsigned long long* gref = nullptr;
    if (gr) {
        gdev = tb.get<int>(gblob.size()); gref = tb.get<unsigned long long>(GRAM_STAGE_WORDS);
        if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
        std::vector<unsigned long long> w((size_t)GRAM_STAGE_WORDS, 0ull);
        int* stw = (int*)(w.data() + 64);
        for (int b = 0; b < 64; ++b) { w[b] = b < B && gr->state_in[b] != -1 ? (unsigned long long)(uintptr_t)gdev : 0ull; stw[b] = b < B ? gr->state_in[b] : -1; }
        HIPC(e, h2d(e, gdev, gblob.data(), gblob.size() * 4));
        HIPC(e, h2d(e, gref, w.data(), w.size() * 8));
    }
    HIPC(e, h2d(e, st, h.data(), h.size() * 4));
    if (fd && !sp) HIPC(e, h2d(e, fd, force_ids, (size_t)B * 4));
    if (fd && sp) {
        std::vector<int> fw((size_t)64 * old, 0);
        for (int b = 0; b < B; ++b) fw[(size_t)b * old + sp->step[b]] = force_ids[b];
        HIPC(e, h2d(e, fd, fw.data(), fw.size() * 4));
    }
    GreedyArgs g{};
    g.logits = dl; g.ksplit = ksplit; g.mpad = mpad; g.V = V; g.B = B; g.table = table; g.x = x; g.d = 8;
    g.out_ids = ids; g.out_ld = old; g.n_new = st; g.finished = st + 64; g.kv_len = st + 128; g.tok_pos = st + 192; g.max_new = st + 256;
    g.n_active = st + 512; g.n_eos = 0; g.pad_id = 0; g.logits_dump = dump; g.dump_stride_step = (long)B * V; g.step_counter = dump ? st + 320 : nullptr;
    g.out_lp = lp; g.force_ids = fd; g.force_ld = old; g.topk = lp ? e->opt_top_logprobs : 0;
    if (sp) { g.samp = gsamp; g.noise_out = gnoise; g.dt = e->f32 ? DT_F32 : e->dt; }
    if (gtrunc) { g.trunc = gtrunc; g.trunc_rec = gtrunc + TRUNC_STAGE_WORDS; }
    if (gt) { g.hist = ghist; g.hist_ld = gld; g.rep_penalty = gt->penalty; g.ngram = gt->ngram; g.suppress = gsup; g.n_suppress = gt->n_suppress; g.bias_tab = gbias; }
    if (gr) { g.gram_ref = gref; g.gram_state = (int*)(gref + 64); g.n_eos = gr->n_eos; for (int i = 0; i < gr->n_eos; ++i) g.eos[i] = gr->eos[i]; g.dt = e->f32 ? DT_F32 : e->dt; }
    if (lmh) { g.lm_add = e->hook_lm_add; g.lm_tok = e->hook_lm_words + 64; g.dt = e->f32 ? DT_F32 : e->dt; }
    launch_greedy(g, e->st);
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    if (gtrunc) HIPC(e, d2h(e, e->hook_trunc_rec, gtrunc + TRUNC_STAGE_WORDS, (size_t)B * 3 * 4));
    if (gr) {
        std::vector<unsigned long long> w((size_t)GRAM_STAGE_WORDS);
        HIPC(e, d2h(e, w.data(), gref, w.size() * 8));
        memcpy(gr->state_out, w.data() + 64, (size_t)B * 4);
    }
    std::vector<int> out((size_t)64 * old);
    HIPC(e, d2h(e, out.data(), ids, out.size() * 4));
    for (int b = 0; b < B; ++b) tok_out[b] = out[(size_t)b * old + (sp ? sp->step[b] : 0)];
    if (logits_out) HIPC(e, d2h(e, logits_out, dump, (size_t)B * V * 4));
    if (lp_out && !sp) HIPC(e, d2h(e, lp_out, lp, (size_t)B * lw_ * 4));
    if (sp) {
        std::vector<float> lw((size_t)64 * old * lw_);
        HIPC(e, d2h(e, lw.data(), lp, lw.size() * 4));
        for (int b = 0; b < B; ++b) memcpy(lp_out + (size_t)b * lw_, &lw[((size_t)b * old + sp->step[b]) * lw_], (size_t)lw_ * 4);
        if (sp->noise_out) HIPC(e, d2h(e, sp->noise_out, gnoise, (size_t)B * V * 4));
    }
    return SONIC_OK;
}
// The frame of the two hooks that send their rows to rows_kernel (rows.hip) instead of the greedy kernel.  The slabs are summed over ksplit in the greedy kernel's order
// and rounded to the handle's element type: those values are the logits row the kernel reads, and logits_out returns them.  B may exceed 64 on these routes (one block
// per row); mpad stays the slab row stride.  rows_check: the shape (the hook's own words), the hook's own refusal, the forced ids.  rows_run: `plan` = the rows'
// B-word arrays, target | rec and, with `choose`, | hrow | hlen; `hist` (choose only; may be empty) and gt's suppress list go up beside it; tok_out = out_ids
// (the forced ids), or with `choose` the kernel's choices; lp_out (optional) = B records of 1 + 2K floats
static int rows_check(sonic_engine* e, const char* shape_msg, const char* refusal, int ksplit, int mpad, int V, int B, const int32_t* force_ids) {
    if (ksplit < 1 || ksplit > 8 || B < 1 || B > 4096 || mpad < B || V < 4 || V % 4 || V > (1 << 24)) return fail(e, SONIC_ERR_INVALID, "%s", shape_msg);
    if (refusal) return fail(e, SONIC_ERR_INVALID, "%s", refusal);
    for (int b = 0; b < B; ++b) if (force_ids[b] < 0 || force_ids[b] >= V) return fail(e, SONIC_ERR_INVALID, "forced id %d out of vocabulary", force_ids[b]);
    return SONIC_OK;
}
static int rows_run(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, int dt, int K, const std::vector<int>& plan, bool choose, const std::vector<int>& hist,
                    const GuardTest* gt, int32_t* tok_out, float* logits_out, float* lp_out) {
    const int W = 1 + 2 * K;
    TmpBuf tb(e->st);
    float* dl = up_f32(e, tb, slabs, (size_t)ksplit * mpad * V);
    unsigned char* rows = tb.get<unsigned char>((size_t)B * V * (dt == DT_F32 ? 4 : 2));
    int* dplan = tb.get<int>(plan.size()); int* dh = tb.get<int>(hist.size()); int* gsup = tb.get<int>(256); int* tok = tb.get<int>(B);
    float* lp = tb.get<float>((size_t)B * W); float* dump = logits_out ? tb.get<float>((size_t)B * V) : nullptr;
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    HIPC(e, h2d(e, dplan, plan.data(), plan.size() * 4));
    if (!hist.empty()) HIPC(e, h2d(e, dh, hist.data(), hist.size() * 4));
    if (gt && gt->n_suppress > 0) HIPC(e, h2d(e, gsup, gt->suppress, (size_t)gt->n_suppress * 4));
    launch_score_slab_rows(dl, ksplit, mpad, V, B, rows, dt, e->st);
    RowsArgs a{};
    a.logits = rows; a.ld = V; a.V = V; a.n = B; a.dt = dt; a.target = dplan; a.rec = dplan + B; a.out_lp = lp; a.topk = K; a.dump = dump; a.out_ld = 1; a.R = B;
    if (choose) { a.choice = tok; a.lp_by_row = true; a.hrow = dplan + 2 * B; a.hlen = dplan + 3 * B; } else a.out_ids = tok;
    if (gt) { a.hist = dh; a.hist_ld = std::max(gt->hist_ld, 1); a.rep_penalty = gt->penalty; a.ngram = gt->ngram; a.suppress = gsup; a.n_suppress = gt->n_suppress; }
    launch_rows(a, e->st);
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    HIPC(e, d2h(e, tok_out, tok, (size_t)B * 4));
    if (logits_out) HIPC(e, d2h(e, logits_out, dump, (size_t)B * V * 4));
    if (lp_out) HIPC(e, d2h(e, lp_out, lp, (size_t)B * W * 4));
    return SONIC_OK;
}
// sonic_test_greedy_lp on a handle with option forced_parallel on: rows_kernel<T, false, ...>.  force_ids is required; tok_out holds the forced ids
static int test_score(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* force_ids, int32_t* tok_out, float* logits_out, float* lp_out) {
    TRY(rows_check(e, "bad score test shape", force_ids ? nullptr : "forced_parallel: the score rows need their forced ids", ksplit, mpad, V, B, force_ids));
    std::vector<int> plan((size_t)2 * B);
    for (int b = 0; b < B; ++b) { plan[b] = force_ids[b]; plan[B + b] = b; }      // record b = sequence b, token 0 (out_ld = 1)
    return rows_run(e, slabs, ksplit, mpad, V, B, e->f32 ? DT_F32 : e->dt, e->opt_top_logprobs, plan, false, {}, nullptr, tok_out, logits_out, lp_out);
}
// sonic_test_greedy_guard with forced ids on a handle with option draft_verify on: rows_kernel<T, true, ...>.  Row b is one draft position: its
// history is hist[b * hist_ld .. + hist_len[b]), its draft id force_ids[b]; tok_out[b] = the kernel's choice (the first maximum of the processed scores),
// lp_out[b * (1 + 2K) ..] = the record of force_ids[b].  Neutral parameters and no history launch the unguarded instantiation
static int test_verify(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const GuardTest& gt, const int32_t* force_ids, int32_t* tok_out, float* logits_out, float* lp_out) {
    TRY(rows_check(e, "bad verify test shape", e->f32 ? "draft_verify: the fp32 kind has no verify kernels" : nullptr, ksplit, mpad, V, B, force_ids));
    if (gt.hist_ld < 0 || gt.hist_ld > (1 << 20) || (gt.hist_ld > 0 && !gt.hist) || !(gt.penalty > 0.f) || !std::isfinite(gt.penalty) || gt.ngram < 0 || gt.ngram > 64 ||
        gt.n_suppress < 0 || gt.n_suppress > 256 || (gt.n_suppress > 0 && !gt.suppress) || greedy_guard_lds(V) > 60000)
        return fail(e, SONIC_ERR_INVALID, "bad greedy guard test arguments");
    const int ld = std::max(gt.hist_ld, 1);
    std::vector<int> hh((size_t)B * ld, 0), plan((size_t)4 * B);
    const bool guard = gt.penalty != 1.0f || gt.ngram > 0 || gt.n_suppress > 0;
    for (int b = 0; b < B; ++b) {
        if (gt.hist_len[b] < 0 || gt.hist_len[b] > gt.hist_ld) return fail(e, SONIC_ERR_INVALID, "history length %d outside 0 .. %d", gt.hist_len[b], gt.hist_ld);
        for (int j = 0; j < gt.hist_len[b]; ++j) {
            const int id = gt.hist[(size_t)b * gt.hist_ld + j];
            if (id < 0 || id >= V) return fail(e, SONIC_ERR_INVALID, "history id %d out of vocabulary", id);
            hh[(size_t)b * ld + j] = id;
        }
        plan[b] = force_ids[b]; plan[B + b] = b; plan[2 * B + b] = b; plan[3 * B + b] = gt.hist_len[b];      // record b = sequence b, token 0 (out_ld = 1)
    }
    for (int i = 0; i < gt.n_suppress; ++i) if (gt.suppress[i] < 0 || gt.suppress[i] >= V) return fail(e, SONIC_ERR_INVALID, "suppressed id %d out of vocabulary", gt.suppress[i]);
    return rows_run(e, slabs, ksplit, mpad, V, B, e->dt, lp_out ? e->opt_top_logprobs : 0, plan, true, hh, guard ? &gt : nullptr, tok_out, logits_out, lp_out);
}
extern "C" int sonic_test_greedy(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, int32_t* tok_out, float* logits_out) {
    if (!e || !slabs || !tok_out) return SONIC_ERR_INVALID;
    ENTER(e);
    return test_greedy(e, slabs, ksplit, mpad, V, B, nullptr, tok_out, logits_out, nullptr);
}
extern "C" int sonic_test_greedy_lp(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* force_ids, int32_t* tok_out,
                                    float* logits_out, float* lp_out) {
    if (!e || !slabs || !tok_out || !lp_out) return SONIC_ERR_INVALID;
    ENTER(e);
    if (e->opt_forced_parallel) return test_score(e, slabs, ksplit, mpad, V, B, force_ids, tok_out, logits_out, lp_out);
    return test_greedy(e, slabs, ksplit, mpad, V, B, force_ids, tok_out, logits_out, lp_out);
}

extern "C" int sonic_test_greedy_guard(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* hist, int hist_ld, const int32_t* hist_len,
                                       float repetition_penalty, int no_repeat_ngram_size, const int32_t* suppress, int n_suppress, const int32_t* force_ids,
                                       int32_t* tok_out, float* logits_out, float* lp_out) {
    if (!e || !slabs || !tok_out || !hist_len) return SONIC_ERR_INVALID;
    ENTER(e);
    const GuardTest gt{hist, hist_ld, hist_len, repetition_penalty, no_repeat_ngram_size, suppress, n_suppress};
    if (e->opt_draft_verify && force_ids) return test_verify(e, slabs, ksplit, mpad, V, B, gt, force_ids, tok_out, logits_out, lp_out);
    return test_greedy(e, slabs, ksplit, mpad, V, B, force_ids, tok_out, logits_out, lp_out, &gt);
}

extern "C" int sonic_test_greedy_bias(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* hist, int hist_ld, const int32_t* hist_len,
                                      float repetition_penalty, int no_repeat_ngram_size, const int32_t* suppress, int n_suppress, const int32_t* force_ids,
                                      const int32_t* seq_ids, const int32_t* seq_off, const float* bias, const int32_t* req_off,
                                      int32_t* tok_out, float* logits_out, float* lp_out) {
    if (!e || !slabs || !tok_out || !hist_len || !req_off) return SONIC_ERR_INVALID;
    ENTER(e);
    const GuardTest gt{hist, hist_ld, hist_len, repetition_penalty, no_repeat_ngram_size, suppress, n_suppress, req_off != nullptr, seq_ids, seq_off, bias, req_off};      // tables: a bias test
    return test_greedy(e, slabs, ksplit, mpad, V, B, force_ids, tok_out, logits_out, lp_out, &gt);
}

// hist_len = NULL: greedy_kernel<T, true, false, false, true>; hist_len without req_off: <T, true, true, false, true>; both: <T, true, true, true, true>
extern "C" int sonic_test_greedy_sample(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* hist, int hist_ld, const int32_t* hist_len,
                                        float repetition_penalty, int no_repeat_ngram_size, const int32_t* suppress, int n_suppress, const int32_t* force_ids,
                                        const int32_t* seq_ids, const int32_t* seq_off, const float* bias, const int32_t* req_off,
                                        const float* temperature, const uint64_t* seed, const int32_t* step,
                                        int32_t* tok_out, float* logits_out, float* lp_out, float* noise_out) {
    if (!e || !slabs || !tok_out || !lp_out || !temperature || !seed || !step) return SONIC_ERR_INVALID;
    ENTER(e);
    if (req_off && !hist_len) return fail(e, SONIC_ERR_INVALID, "sonic_test_greedy_sample: tables need the histories");
    const SampTest sp{temperature, seed, step, noise_out};
    if (!hist_len) return test_greedy(e, slabs, ksplit, mpad, V, B, force_ids, tok_out, logits_out, lp_out, nullptr, &sp);
    const GuardTest gt{hist, hist_ld, hist_len, repetition_penalty, no_repeat_ngram_size, suppress, n_suppress, req_off != nullptr, seq_ids, seq_off, bias, req_off};      // tables: a bias test
    return test_greedy(e, slabs, ksplit, mpad, V, B, force_ids, tok_out, logits_out, lp_out, &gt, &sp);
}

extern "C" int sonic_test_skinny_gu(sonic_engine* e, const float* X, const float* Wgu_interleaved, float* act, int M, int N, int K) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    if (!skinny_gu_eligible(M, N, K)) return fail(e, SONIC_ERR_INVALID, "shape not handled by the fused gate/up kernel");
    TmpBuf tb(e->st);
    bf16_t* dX = up_bf16(e, tb, X, (size_t)M * K); bf16_t* dW = up_bf16(e, tb, Wgu_interleaved, (size_t)N * K);
    bf16_t* dWt = tb.get<bf16_t>((size_t)N * K); bf16_t* dA = tb.get<bf16_t>((size_t)M * (N / 2));
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    launch_tile_weights_gu8(dW, dWt, N, K, e->st);
    launch_skinny_gu(skinny_args(dX, K, dWt, nullptr, M, N, K, 1, e->dt), dA, e->st);
    return down_bf16(e, tb, dA, act, (size_t)M * (N / 2));
}

// ------------------------------------------------------------------------------------------ decode-step and prefill glue kernels, one launch each
// (tests/test_gpu_decode_glue.py; the references with the kernels' rounding points are in tests/glue_ref.py).  Every hook checks every shape and index
// before its first launch and refuses what the kernel behind it does not handle.
static int glue_16bit(sonic_engine* e, const char* what) { return e->f32 ? fail(e, SONIC_ERR_INVALID, "%s needs a 16-bit engine", what) : SONIC_OK; }
// the five outputs of quant_emit_row for `rows` rows of width K: the lists are pre-filled with -1 so that entries the kernel leaves alone show
struct QuantHost { int8_t* q; float* sca; int32_t* oc_cnt; int32_t* oc_list; float* oc_val; };
static int quant_alloc(sonic_engine* e, TmpBuf& tb, int rows, int K, QuantOut* qo) {
    qo->q = tb.get<int8_t>((size_t)rows * K); qo->ldq = K; qo->sca = tb.get<float>(rows); qo->oc_cnt = tb.get<int>(rows);
    qo->oc_list = tb.get<int>((size_t)rows * K); qo->oc_ld = K; qo->oc_val = tb.get<float>((size_t)rows * K);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    fill_words(qo->oc_list, -1, (size_t)rows * K, e->st);
    return SONIC_OK;
}
static int quant_fetch(sonic_engine* e, const QuantOut& qo, int rows, int K, const QuantHost& h) {
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    HIPC(e, d2h(e, h.q, qo.q, (size_t)rows * K)); HIPC(e, d2h(e, h.sca, qo.sca, (size_t)rows * 4)); HIPC(e, d2h(e, h.oc_cnt, qo.oc_cnt, (size_t)rows * 4));
    HIPC(e, d2h(e, h.oc_list, qo.oc_list, (size_t)rows * K * 4)); HIPC(e, d2h(e, h.oc_val, qo.oc_val, (size_t)rows * K * 4));
    return SONIC_OK;
}

// add_rmsnorm_kernel as decode_step() launches it behind o_proj / down_proj: x[r] += sum of the slabs, y[r] = RMSNorm(x[r]) * w for r < rows.  x and y are
// [rows_alloc][d] and both are uploaded first, so rows the kernel leaves alone come back as they went in.  q_out != NULL (fp16 engine): the launch also gets a
// QuantOut (quant_emit_row<true>, DeqInfo off) and the five outputs come back: q [rows][d], sca / oc_cnt [rows], oc_list / oc_val [rows][d] (-1 / 0 where unwritten).
extern "C" int sonic_test_add_rmsnorm(sonic_engine* e, float* x, const float* slabs, int ksplit, int mpad, const float* w, float eps, float* y, int rows, int rows_alloc, int d,
                                      int8_t* q_out, float* sca_out, int32_t* oc_cnt_out, int32_t* oc_list_out, float* oc_val_out) {
    if (!e || !x || !slabs || !w || !y) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(glue_16bit(e, "sonic_test_add_rmsnorm"));
    if (d < 8 || d % 8 || d > 2048 || ksplit < 1 || ksplit > 8 || rows < 1 || rows > 4096 || rows_alloc < rows || rows_alloc > 8192 || mpad < rows || mpad > 8192)
        return fail(e, SONIC_ERR_INVALID, "add_rmsnorm: d %% 8 == 0, d <= 2048, 1 <= ksplit <= 8, 1 <= rows <= rows_alloc, mpad >= rows");
    if (q_out && (e->dt != DT_F16 || !sca_out || !oc_cnt_out || !oc_list_out || !oc_val_out))
        return fail(e, SONIC_ERR_INVALID, "add_rmsnorm: the quantised outputs need an fp16 engine and all five buffers");
    TmpBuf tb(e->st);
    const size_t n = (size_t)rows_alloc * d;
    bf16_t* dx = up_bf16(e, tb, x, n); bf16_t* dy = up_bf16(e, tb, y, n);
    float* dP = up_f32(e, tb, slabs, (size_t)ksplit * mpad * d); float* dw = up_f32(e, tb, w, d);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    QuantOut qo{};
    if (q_out) TRY(quant_alloc(e, tb, rows, d, &qo));
    launch_add_rmsnorm(dx, dP, ksplit, mpad, dw, dy, rows, d, eps, e->st, e->dt, nullptr, q_out ? &qo : nullptr);
    TRY(down_bf16(e, tb, dx, x, n));
    TRY(down_bf16(e, tb, dy, y, n));
    if (q_out) TRY(quant_fetch(e, qo, rows, d, QuantHost{q_out, sca_out, oc_cnt_out, oc_list_out, oc_val_out}));
    return SONIC_OK;
}

// quant_rows_kernel (launch_quant_rows, the decode flavour of the activation quantiser): X [M][ld] fp16 values, the first K of every row are quantised
extern "C" int sonic_test_quant_rows(sonic_engine* e, const float* X, int M, int K, int ld, int8_t* q_out, float* sca_out, int32_t* oc_cnt_out, int32_t* oc_list_out, float* oc_val_out) {
    if (!e || !X || !q_out || !sca_out || !oc_cnt_out || !oc_list_out || !oc_val_out) return SONIC_ERR_INVALID;
    ENTER(e);
    if (e->f32 || e->dt != DT_F16) return fail(e, SONIC_ERR_INVALID, "sonic_test_quant_rows needs an fp16 engine");
    if (M < 1 || M > 4096 || K < 8 || K % 8 || K > 8192 || ld < K || ld % 8 || ld > (1 << 20))
        return fail(e, SONIC_ERR_INVALID, "quant_rows: 1 <= M <= 4096, K %% 8 == 0, K <= 8192, ld >= K, ld %% 8 == 0");
    TmpBuf tb(e->st);
    bf16_t* dX = up_bf16(e, tb, X, (size_t)M * ld);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    QuantOut qo{};
    TRY(quant_alloc(e, tb, M, K, &qo));
    launch_quant_rows(dX, ld, M, K, qo, e->st);
    return quant_fetch(e, qo, M, K, QuantHost{q_out, sca_out, oc_cnt_out, oc_list_out, oc_val_out});
}

// swiglu_slab_kernel: slabs [ksplit][mpad][2 ff] fp32 with gate / up columns interleaved in groups of 16 (gu8 = 0) or 8 (gu8 = 1) -> act [rows][ff]
extern "C" int sonic_test_swiglu_slab(sonic_engine* e, const float* slabs, int ksplit, int mpad, int ff, int rows, int gu8, float* act) {
    if (!e || !slabs || !act) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(glue_16bit(e, "sonic_test_swiglu_slab"));
    if (ff < 16 || ff % 16 || ff > (1 << 16) || ksplit < 1 || ksplit > 8 || rows < 1 || rows > 4096 || mpad < rows || mpad > 8192 || (gu8 != 0 && gu8 != 1))
        return fail(e, SONIC_ERR_INVALID, "swiglu_slab: ff %% 16 == 0, 1 <= ksplit <= 8, 1 <= rows <= mpad, gu8 0 or 1");
    TmpBuf tb(e->st);
    float* dP = up_f32(e, tb, slabs, (size_t)ksplit * mpad * 2 * ff); bf16_t* dA = tb.get<bf16_t>((size_t)rows * ff);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    launch_swiglu_slab(dP, ksplit, mpad, 2 * ff, dA, rows, e->st, e->dt, gu8);
    return down_bf16(e, tb, dA, act, (size_t)rows * ff);
}

// The o_proj -> RMSNorm -> gate/up chain of one decoder layer through launch_o_gu, the function decode_step() launches it with (form = OGU_FUSED / _SPLIT_NORM /
// _HALF_FUSED).  att [M][K], Wo [D][K], resid [rows_alloc][D] (in place: rows >= M must come back untouched), ln_w [D], Wgu [2 ff][D] with gate / up rows
// interleaved in groups of 16 (as for sonic_test_skinny_gu).
//   form 0: launch_skinny_o + launch_skinny_gu_norm                          (the default step)
//   form 1: launch_skinny_o + launch_rmsnorm_ss + launch_skinny_gu           (the continuous loops' split form; hn_out [M][D])
//   form 2: launch_skinny into slabs + launch_add_rmsnorm + launch_skinny_gu (fused gate/up behind an unfused o_proj; hn_out [M][D])
// act_out [M][ff]; ss_out (optional, forms 0 / 1): the raw sum-of-squares partials [2 regions][D / 64][32 rows][4].
// rmsnorm_ss_kernel splits a row's D / 64 partial groups into two halves and is launched with D / 8 <= 256 threads: form 1 needs D % 128 == 0 and D <= 2048.
extern "C" int sonic_test_decode_o_gu(sonic_engine* e, const float* att, const float* Wo, float* resid, const float* ln_w, float eps, const float* Wgu, int form,
                                      int M, int K, int D, int ff, int rows_alloc, float* hn_out, float* act_out, float* ss_out) {
    if (!e || !att || !Wo || !resid || !ln_w || !Wgu || !act_out) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(glue_16bit(e, "sonic_test_decode_o_gu"));
    if (form < 0 || form > 2 || M < 1 || M > 64 || rows_alloc < M || rows_alloc > 4096 || ff < 16 || ff > (1 << 16) || D % 64 || D > 2048)
        return fail(e, SONIC_ERR_INVALID, "decode_o_gu: form 0..2, 1 <= M <= 64, rows_alloc >= M, D %% 64 == 0, D <= 2048");
    if (!skinny_gu_eligible(M, 2 * ff, D)) return fail(e, SONIC_ERR_INVALID, "decode_o_gu: gate/up shape not handled by the fused gate/up kernel");
    if (form < 2 && !skinny_o_eligible(M, D, K)) return fail(e, SONIC_ERR_INVALID, "decode_o_gu: o_proj shape not handled by the fused o_proj kernel");
    if (form == 1 && D % 128) return fail(e, SONIC_ERR_INVALID, "decode_o_gu: the split norm needs D %% 128 == 0");
    if (form == 2 && (D % 16 || K % 256 || K < 256 || skinny_pick_ksplit(D, K) < 1 || skinny_pick_ksplit(D, K) > 8)) return fail(e, SONIC_ERR_INVALID, "decode_o_gu: o_proj shape not handled by the skinny GEMM");
    if (form != 0 && !hn_out) return fail(e, SONIC_ERR_INVALID, "decode_o_gu: forms 1 and 2 return hn_out");
    if (form == 2 && ss_out) return fail(e, SONIC_ERR_INVALID, "decode_o_gu: the unfused form has no sum-of-squares partials");
    TmpBuf tb(e->st);
    const size_t nss = (size_t)2 * (D / 64) * 32 * 4;
    bf16_t* dA = up_bf16(e, tb, att, (size_t)M * K); bf16_t* dWo = up_bf16(e, tb, Wo, (size_t)D * K); bf16_t* dWot = tb.get<bf16_t>((size_t)D * K);
    bf16_t* dR = up_bf16(e, tb, resid, (size_t)rows_alloc * D); float* dw = up_f32(e, tb, ln_w, D);
    bf16_t* dWg = up_bf16(e, tb, Wgu, (size_t)2 * ff * D); bf16_t* dWgt = tb.get<bf16_t>((size_t)2 * ff * D);
    bf16_t* dH = tb.get<bf16_t>((size_t)M * D); bf16_t* dAct = tb.get<bf16_t>((size_t)M * ff); float* dSS = tb.get<float>(nss);
    float* P = form == OGU_HALF_FUSED ? tb.get<float>((size_t)skinny_pick_ksplit(D, K) * (((M + 15) / 16) * 16) * D) : nullptr;       // o_proj's slabs
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    launch_tile_weights(dWo, dWot, D, K, e->st);
    launch_tile_weights_gu8(dWg, dWgt, 2 * ff, D, e->st);
    launch_o_gu(e, form, OGuChain{dA, dWot, dR, dw, dWgt, 1, dH, dAct, dSS, P, nullptr, nullptr}, M, K, D, ff, eps);
    TRY(down_bf16(e, tb, dR, resid, (size_t)rows_alloc * D));
    if (form != 0) TRY(down_bf16(e, tb, dH, hn_out, (size_t)M * D));
    TRY(down_bf16(e, tb, dAct, act_out, (size_t)M * ff));
    if (ss_out) HIPC(e, d2h(e, ss_out, dSS, nss * 4));
    return SONIC_OK;
}

// The prefill's RoPE + KV append through run_prefill()'s own descriptor builder (rope_append_args): packed qkv [n_tok][(Hq + 2 Hkv) * 128], the RoPE table cs [ctx_max][128], per token its sequence
// and position, per sequence its first packed token and length.  tiled = 1: rope_append_pf_kernel (q_off / q_len / n_seq / max_p passed); tiled = 0:
// rope_append_kernel<T, false> (they stay null: option no_rope_tiles).  Kc / Vc [B][Hkv][ctx_max][128] and Vt [B][Hkv][128][vt_ld] are uploaded, and read back
// after the launch; q_out [n_tok][Hq * 128].  The tile kernel takes a tile's first position from tok_pos of its first token and writes V^T for the 16 positions
// behind it: the contract is that sequence b's tokens are packed at q_off[b] .. + q_len[b] with positions 0 .. q_len[b] - 1, which is checked here.
extern "C" int sonic_test_rope_append(sonic_engine* e, const float* qkv, const float* cs, const int32_t* tok_seq, const int32_t* tok_pos, const int32_t* q_off, const int32_t* q_len,
                                      int n_tok, int B, int Hq, int Hkv, int ctx_max, int vt_ld, int tiled, float* q_out, float* Kc, float* Vc, float* Vt) {
    if (!e || !qkv || !cs || !tok_seq || !tok_pos || !q_off || !q_len || !q_out || !Kc || !Vc || !Vt) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(glue_16bit(e, "sonic_test_rope_append"));
    if (B < 1 || B > 4096 || n_tok < 1 || n_tok > (1 << 20) || Hq < 1 || Hq > 64 || Hkv < 1 || Hkv > 16 || ctx_max < 1 || ctx_max > (1 << 20) || vt_ld < ctx_max || vt_ld > (1 << 21))
        return fail(e, SONIC_ERR_INVALID, "rope_append: 1 <= Hkv <= 16, vt_ld >= ctx_max >= 1");
    long covered = 0; int max_p = 0;
    for (int b = 0; b < B; ++b) {
        if (q_len[b] < 1 || q_len[b] > ctx_max || q_off[b] < 0 || (long)q_off[b] + q_len[b] > n_tok)
            return fail(e, SONIC_ERR_INVALID, "sequence %d: q_off %d, q_len %d do not fit %d tokens / a context of %d", b, q_off[b], q_len[b], n_tok, ctx_max);
        for (int i = 0; i < q_len[b]; ++i)
            if (tok_seq[q_off[b] + i] != b || tok_pos[q_off[b] + i] != i)
                return fail(e, SONIC_ERR_INVALID, "token %d: sequence %d position %d where sequence %d position %d is packed", q_off[b] + i, tok_seq[q_off[b] + i], tok_pos[q_off[b] + i], b, i);
        covered += q_len[b]; max_p = q_len[b] > max_p ? q_len[b] : max_p;
    }
    if (covered != n_tok) return fail(e, SONIC_ERR_INVALID, "the sequences cover %ld of %d tokens", covered, n_tok);     // (with the loop above: every token in exactly one sequence)
    TmpBuf tb(e->st);
    const int N = (Hq + 2 * Hkv) * 128;
    const size_t nc = (size_t)B * Hkv * ctx_max * 128, nvt = (size_t)B * Hkv * 128 * vt_ld, nq = (size_t)n_tok * Hq * 128;
    bf16_t* dqkv = up_bf16(e, tb, qkv, (size_t)n_tok * N); float* dcs = up_f32(e, tb, cs, (size_t)ctx_max * 128);
    bf16_t* dk = up_bf16(e, tb, Kc, nc); bf16_t* dv = up_bf16(e, tb, Vc, nc); bf16_t* dvt = up_bf16(e, tb, Vt, nvt); bf16_t* dq = tb.get<bf16_t>(nq);
    int* di = tb.get<int>((size_t)2 * n_tok + 2 * B);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    HIPC(e, h2d(e, di, tok_seq, (size_t)n_tok * 4)); HIPC(e, h2d(e, di + n_tok, tok_pos, (size_t)n_tok * 4));
    HIPC(e, h2d(e, di + 2 * n_tok, q_off, (size_t)B * 4)); HIPC(e, h2d(e, di + 2 * n_tok + B, q_len, (size_t)B * 4));
    launch_rope_append(rope_append_args(dqkv, dq, dk, dv, dvt, vt_ld, di, di + n_tok, dcs, Hq, Hkv, ctx_max, n_tok, e->dt, tiled ? di + 2 * n_tok : nullptr, di + 2 * n_tok + B, B, max_p),
                       false, e->st);
    TRY(down_bf16(e, tb, dq, q_out, nq));
    TRY(down_bf16(e, tb, dk, Kc, nc));
    TRY(down_bf16(e, tb, dv, Vc, nc));
    return down_bf16(e, tb, dvt, Vt, nvt);
}

// rope_enc_kernel in place on qk [M][ld]: heads2 heads of hd = 64 at the front of every row, the first rd dims of each rotated with row (m mod T) of cs [T][rd]
extern "C" int sonic_test_rope_enc(sonic_engine* e, float* qk, int M, int ld, int T, int heads2, int hd, int rd, const float* cs) {
    if (!e || !qk || !cs) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(glue_16bit(e, "sonic_test_rope_enc"));
    if (hd != 64 || rd < 16 || rd > hd || rd % 16 || heads2 < 1 || heads2 > 256 || M < 1 || M > (1 << 20) || T < 1 || ld < heads2 * hd || ld % 8 || ld > (1 << 20))
        return fail(e, SONIC_ERR_INVALID, "rope_enc: hd == 64, rd %% 16 == 0, 16 <= rd <= hd, ld >= heads2 * hd, ld %% 8 == 0");
    TmpBuf tb(e->st);
    bf16_t* dqk = up_bf16(e, tb, qk, (size_t)M * ld); float* dcs = up_f32(e, tb, cs, (size_t)T * rd);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    launch_rope_enc(dqk, ld, M, T, heads2, hd, rd, dcs, e->st, e->dt);
    return down_bf16(e, tb, dqk, qk, (size_t)M * ld);
}

// ------------------------------------------------------------------------------------------ int8 decode step: one decode-flavour Linear8bitLt plus its consumer
// (tests/test_gpu_int8_decode_glue.py).  X [M][K] and W [N][K] are fp32 holding fp16 values, 1 <= M <= 64.  W is quantised on the device (launch_quant_weights), tiled
// (launch_tile_weights_i8) and, with layout = 1, also transposed into the k-major copy (launch_transpose_i8); the row-major matrix is not handed on, as in the step.  The
// Linear runs as decode_step_i8 runs it - skinny_i8 into int32 slabs, the consumer's DeqInfo from deq_info - and the consumer is launched through its own launcher.
// info_out (optional) [2]: ksplit as launched, the tiling skinny_i8_cfg chose.  slab_sum_out (optional) int32 [M][N]: the slabs summed over ksplit (rows behind M, which
// the GEMM fills with copies of its last row, are not returned).  Every shape and index is checked before the first launch.
struct I8Lin { bf16_t* X = nullptr; QW w; QuantOut qx{}; float* P = nullptr; int ks = 0, mpad = 0, cfg = 0; };
static int i8lin_check(sonic_engine* e, const char* who, int M, int N, int K, int layout) {
    if (!e->i8) return fail(e, SONIC_ERR_INVALID, "%s needs an engine created with mode int8", who);
    if (M < 1 || M > 64 || N < 32 || N > (1 << 16) || K < 256 || K > 8192 || (layout != 0 && layout != 1))
        return fail(e, SONIC_ERR_INVALID, "%s: 1 <= M <= 64, 32 <= N <= 65536, 256 <= K <= 8192, layout 0 (tiled) or 1 (tiled + k-major)", who);
    if (skinny_i8_cfg(N, K) < 0 || skinny_pick_ksplit_i8(N, K) < 1) return fail(e, SONIC_ERR_INVALID, "%s: N = %d, K = %d is not a shape of the int8 skinny GEMM (N %% 32 == 0, K %% 256 == 0)", who, N, K);
    return SONIC_OK;
}
// uploads, allocations and the weight preparation; qx: the five arrays of the rows' quantised form (form 0: written by launch_quant_rows; scan form: the spill space)
static int i8lin_prepare(sonic_engine* e, TmpBuf& tb, const float* X, const float* W, int M, int N, int K, int layout, I8Lin* L) {
    L->cfg = skinny_i8_cfg(N, K); L->ks = skinny_pick_ksplit_i8(N, K); L->mpad = ((M + 15) / 16) * 16;
    L->X = up_bf16(e, tb, X, (size_t)M * K); bf16_t* dW = up_bf16(e, tb, W, (size_t)N * K);
    int8_t* cb = tb.get<int8_t>((size_t)N * K); L->w.scb = tb.get<float>(N); L->w.cbt = tb.get<int8_t>((size_t)N * K);
    if (layout == 1) L->w.cbk = tb.get<int8_t>((size_t)N * K);
    L->P = tb.get<float>((size_t)L->ks * L->mpad * N);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    TRY(quant_alloc(e, tb, M, K, &L->qx));
    launch_quant_weights(dW, cb, L->w.scb, N, K, e->st);
    launch_tile_weights_i8(cb, L->w.cbt, N, K, e->st);
    if (layout == 1) launch_transpose_i8(cb, L->w.cbk, N, K, e->st);
    L->w.cb = nullptr; L->w.cb_rowmajor_kept = false;
    return SONIC_OK;
}
// form 0: launch_quant_rows + skinny_i8 on the codes; amax != null: skinny_i8 quantises the fp16 rows itself
static void i8lin_run(sonic_engine* e, I8Lin* L, const float* amax, int M, int N, int K) {
    if (!amax) launch_quant_rows(L->X, K, M, K, L->qx, e->st);
    L->ks = skinny_i8(e, amax ? (const void*)L->X : (const void*)L->qx.q, amax, L->w.cbt, L->P, M, N, K);
}
static int i8lin_report(sonic_engine* e, const I8Lin& L, int M, int N, int32_t* info_out, int32_t* slab_sum_out) {
    if (info_out) { info_out[0] = L.ks; info_out[1] = L.cfg; }
    if (!slab_sum_out) return SONIC_OK;
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    std::vector<int32_t> h((size_t)L.ks * L.mpad * N);
    HIPC(e, d2h(e, h.data(), L.P, h.size() * 4));
    for (int m = 0; m < M; ++m)
        for (int n = 0; n < N; ++n) {
            int64_t s = 0;
            for (int k = 0; k < L.ks; ++k) s += h[((size_t)k * L.mpad + m) * N + n];
            slab_sum_out[(size_t)m * N + n] = (int32_t)s;
        }
    return SONIC_OK;
}

// o_proj / down_proj of the int8 step, then launch_add_rmsnorm with the DeqInfo and a QuantOut: x [rows_alloc][N] (in place) and y [rows_alloc][N] go up with the caller's
// contents; norm_w [N].  form 0: launch_quant_rows -> skinny_i8 -> the listed DeqInfo.  form 1 (the step's default): amax [M][4] = the rows' absmax partials without the
// elements >= 6.0, big [M][4] = the counts of those elements; skinny_i8 gets the partials, the DeqInfo sca = amax, scan = 1, scan_cnt = big.  The five outputs are the
// QuantOut of y as sonic_test_add_rmsnorm returns them: q [M][N], sca / oc_cnt [M], oc_list / oc_val [M][N].
extern "C" int sonic_test_decode_i8_norm(sonic_engine* e, const float* X, const float* W, float* x, const float* norm_w, float eps, float* y, const float* amax, const int32_t* big,
                                         int M, int N, int K, int rows_alloc, int form, int layout,
                                         int8_t* q_out, float* sca_out, int32_t* oc_cnt_out, int32_t* oc_list_out, float* oc_val_out, int32_t* info_out, int32_t* slab_sum_out) {
    if (!e || !X || !W || !x || !norm_w || !y || !q_out || !sca_out || !oc_cnt_out || !oc_list_out || !oc_val_out) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(i8lin_check(e, "sonic_test_decode_i8_norm", M, N, K, layout));
    const int threads = ((N >> 3) + 63) / 64 * 64;
    if (N % 8 || N > 2048 || rows_alloc < M || rows_alloc > 4096 || (form != 0 && form != 1))
        return fail(e, SONIC_ERR_INVALID, "decode_i8_norm: N %% 8 == 0, N <= 2048, rows_alloc >= M, form 0 or 1");
    if (form == 1 && (!amax || !big || K > 32 * threads)) return fail(e, SONIC_ERR_INVALID, "decode_i8_norm: form 1 needs the partials, the counts and K <= 32 x the block size (%d)", 32 * threads);
    TmpBuf tb(e->st);
    I8Lin L;
    const size_t n = (size_t)rows_alloc * N;
    bf16_t* dx = up_bf16(e, tb, x, n); bf16_t* dy = up_bf16(e, tb, y, n); float* dw = up_f32(e, tb, norm_w, N);
    float* damax = form == 1 ? up_f32(e, tb, amax, (size_t)M * 4) : nullptr; int* dbig = form == 1 ? tb.get<int>((size_t)M * 4) : nullptr;
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    if (form == 1) HIPC(e, h2d(e, dbig, big, (size_t)M * 16));
    TRY(i8lin_prepare(e, tb, X, W, M, N, K, layout, &L));
    QuantOut qo{};
    TRY(quant_alloc(e, tb, M, N, &qo));
    i8lin_run(e, &L, damax, M, N, K);
    DeqInfo dq = deq_info(e, L.qx, L.w, K, L.X, N);
    if (form == 1) { dq.sca = damax; dq.scan = 1; dq.scan_cnt = dbig; }
    launch_add_rmsnorm(dx, L.P, L.ks, L.mpad, dw, dy, M, N, eps, e->st, DT_F16, &dq, &qo);
    TRY(down_bf16(e, tb, dx, x, n));
    TRY(down_bf16(e, tb, dy, y, n));
    TRY(quant_fetch(e, qo, M, N, QuantHost{q_out, sca_out, oc_cnt_out, oc_list_out, oc_val_out}));
    return i8lin_report(e, L, M, N, info_out, slab_sum_out);
}

// gate/up of the int8 step (W [2 ff][K], gate / up rows interleaved in groups of 16), then launch_swiglu_quant: act [rows_alloc][ff] goes up with the caller's contents;
// the five outputs are the QuantOut of act, [M][ff]
extern "C" int sonic_test_decode_i8_swiglu(sonic_engine* e, const float* X, const float* W, float* act, int M, int ff, int K, int rows_alloc, int layout,
                                           int8_t* q_out, float* sca_out, int32_t* oc_cnt_out, int32_t* oc_list_out, float* oc_val_out, int32_t* info_out, int32_t* slab_sum_out) {
    if (!e || !X || !W || !act || !q_out || !sca_out || !oc_cnt_out || !oc_list_out || !oc_val_out) return SONIC_ERR_INVALID;
    ENTER(e);
    if (ff < 16 || ff % 16 || ff > 8192 || rows_alloc < M || rows_alloc > 4096) return fail(e, SONIC_ERR_INVALID, "decode_i8_swiglu: ff %% 16 == 0, ff <= 8192, rows_alloc >= M");
    TRY(i8lin_check(e, "sonic_test_decode_i8_swiglu", M, 2 * ff, K, layout));
    TmpBuf tb(e->st);
    I8Lin L;
    bf16_t* dA = up_bf16(e, tb, act, (size_t)rows_alloc * ff);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    TRY(i8lin_prepare(e, tb, X, W, M, 2 * ff, K, layout, &L));
    QuantOut qo{};
    TRY(quant_alloc(e, tb, M, ff, &qo));
    i8lin_run(e, &L, nullptr, M, 2 * ff, K);
    launch_swiglu_quant(L.P, L.ks, L.mpad, ff, dA, M, deq_info(e, L.qx, L.w, K, L.X, 2 * ff), qo, e->st);
    TRY(down_bf16(e, tb, dA, act, (size_t)rows_alloc * ff));
    TRY(quant_fetch(e, qo, M, ff, QuantHost{q_out, sca_out, oc_cnt_out, oc_list_out, oc_val_out}));
    return i8lin_report(e, L, M, 2 * ff, info_out, slab_sum_out);
}

// q|k|v of the int8 step (X = the hidden rows [B][D], Wqkv [(Hq + 2 Hkv) * 128][D]), then launch_decode_attn in fused mode with the DeqInfo, amax_out and big_out; rope_cs,
// the caches and kv_len as sonic_test_decode_attention_cache takes them.  amax [B][4] and big [B][4] go up with the caller's contents and come back as the launch left them
extern "C" int sonic_test_decode_i8_attn(sonic_engine* e, const float* X, const float* Wqkv, const float* rope_cs, const float* kcache, const float* vcache, const int32_t* kv_len,
                                         float* amax, int32_t* big, float* out, float* kcache_out, float* vcache_out, int B, int D, int Hq, int Hkv, int ctx_max, int layout,
                                         int32_t* info_out, int32_t* slab_sum_out) {
    if (!e || !X || !Wqkv || !rope_cs || !kcache || !vcache || !kv_len || !amax || !big || !out) return SONIC_ERR_INVALID;
    ENTER(e);
    const int hd = 128;
    if (Hkv < 1 || Hkv > 4 || Hq < Hkv || Hq % Hkv || Hq / Hkv > 4 || ctx_max < 1 || ctx_max > (1 << 20)) return fail(e, SONIC_ERR_INVALID, "decode_i8_attn: 1 <= Hkv <= 4, Hq / Hkv in 1 .. 4, ctx_max >= 1");
    const int N = (Hq + 2 * Hkv) * hd;
    TRY(i8lin_check(e, "sonic_test_decode_i8_attn", B, N, D, layout));
    for (int b = 0; b < B; ++b)
        if (kv_len[b] < 1 || kv_len[b] > ctx_max) return fail(e, SONIC_ERR_INVALID, "kv_len[%d] = %d outside 1..%d", b, kv_len[b], ctx_max);
    TmpBuf tb(e->st);
    I8Lin L;
    const size_t nc = (size_t)B * Hkv * ctx_max * hd, no = (size_t)B * Hq * hd;
    bf16_t* dk = up_bf16(e, tb, kcache, nc); bf16_t* dv = up_bf16(e, tb, vcache, nc); float* dcs = up_f32(e, tb, rope_cs, (size_t)ctx_max * hd);
    float* damax = up_f32(e, tb, amax, (size_t)B * 4); int* dbig = tb.get<int>((size_t)B * 4);
    bf16_t* dO = tb.get<bf16_t>(no); int* kl = tb.get<int>(B);
    if (tb.bad()) return fail(e, SONIC_ERR_OOM, "HIP out of memory in test hook");
    HIPC(e, h2d(e, dbig, big, (size_t)B * 16)); HIPC(e, h2d(e, kl, kv_len, (size_t)B * 4));
    TRY(i8lin_prepare(e, tb, X, Wqkv, B, N, D, layout, &L));
    i8lin_run(e, &L, nullptr, B, N, D);
    DecodeAttnArgs da = decode_attn_args(dk, dv, L.P, nullptr, L.ks, L.mpad, dcs, dO, kl, Hq, Hkv, ctx_max, DT_F16);
    da.dq = deq_info(e, L.qx, L.w, D, L.X, N); da.amax_out = damax; da.big_out = dbig;
    launch_decode_attn(da, B, e->st);
    TRY(down_bf16(e, tb, dO, out, no));
    if (kcache_out) TRY(down_bf16(e, tb, dk, kcache_out, nc));
    if (vcache_out) TRY(down_bf16(e, tb, dv, vcache_out, nc));
    HIPC(e, d2h(e, amax, damax, (size_t)B * 16)); HIPC(e, d2h(e, big, dbig, (size_t)B * 16));
    return i8lin_report(e, L, B, N, info_out, slab_sum_out);
}
