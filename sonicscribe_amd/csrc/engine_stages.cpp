// sonic_hip engine: the stages of the bf16 / fp16 / int8 pipeline on the engine stream - GEMM wrappers, log-mel, encoder, request plan, prefill,
// the token step and its captured chunk graphs, the greedy loop.
#include "engine_internal.h"

// ------------------------------------------------------------------------------------------ pipeline stages
void gemm(sonic_engine* e, int epi, const bf16_t* A, long lda, const bf16_t* W, const float* bias, bf16_t* C, long ldc,
          int M, int N, int K, const bf16_t* R, long ldr, int w_tiled, int gu8) {
    GemmArgs a{};
    a.A = A; a.lda = lda; a.W = W; a.C = C; a.ldc = ldc; a.bias = bias; a.R = R; a.ldr = ldr; a.M = M; a.N = N; a.K = K; a.batch = 1; a.dt = e->dt;
    a.w_tiled = w_tiled; a.gu8 = gu8;
    a.gelu_lut = e->opt_no_gelu_lut ? nullptr : e->gelu_lut;
    launch_gemm(a, epi, e->st);
}
// One nn.Linear of the model on X [M][K] (row stride ldx).  Native mode: the 16-bit GEMM.  int8 mode and a swapped module (q.cb):
// Linear8bitLt = activation quantisation (3 streaming passes) + int8 MFMA GEMM whose epilogue dequantises and adds the outlier columns.
// rope_cs (optional): fuse the encoder's partial RoPE on columns < rope_ncols into the epilogue; returns whether it was fused (only the
// 256x256 kernel does it), else the caller runs the separate RoPE pass.
static QuantActArgs make_qa(sonic_engine* e, const bf16_t* X, long ldx, int M, int K, const QGroup& grp) {
    QuantActArgs qa{};
    qa.X = X; qa.ld = ldx; qa.M = M; qa.K = K; qa.gmap = grp.gmap; qa.gdiv = grp.gdiv; qa.G = grp.G; qa.flags = e->q_flags;
    qa.q = e->qa; qa.sca = e->q_sca; qa.oc_cnt = e->q_oc_cnt; qa.oc_list = e->q_oc_list; qa.oc_ld = e->q_kmax;
    return qa;
}
// LayerNorm whose output feeds a Linear8bitLt directly (ld == K == d): in int8 mode the norm kernel also quantises the row
static bool layernorm_q(sonic_engine* e, const bf16_t* x, const float* w, const float* b, bf16_t* y, int M, int d, float eps, const QGroup& grp) {
    if (e->i8 && !e->opt_i8_no_lnq) {
        const QuantActArgs qa = make_qa(e, y, d, M, d, grp);
        launch_quant_act_begin(qa, e->st);
        launch_layernorm(x, w, b, y, M, d, eps, e->st, e->dt, &qa);
        return true;
    }
    launch_layernorm(x, w, b, y, M, d, eps, e->st, e->dt);
    return false;
}
static bool rmsnorm_q(sonic_engine* e, const bf16_t* x, const float* w, bf16_t* y, int M, int d, float eps, const QGroup& grp) {
    if (e->i8 && !e->opt_i8_no_lnq) {
        const QuantActArgs qa = make_qa(e, y, d, M, d, grp);
        launch_quant_act_begin(qa, e->st);
        launch_rmsnorm(x, w, y, M, d, eps, nullptr, e->st, e->dt, &qa);
        return true;
    }
    launch_rmsnorm(x, w, y, M, d, eps, nullptr, e->st, e->dt);
    return false;
}
bool qlinear(sonic_engine* e, int epi, const bf16_t* X, long ldx, const bf16_t* w16, const QW& q, const float* bias, bf16_t* C, long ldc,
             int M, int N, int K, const bf16_t* R, long ldr, const QGroup& grp, const float* rope_cs, int rope_T, int rope_ncols,
             bool prequant, const QkvVt* vt) {
    if (!e->i8 || !(q.cb || q.cbt)) { gemm(e, epi, X, ldx, w16, bias, C, ldc, M, N, K, R, ldr); return false; }
    const QuantActArgs qa = make_qa(e, X, ldx, M, K, grp);
    if (prequant) launch_quant_act_finish(qa, e->st);      // the LayerNorm that wrote X also wrote its codes, absmax and flags
    else launch_quant_act(qa, e->st);
    GemmArgs a{};
    a.A = (const bf16_t*)e->qa; a.lda = K; a.W = (const bf16_t*)q.cb; a.C = C; a.ldc = ldc; a.bias = bias; a.R = R; a.ldr = ldr; a.M = M; a.N = N; a.K = K; a.batch = 1; a.dt = DT_F16;
    // decoder projections: ONE int8 operand copy since round 5 - the fragment-tiled one of the decode step (+ the k-major copy for outlier columns)
    if (q.cbt && (!e->opt_prefill_rowmajor || !q.cb_rowmajor_kept)) { a.W = (const bf16_t*)q.cbt; a.w_tiled = 1; }     // (outlier columns are gathered from the tiled copy)
    a.q.sca = e->q_sca; a.q.scb = q.scb; a.q.x16 = X; a.q.ldx16 = ldx; a.q.oc_cnt = e->q_oc_cnt; a.q.oc_list = e->q_oc_list; a.q.oc_ld = e->q_kmax;
    a.q.row_group = grp.gmap; a.q.group_div = grp.gdiv;
    // int8 q|k|v: RoPE + V^T inside the GEMM's epilogue (round 3; the register form of the 16-bit kinds spilled beside the dequantisation, the int8
    // kind does both on the staged tile).  Returns true: the caller skips its RoPE and transpose passes.
    bool fuse = false;
    if (vt && rope_cs && !e->opt_i8_no_qkv_fuse && !g_opts.gemm_force128) {
        GemmArgs t = a; t.Vt = vt->Vt; t.n_split = vt->n_split; t.seg_T = vt->seg_T; t.vt_ld = vt->vt_ld; t.vt_seg_stride = vt->vt_seg_stride;
        if (gemm256_eligible(t, EPI_QKV_VT)) { a = t; a.rope_cs = rope_cs; a.rope_T = rope_T; a.rope_ncols = rope_ncols; epi = EPI_QKV_VT; fuse = true; }
    }
    // residual-epilogue linears (o_proj, fc2, down_proj: their inputs are activation outputs, where long outlier lists occur): requests with
    // more than `i8_defer_thr` outlier columns are finished by the dense side product instead of the epilogue's per-element list walk
    const bool defer = epi == EPI_BIAS_RESID && e->defer_tmp && e->opt_i8_defer_thr >= 0 && (size_t)M * ldc <= e->defer_cap;
    if (defer) { a.q.defer_out = e->defer_tmp; a.q.defer_thr = e->opt_i8_defer_thr; }
    launch_gemm(a, epi, e->st);
    if (defer) launch_i8_outlier_side(a, e->st);
    return fuse;
}

int run_mel(sonic_engine* e, int W, bool want_f32) {
    const sonic_dims& d = e->d;
    if (want_f32 && !e->feats_f32) {
        HIPC(e, hipMalloc((void**)&e->feats_f32, (size_t)e->Bm * d.n_mels * d.n_frames * 4));
    }
    int mx = 0; for (int i = 0; i < W; ++i) mx = e->n_samples_h[i] > mx ? e->n_samples_h[i] : mx;
    launch_logmel(e->pcm, (long)d.n_frames * 160, e->n_samples_d, mx, e->lc, e->logspec, e->segmax, W, d.n_frames, d.n_mels,
                  e->feats_fm, want_f32 ? e->feats_f32 : nullptr, e->st, e->dt);
    return SONIC_OK;
}

// feats_fm (16-bit, frame-major, padded) -> pe [W*Ta][dec_d].  win_group: request of each window (int8 mode: LLM.int8 finds its outlier
// columns over all rows of one reference call, i.e. over all windows of a request - HF runs them as one encoder batch)
int run_encoder(sonic_engine* e, int W, float* enc_layers_out, float* enc_out_host, int n_groups) {
    const sonic_dims& d = e->d;
    const int C = d.enc_d, T = e->T, M = W * T, H = d.enc_heads, dt = e->dt;
    const QGroup grp{e->win_req, T, n_groups}, grp_p{e->win_req, e->Ta, n_groups};
    {   // conv stem as two batched im2col-free GEMMs (modeling_glmasr.py:313-316); nn.Conv1d is not swapped in int8 mode
        GemmArgs a{};
        a.A = e->feats_fm; a.lda = d.n_mels; a.W = e->conv1w; a.bias = e->conv1b; a.C = e->h1 + C; a.ldc = C; a.dt = dt;
        a.M = d.n_frames; a.N = C; a.K = 3 * d.n_mels; a.batch = W;
        a.strideA = (long)(d.n_frames + 2) * d.n_mels; a.strideC = (long)(d.n_frames + 2) * C;
        launch_gemm(a, EPI_BIAS_GELU, e->st);
        GemmArgs b{};
        b.A = e->h1; b.lda = 2L * C; b.W = e->conv2w; b.bias = e->conv2b; b.C = e->x; b.ldc = C; b.dt = dt;
        b.M = T; b.N = C; b.K = 3 * C; b.batch = W; b.strideA = (long)(d.n_frames + 2) * C; b.strideC = (long)T * C;
        launch_gemm(b, EPI_BIAS_GELU, e->st);
    }
    float* tap = nullptr;
    if (enc_layers_out || enc_out_host) HIPC(e, hipMalloc((void**)&tap, (size_t)M * C * 4));
    e->gemm_ev_used = 0;
    for (int l = 0; l < d.enc_layers; ++l) {
        const EncLayerW& L = e->enc[l];
        const bool pq1 = layernorm_q(e, e->x, L.ln1w, L.ln1b, e->ln, M, C, d.enc_ln_eps, grp);
        const bool tev = e->opt_gemm_timing && (size_t)(8 * l + 7) < e->gemm_ev.size();
        auto mark = [&](int i) { if (tev) (void)hipEventRecord(e->gemm_ev[8 * l + i], e->st); };
        FlashArgs f{};
        f.dt = dt; f.T = T; f.Hq = H; f.Hkv = H; f.scale = 1.0f / sqrtf((float)e->hd_e); f.Vt = e->vt; f.vt_ld = e->Tp; f.O = e->att; f.o_ld = C;
        f.k_head_stride = e->hd_e; f.vt_seq_stride = (long)C * e->Tp; f.vt_head_stride = (long)e->hd_e * e->Tp;
        if (e->i8) {
            // Linear8bitLt q / k / v share their input, hence one quantisation and one fused int8 GEMM; Q | K | V land row-major
            // ([M][3C]) and V is transposed by its own pass (the fused V^T epilogue plus the dequantisation spills registers)
            mark(0);
            const bool can_fuse = e->hd_e == 64 && d.enc_rotary_dim == 32 && !e->opt_no_fused_rope;
            const QkvVt vt{e->vt, 2 * C, T, e->Tp, (long)C * e->Tp};
            const bool fused = qlinear(e, EPI_BIAS, e->ln, C, nullptr, L.qqkv, L.bqkv, e->qkv_rm, 3L * C, M, 3 * C, C, nullptr, 0, grp,
                                       can_fuse ? e->enc_cs : nullptr, T, 2 * C, pq1, &vt);
            mark(1);
            if (!fused) {
                launch_rope_enc(e->qkv_rm, 3L * C, M, T, 2 * H, e->hd_e, d.enc_rotary_dim, e->enc_cs, e->st, dt);
                launch_transpose_v(e->qkv_rm, 3L * C, 2 * C, e->vt, W, T, C, e->Tp, (long)C * e->Tp, e->st);
            }
            f.Q = e->qkv_rm; f.q_ld = 3L * C; f.K = e->qkv_rm + C; f.k_ld = 3L * C;
            f.q_seq_stride = (long)T * 3 * C; f.k_seq_stride = (long)T * 3 * C;
        } else {
            GemmArgs a{};
            a.A = e->ln; a.lda = C; a.W = L.wqkv; a.bias = L.bqkv; a.C = e->qk; a.ldc = 2L * C; a.M = M; a.N = 3 * C; a.K = C; a.batch = 1; a.dt = dt;
            a.Vt = e->vt; a.n_split = 2 * C; a.seg_T = T; a.vt_ld = e->Tp; a.vt_seg_stride = (long)C * e->Tp;
            // partial RoPE of q / k in the GEMM's epilogue (the rotation pairs are in one lane's accumulators): no separate HBM pass
            const bool roped = e->hd_e == 64 && d.enc_rotary_dim == 32 && !e->opt_no_fused_rope && !g_opts.gemm_force128 && gemm256_eligible(a, EPI_QKV_VT);
            if (roped) { a.rope_cs = e->enc_cs; a.rope_T = T; a.rope_ncols = 2 * C; }
            mark(0);
            launch_gemm(a, EPI_QKV_VT, e->st);
            mark(1);
            if (!roped) launch_rope_enc(e->qk, 2L * C, M, T, 2 * H, e->hd_e, d.enc_rotary_dim, e->enc_cs, e->st, dt);
            f.Q = e->qk; f.q_ld = 2L * C; f.K = e->qk + C; f.k_ld = 2L * C;
            f.q_seq_stride = (long)T * 2 * C; f.k_seq_stride = (long)T * 2 * C;
        }
        launch_flash(f, 64, false, W, T, e->st);
        mark(2);
        qlinear(e, EPI_BIAS_RESID, e->att, C, L.wo, L.qo, L.bo, e->x, C, M, C, C, e->x, C, grp);
        mark(3);
        const bool pq2 = layernorm_q(e, e->x, L.ln2w, L.ln2b, e->ln, M, C, d.enc_ln_eps, grp);
        mark(4);
        qlinear(e, EPI_BIAS_GELU, e->ln, C, L.w1, L.q1, L.b1, e->ff, d.enc_ff, M, d.enc_ff, C, nullptr, 0, grp, nullptr, 0, 0, pq2);
        mark(5);
        if (tev) e->gemm_ev_used = l + 1;
        mark(6);
        qlinear(e, EPI_BIAS_RESID, e->ff, d.enc_ff, L.w2, L.q2, L.b2, e->x, C, M, C, d.enc_ff, e->x, C, grp);
        mark(7);
        if (enc_layers_out) {
            launch_bf16_to_f32(e->x, tap, (long)M * C, e->st, dt);
            HIPC(e, stream_sync(e));
            for (int b = 0; b < W; ++b)
                HIPC(e, d2h(e, enc_layers_out + ((size_t)b * d.enc_layers + l) * T * C, tap + (size_t)b * T * C, (size_t)T * C * 4));
        }
    }
    launch_layernorm(e->x, e->enc_nw, e->enc_nb, e->ln, M, C, d.enc_ln_eps, e->st, dt);
    if (enc_out_host) {
        launch_bf16_to_f32(e->ln, tap, (long)M * C, e->st, dt);
        HIPC(e, stream_sync(e));
        HIPC(e, d2h(e, enc_out_host, tap, (size_t)M * C * 4));
    }
    if (tap) (void)hipFree(tap);
    // 4-frame merge is a view: [M][C] == [W*Ta][4C] (modeling_glmasr.py:392-397)
    const int Mp = W * e->Ta, PI = C * d.merge, PM = 2 * d.dec_d;
    qlinear(e, EPI_BIAS_GELU, e->ln, PI, e->pj1w, e->qpj1, e->pj1b, e->ph, PM, Mp, PM, PI, nullptr, 0, grp_p);
    qlinear(e, EPI_BIAS, e->ph, PM, e->pj2w, e->qpj2, e->pj2b, e->pe, d.dec_d, Mp, d.dec_d, PM, nullptr, 0, grp_p);
    return SONIC_OK;
}

static int floordiv(int a, int b) { int q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }
int keep_rows(const sonic_dims& d, int n_valid_frames) {  // modeling_glmasr.py:399-403 (python floor division)
    int L = n_valid_frames;
    L = floordiv(L + 2 - 2 - 1, 1) + 1;
    L = floordiv(L + 2 - 2 - 1, 2) + 1;
    const int k = floordiv(L - d.merge, d.merge) + 1;
    const int Ta = d.enc_T / d.merge;
    return k < 0 ? 0 : (k > Ta ? Ta : k);
}
int frames_of(int n_samples) { return n_samples > 0 ? (n_samples + 159) / 160 : 0; }

// ------------------------------------------------------------------------------------------ launch descriptors: one builder each (production and the hooks)
SkinnyArgs skinny_args(const bf16_t* X, long ldx, const bf16_t* W, float* P, int M, int N, int K, int ksplit, int dt) {
    SkinnyArgs a{};
    a.X = X; a.ldx = ldx; a.W = W; a.P = P; a.M = M; a.N = N; a.K = K; a.ksplit = ksplit; a.dt = dt;
    return a;
}
// P != null, the token step's form: the kernel sums the q|k|v slabs, ropes at kv_len - 1 and appends K / V itself; else Q holds the roped queries
DecodeAttnArgs decode_attn_args(bf16_t* Kc, bf16_t* Vc, const float* P, const bf16_t* Q, int ksplit, int mpad, const float* cs, bf16_t* O, const int* kv_len,
                                int Hq, int Hkv, int ctx_max, int dt) {
    DecodeAttnArgs a{};
    a.Q = Q; a.P = P; a.ksplit = ksplit; a.mpad = mpad; a.cs = cs; a.Kc = Kc; a.Vc = Vc; a.O = O; a.kv_len = kv_len; a.Hq = Hq; a.Hkv = Hkv; a.ctx_max = ctx_max;
    a.scale = 1.0f / sqrtf(128.f); a.dt = dt;            // head dim 128: the only one the decoder's kernels have (sonic_create refuses others)
    return a;
}
// the prefill's causal attention: packed ragged queries, K in cache layout [B][Hkv][ctx_max][128], V^T [B][Hkv][128][ctx_max]
FlashArgs prefill_flash_args(const bf16_t* Q, const bf16_t* Kc, const bf16_t* Vt, bf16_t* O, const int* q_off, const int* q_len, const int* kv_len,
                             int Hq, int Hkv, int ctx_max, int dt) {
    FlashArgs f{}; f.dt = dt;
    f.Q = Q; f.q_ld = Hq * 128L; f.K = Kc; f.k_ld = 128; f.Vt = Vt; f.vt_ld = ctx_max; f.O = O; f.o_ld = Hq * 128L;
    f.k_seq_stride = (long)Hkv * ctx_max * 128; f.k_head_stride = ctx_max * 128L; f.vt_seq_stride = (long)Hkv * 128 * ctx_max; f.vt_head_stride = 128L * ctx_max;
    f.q_off = q_off; f.q_len = q_len; f.kv_len = kv_len; f.Hq = Hq; f.Hkv = Hkv; f.scale = 1.0f / sqrtf(128.f);
    return f;
}
// the prefill's RoPE + KV append on packed qkv [n_tok][(Hq + 2 Hkv) * 128].  q_off != null: tiles of 16 positions per sequence (round 5); else one token at a time
RopeAppendArgs rope_append_args(const bf16_t* qkv, bf16_t* q_out, bf16_t* Kc, bf16_t* Vc, bf16_t* Vt, long vt_ld, const int* tok_seq, const int* tok_pos, const float* cs,
                                int Hq, int Hkv, int ctx_max, int n_tok, int dt, const int* q_off, const int* q_len, int n_seq, int max_p) {
    RopeAppendArgs ra{}; ra.dt = dt;
    ra.qkv = qkv; ra.ld = (Hq + 2 * Hkv) * 128; ra.q_out = q_out; ra.Kc = Kc; ra.Vc = Vc; ra.Vt = Vt; ra.vt_ld = vt_ld;
    ra.tok_seq = tok_seq; ra.tok_pos = tok_pos; ra.cs = cs; ra.Hq = Hq; ra.Hkv = Hkv; ra.ctx_max = ctx_max; ra.n_tok = n_tok;
    if (q_off) { ra.q_off = q_off; ra.q_len = q_len; ra.n_seq = n_seq; ra.max_p = max_p; }
    return ra;
}

// the word-timestamp launches (align.hip) over the handle's align plan and buffers: Q = the roped query rows, K = the audio keys as the strides say
// (the prefill: a layer's K cache; the hook: caller rows), `heads` = n_heads ascending head ids on the device
AlignArgs align_probs_args(sonic_engine* e, const bf16_t* Q, const bf16_t* K, long k_ld, long k_head_stride, long k_seq_stride, const int* heads, int n_heads, int Hq, int Hkv, const int* rec) {
    AlignArgs a{};
    a.Q = Q; a.q_ld = Hq * 128L; a.K = K; a.k_ld = k_ld; a.k_head_stride = k_head_stride; a.k_seq_stride = k_seq_stride;
    a.qrow = e->align_plan_d; a.rseq = e->align_plan_d + e->tok_cap; a.seqp = e->align_plan_d + 2 * (size_t)e->tok_cap; a.heads = heads; a.rec = rec;
    a.n_heads = n_heads; a.grp = Hq / Hkv; a.S = e->align_S; a.n_seq = e->align_nseq; a.A_max = e->align_Amax; a.L_max = e->align_Lmax; a.dt = e->dt;
    a.scale = 1.0f / sqrtf(128.f); a.h_total = (float)e->align_Htot;
    a.P = e->align_P; a.Z = e->align_P + e->align_Zoff; a.M = e->align_M; a.t_out = e->align_t; a.trace = e->align_trace;
    return a;
}

static long long* kt_slot(sonic_engine* e, int l, int slot) { return (e->kt && l == e->kt_layer) ? e->kt + (long)slot * KT_SLOT_BLOCKS * 8 : nullptr; }
void skinny(sonic_engine* e, const bf16_t* X, long ldx, const bf16_t* W, float* P, int M, int N, int K, int* ks_out, long long* kt) {
    SkinnyArgs a = skinny_args(X, ldx, W, P, M, N, K, skinny_pick_ksplit(N, K), e->dt); a.kt = kt;
    if (ks_out) *ks_out = a.ksplit;
    launch_skinny(a, e->st);
}
// int8 decode step: rows X [M][K] x fragment-tiled int8 weights -> int32 slabs (dequantised by the consumer).  amax == null: X holds the quantised rows; else the
// UNQUANTISED fp16 rows with their gathered absmax partials, and the kernel quantises its X slice while staging it.  (The int8 kernels do not read dt.)
static int skinny_i8(sonic_engine* e, const void* X, const float* amax, const int8_t* Wt, float* P, int M, int N, int K) {
    SkinnyArgs a = skinny_args((const bf16_t*)X, K, (const bf16_t*)Wt, P, M, N, K, skinny_pick_ksplit_i8(N, K), DT_BF16); a.i8 = 1; a.x_amax = amax;
    launch_skinny(a, e->st);
    return a.ksplit;
}
// a token step's attention for layer l: the q|k|v slabs -> satt, RoPE + KV append fused into the kernel
static DecodeAttnArgs step_attn_args(sonic_engine* e, int l, int ks, int mpad, int dt) {
    const sonic_dims& d = e->d;
    const size_t kvoff = (size_t)l * e->Bm * d.dec_kv_heads * e->max_ctx * d.dec_head_dim;
    return decode_attn_args(e->Kc + kvoff, e->Vc + kvoff, e->slab, nullptr, ks, mpad, e->dec_cs, e->satt, e->kv_len, d.dec_heads, d.dec_kv_heads, e->max_ctx, dt);
}

GreedyArgs greedy_args(sonic_engine* e, int R, bool dump) {
    const sonic_dims& d = e->d;
    GreedyArgs g{};
    g.logits = e->lslab; g.ksplit = skinny_pick_ksplit(d.vocab, d.dec_d); g.mpad = ((R + 15) / 16) * 16; g.V = d.vocab; g.B = R; g.table = e->embed; g.x = e->sx; g.d = d.dec_d;
    g.out_ids = e->out_ids; g.out_lp = e->opt_token_logprobs ? e->out_lp : nullptr; g.out_ld = e->out_cap; g.n_new = e->n_new; g.finished = e->finished; g.kv_len = e->kv_len; g.tok_pos = e->tok_pos;
    g.max_new = e->max_new_d; g.n_active = e->n_active; g.dev_err = e->n_active + 1; g.n_eos = d.n_eos; g.pad_id = d.n_eos > 0 ? d.eos[0] : 0;
    for (int i = 0; i < d.n_eos; ++i) g.eos[i] = d.eos[i];
    g.logits_dump = dump ? e->dump : nullptr; g.dump_stride_step = (long)R * d.vocab; g.step_counter = dump ? e->step_ctr : nullptr;
    g.norm_w = e->dec.empty() ? nullptr : e->dec[0].ln1; g.norm_eps = d.dec_rms_eps; g.y = e->dec.empty() ? nullptr : e->shn;        // the next step's first RMSNorm rides along (d <= 8192)
    g.force_ids = e->force_d; g.force_ld = e->force_ld;
    g.dt = e->dt;
    // (request bias without guards: the guard values are the neutral ones - r * 1.0 and __fdiv_rn(r, 1.0) are exact, n = 0, no suppress list)
    if (hist_on(e)) { g.hist = e->hist; g.hist_ld = e->max_ctx; g.rep_penalty = e->gen_penalty; g.ngram = e->gen_ngram; g.suppress = e->gen_suppress_d; g.n_suppress = (int)e->gen_suppress.size(); }
    if (g.out_lp) g.topk = e->opt_top_logprobs;                  // (the alternatives ride in the log-probability records)
    req_greedy_args(e, g);                                       // the per-request stages' rows (after out_lp and hist: two of them ride on those)
    if (e->i8) g.qo = QuantOut{e->hn_q, d.dec_d, e->sca_hn, e->oc_hn, e->ol_hn, d.dec_d, e->ov_hn};     // layer 0's q/k/v input, quantised
    return g;
}

// The o_proj -> RMSNorm -> gate/up chain of one decoder layer on M rows, att [M][K] -> act [M][ff], residual rows x [.][D] updated in place.  decode_step and
// sonic_test_decode_o_gu both launch it here.  kt_o / kt_gu: the fused kernels' diagnostics slots; the error word of the fused gate/up kernel is the engine's.
//   OGU_FUSED       o_proj + residual add + row sum-of-squares partials (ss) -> gate/up with RMSNorm applied while staging X + SwiGLU: two kernels for four
//   OGU_SPLIT_NORM  33 .. 64 rows: the rows are normalised ONCE by their own small kernel (from the same partials, in the same order: same bits) into hn and gate/up
//                   stages them as they are - 256 blocks each normalising all 64 rows was the longest single piece of the 64-row step
//   OGU_HALF_FUSED  o_proj into slabs -> add+RMSNorm into hn -> gate/up + SwiGLU in one kernel, no slabs
//   OGU_UNFUSED     ... -> gate/up into slabs -> SwiGLU (gu8: the weights' gate / up interleave, launch_swiglu_slab)
void launch_o_gu(sonic_engine* e, int form, const OGuChain& c, int M, int K, int D, int ff, float eps) {
    const int dt = e->dt, mpad = ((M + 15) / 16) * 16;
    if (form == OGU_FUSED || form == OGU_SPLIT_NORM) {
        SkinnyArgs oa = skinny_args(c.att, K, c.Wo, nullptr, M, D, K, 1, dt); oa.kt = c.kt_o;
        launch_skinny_o(oa, c.x, D, c.ss, e->st);
        SkinnyArgs ga = skinny_args(c.x, D, c.Wgu, nullptr, M, 2 * ff, D, 1, dt); ga.kt = c.kt_gu; ga.err = e->n_active + 1;
        if (form == OGU_SPLIT_NORM) {
            launch_rmsnorm_ss(c.x, c.ss, c.ln_w, c.hn, M, D, eps, e->st, dt);
            ga.X = c.hn; launch_skinny_gu(ga, c.act, e->st);
        } else
            launch_skinny_gu_norm(ga, c.act, c.ss, D / 16, c.ln_w, eps, e->st);
        return;
    }
    int ks;
    skinny(e, c.att, K, c.Wo, c.slab, M, D, K, &ks);
    launch_add_rmsnorm(c.x, c.slab, ks, mpad, c.ln_w, c.hn, M, D, eps, e->st, dt);
    if (form == OGU_HALF_FUSED) { launch_skinny_gu(skinny_args(c.hn, D, c.Wgu, nullptr, M, 2 * ff, D, 1, dt), c.act, e->st); return; }
    skinny(e, c.hn, D, c.Wgu, c.slab, M, 2 * ff, D, &ks);
    launch_swiglu_slab(c.slab, ks, mpad, 2 * ff, c.act, M, e->st, dt, c.gu8);
}

// The form of the 16-bit token step for R rows, decided once: the layer loop and step_launches_per_layer read it.
//   gemv        1 - 4 rows, opt-in (decode_gemv): the GEMV chain
//   fuse_gu / fuse_o   the fused gate/up kernel, and the fused o_proj in front of it, take the shape (launch_o_gu's forms)
//   pre         <= 2 rows (the B = 1 call shape of BASELINE configs 1 and 5; round 6): no standalone add+RMSNorm launch behind down_proj - the next q|k|v projection
//               (and, behind the last layer, the lm_head) sums the slabs, adds the residual and normalises its rows itself (skinny_xs_kernel<.., PRE>, the same
//               arithmetic statement by statement: same bits).  down_proj then writes its slabs to slab2 (the consumer writes slab while other blocks of it still
//               read) and the residual stream alternates between sx and sx2
//   split_norm  33 .. 64 rows, on request or inside a continuous loop's graph (gu64_split_norm): OGU_SPLIT_NORM.  Never with pre (rows), so its rows are in sx
struct StepForm { bool gemv, pre, fuse_o, fuse_gu, split_norm; };
static StepForm step_form(sonic_engine* e, int R) {
    const sonic_dims& d = e->d;
    const int D = d.dec_d;
    // wgu_t8 is set for every decoder layer or for none: engine_weights.cpp asks skinny_gu_eligible(1, 2 ff, d) of the model's dims under one lock, the same answer
    // layer after layer (and never in int8 mode) - so layer 0 speaks for all
    const bool gu8 = d.dec_layers > 0 && e->dec[0].wgu_t8;
    StepForm f{};
    f.gemv = e->opt_decode_gemv && R <= GEMV_MAX_ROWS && gu8 && gemv_eligible(R, e->qkvN, D, GEMV_SLAB_NORM) && gemv_eligible(R, D, e->QD, GEMV_RESID) &&
             gemv_eligible(R, 2 * d.dec_ff, D, GEMV_SWIGLU_NORM) && gemv_eligible(R, D, d.dec_ff, GEMV_RESID) && gemv_eligible(R, d.vocab, D, GEMV_SLAB_NORM);
    f.fuse_gu = gu8 && skinny_gu_eligible(R, 2 * d.dec_ff, D);
    f.fuse_o = f.fuse_gu && skinny_o_eligible(R, D, e->QD);
    f.pre = f.fuse_o && !e->opt_no_pre_norm && skinny_pre_eligible(R, e->qkvN, D) && skinny_pre_eligible(R, d.vocab, D) && D % 8 == 0;
    f.split_norm = f.fuse_o && (e->opts.gu64_split_norm > 0 || (e->opts.gu64_split_norm == 0 && e->cap_svc)) && R > 32 && D % 128 == 0 && D <= 2048;
    return f;
}
// 1 - 4 rows, opt-in (gemv.hip): q|k|v (norm inside) -> attention -> o_proj (+ residual) -> gate/up (norm inside, SwiGLU) -> down_proj (+ residual); lm_head (norm inside)
static void decode_step_gemv(sonic_engine* e, int R, bool dump) {
    const sonic_dims& d = e->d;
    const int D = d.dec_d, mpad = ((R + 15) / 16) * 16, dt = e->dt;
    auto gv = [&](int mode, const bf16_t* X, long ldx, const bf16_t* W, int N, int K, const float* nw, float* P, bf16_t* resid, bf16_t* act) {
        GemvArgs g{}; g.X = X; g.ldx = ldx; g.W = W; g.M = R; g.N = N; g.K = K; g.dt = dt; g.norm_w = nw; g.eps = d.dec_rms_eps; g.P = P; g.resid = resid; g.ldr = D; g.act = act;
        launch_gemv(g, mode, e->st);
    };
    for (int l = 0; l < d.dec_layers; ++l) {
        const DecLayerW& L = e->dec[l];
        gv(GEMV_SLAB_NORM, e->sx, D, L.wqkv_t, e->qkvN, D, L.ln1, e->slab, nullptr, nullptr);
        launch_decode_attn(step_attn_args(e, l, 1, mpad, dt), R, e->st);
        gv(GEMV_RESID, e->satt, e->QD, L.wo_t, D, e->QD, nullptr, nullptr, e->sx, nullptr);
        gv(GEMV_SWIGLU_NORM, e->sx, D, L.wgu_t8, 2 * d.dec_ff, D, L.ln2, nullptr, nullptr, e->sact);
        gv(GEMV_RESID, e->sact, d.dec_ff, L.wdown_t, D, d.dec_ff, nullptr, nullptr, e->sx, nullptr);
    }
    gv(GEMV_SLAB_NORM, e->sx, D, e->embed_t, d.vocab, D, e->dec_nw, e->lslab, nullptr, nullptr);
    GreedyArgs g = greedy_args(e, R, dump);
    g.ksplit = 1;
    launch_greedy(g, e->st);
}
// experiment (decode_prefetch bits 0 / 1): the attention launch covers R x Hkv of the 256 CUs - the others stream the weights of the kernels behind it
static void attn_prefetch(sonic_engine* e, const DecLayerW& L, int R, DecodeAttnArgs* da) {
    const sonic_dims& d = e->d;
    if (!(e->opts.decode_prefetch & 3) || R * d.dec_kv_heads > 128 || !L.wo_t) return;
    da->pf_y = (256 - R * d.dec_kv_heads) / R;
    if (e->opts.decode_prefetch & 1) da->pf[0] = PrefetchRange{L.wo_t, (long)d.dec_d * e->QD * 2};
    if ((e->opts.decode_prefetch & 2) && L.wgu_t8) da->pf[1] = PrefetchRange{L.wgu_t8, (long)d.dec_ff * d.dec_d * 2};       // the first half of gate/up (25 MB)
}

// one decode step for R rows: sx ([R][d]) -> next token (generation/utils.py:2876-2943)
static void decode_step(sonic_engine* e, int R, bool dump) {
    if (e->f32) { decode_step_f32(e, R, dump); return; }
    if (e->i8) { decode_step_i8(e, R, dump); return; }
    const sonic_dims& d = e->d;
    const int D = d.dec_d, mpad = ((R + 15) / 16) * 16, dt = e->dt;
    const StepForm f = step_form(e, R);
    const int ogu = !f.fuse_gu ? OGU_UNFUSED : !f.fuse_o ? OGU_HALF_FUSED : f.split_norm ? OGU_SPLIT_NORM : OGU_FUSED;
    e->step_launches_per_layer = f.gemv ? 5 : !f.fuse_o ? 8 : f.pre ? 5 : f.split_norm ? 7 : 6;
    if (f.gemv) { decode_step_gemv(e, R, dump); return; }
    if (D > 8192) launch_rmsnorm(e->sx, e->dec[0].ln1, e->shn, R, D, d.dec_rms_eps, nullptr, e->st, dt);   // else: done by the greedy kernel of the previous step
    bf16_t* resid = e->sx;                               // where the residual rows live right now
    int ks, ks_down = 0;
    auto skinny_pre = [&](const bf16_t* W, float* P, int N, const float* nw, bf16_t* xout, int* ks_out, long long* kt) {
        SkinnyArgs a = skinny_args(resid, D, W, P, R, N, D, skinny_pick_ksplit(N, D), dt); a.kt = kt;
        a.pre_P = e->slab2; a.pre_ks = ks_down; a.pre_mpad = mpad; a.pre_x = resid; a.pre_xout = xout; a.pre_w = nw; a.pre_eps = d.dec_rms_eps;
        if (ks_out) *ks_out = a.ksplit;
        launch_skinny(a, e->st);
    };
    for (int l = 0; l < d.dec_layers; ++l) {
        const DecLayerW& L = e->dec[l];
        if (f.pre && l > 0) {
            bf16_t* other = resid == e->sx ? e->sx2 : e->sx;
            skinny_pre(L.wqkv_t, e->slab, e->qkvN, L.ln1, other, &ks, kt_slot(e, l, 0));
            resid = other;
        } else
            skinny(e, e->shn, D, L.wqkv_t, e->slab, R, e->qkvN, D, &ks, kt_slot(e, l, 0));
        DecodeAttnArgs da = step_attn_args(e, l, ks, mpad, dt); da.kt = kt_slot(e, l, 1);
        attn_prefetch(e, L, R, &da);
        launch_decode_attn(da, R, e->st);
        launch_o_gu(e, ogu, OGuChain{e->satt, L.wo_t, resid, L.ln2, L.wgu_t ? L.wgu_t : L.wgu_t8, L.wgu_t ? 0 : 1, e->shn, e->sact, e->ssq, e->slab, kt_slot(e, l, 2), kt_slot(e, l, 3)},
                    R, e->QD, D, d.dec_ff, d.dec_rms_eps);
        skinny(e, e->sact, d.dec_ff, L.wdown_t, f.pre ? e->slab2 : e->slab, R, D, d.dec_ff, &ks, kt_slot(e, l, 4));
        ks_down = ks;
        if (f.pre) continue;                             // the next layer's q|k|v (or the lm_head) consumes the slabs
        const float* nw = (l + 1 < d.dec_layers) ? e->dec[l + 1].ln1 : e->dec_nw;
        PrefetchRange pfq{nullptr, 0};
        if ((e->opts.decode_prefetch & 4) && l + 1 < d.dec_layers && e->dec[l + 1].wqkv_t) pfq = PrefetchRange{e->dec[l + 1].wqkv_t, (long)e->qkvN * D * 2};
        launch_add_rmsnorm(e->sx, e->slab, ks, mpad, nw, e->shn, R, D, d.dec_rms_eps, e->st, dt, nullptr, nullptr, &pfq, R < 256 ? 256 - R : 0);
    }
    if (f.pre) skinny_pre(e->embed_t, e->lslab, d.vocab, e->dec_nw, nullptr, nullptr, nullptr);   // tied lm_head behind the last layer's slabs (the updated residual is not needed again)
    else skinny(e, e->shn, D, e->embed_t, e->lslab, R, d.vocab, D, nullptr);                    // tied lm_head (modeling_glmasr.py:517)
    launch_greedy(greedy_args(e, R, dump), e->st);
}

// int8 mode (asr.py:169-210): every decoder projection is a Linear8bitLt.  In a decode step each row is one reference call, so its
// outlier "columns" are its own elements >= 6.0.  Producers that own whole rows emit them quantised (greedy / add+RMSNorm / SwiGLU
// kernels; the attention output by its own one-block-per-row pass), the skinny int8 GEMM streams the fragment-tiled int8 weights
// (half the bytes of the bf16 step) into exact int32 slabs, and the consumer dequantises them (int8_util.h deq4).
void decode_step_i8(sonic_engine* e, int R, bool dump) {
    const sonic_dims& d = e->d;
    e->step_launches_per_layer = 8;
    const int D = d.dec_d, FF = d.dec_ff, mpad = ((R + 15) / 16) * 16;
    const QuantOut q_hn{e->hn_q, D, e->sca_hn, e->oc_hn, e->ol_hn, D, e->ov_hn};
    const QuantOut q_att{e->att_q, e->QD, e->sca_att, e->oc_att, e->ol_att, e->QD, e->ov_att};
    const QuantOut q_act{e->act_q, FF, e->sca_act, e->oc_act, e->ol_act, FF, e->ov_act};
    auto deq = [&](const QuantOut& q, const QW& w, int K, const bf16_t* x16, int N) {
        DeqInfo dq{}; dq.sca = q.sca; dq.scb = w.scb; dq.cb = w.cb; dq.cbt = w.cbt; dq.cbk = w.cbk; dq.N = N; dq.K = K; dq.x16 = x16; dq.ldx16 = K; dq.oc_cnt = q.oc_cnt; dq.oc_list = q.oc_list; dq.oc_ld = q.oc_ld;
        dq.row_group = nullptr; dq.group_div = 1; dq.oc_val = q.oc_val; dq.dbg = e->opt_i8_dbg;
        return dq;
    };
    for (int l = 0; l < d.dec_layers; ++l) {
        const DecLayerW& L = e->dec[l];
        int ks = skinny_i8(e, e->hn_q, nullptr, L.qqkv.cbt, e->slab, R, e->qkvN, D);
        DecodeAttnArgs da = step_attn_args(e, l, ks, mpad, DT_F16); da.dq = deq(q_hn, L.qqkv, D, e->shn, e->qkvN);
        // o_proj's input rows are spread over the attention blocks of 4 kv heads: they gather the row absmax (atomicMax), o_proj quantises on the
        // fly and its consumer lists the outliers itself - no one-block-per-row quantisation launch in between (option i8_no_xq: the round-2 form)
        const bool xq = !e->opt_i8_no_xq && d.dec_kv_heads <= 4 && !e->opts.decode_attn_v1;   // the partials are [64][4]: one per kv-head block
        if (xq) { da.amax_out = e->amax_att; da.big_out = e->big_att; }
        launch_decode_attn(da, R, e->st);
        DeqInfo dq;
        if (xq) {
            ks = skinny_i8(e, e->satt, e->amax_att, L.qo.cbt, e->slab, R, D, e->QD);
            dq = deq(q_att, L.qo, e->QD, e->satt, D); dq.sca = e->amax_att; dq.scan = 1; dq.scan_cnt = e->big_att;
        } else {
            launch_quant_rows(e->satt, e->QD, R, e->QD, q_att, e->st);
            ks = skinny_i8(e, e->att_q, nullptr, L.qo.cbt, e->slab, R, D, e->QD);
            dq = deq(q_att, L.qo, e->QD, e->satt, D);
        }
        launch_add_rmsnorm(e->sx, e->slab, ks, mpad, L.ln2, e->shn, R, D, d.dec_rms_eps, e->st, DT_F16, &dq, &q_hn);
        ks = skinny_i8(e, e->hn_q, nullptr, L.qgu.cbt, e->slab, R, 2 * FF, D);
        launch_swiglu_quant(e->slab, ks, mpad, FF, e->sact, R, deq(q_hn, L.qgu, D, e->shn, 2 * FF), q_act, e->st);
        ks = skinny_i8(e, e->act_q, nullptr, L.qdown.cbt, e->slab, R, D, FF);
        dq = deq(q_act, L.qdown, FF, e->sact, D);
        const float* nw = (l + 1 < d.dec_layers) ? e->dec[l + 1].ln1 : e->dec_nw;
        launch_add_rmsnorm(e->sx, e->slab, ks, mpad, nw, e->shn, R, D, d.dec_rms_eps, e->st, DT_F16, &dq, &q_hn);
    }
    skinny(e, e->shn, D, e->embed_t, e->lslab, R, d.vocab, D, nullptr);   // lm_head is not swapped (asr.py:177): fp16 skinny GEMM
    launch_greedy(greedy_args(e, R, dump), e->st);
}

// fan (the parallel forced run's forced_fanout; 1 otherwise): sequence r takes its audio rows from audio request r / fan - req_win then has R / fan + 1 entries
static int plan_requests(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                         const int32_t* max_new, HostPlan& hp, int fan = 1) {
    const sonic_dims& d = e->d;
    const int W = e->W, A = R / fan;
    if (R < 1 || R > e->Bm) return fail(e, SONIC_ERR_INVALID, "request count %d out of range 1..%d", R, e->Bm);
    if (!req_win && A != W) return fail(e, SONIC_ERR_INVALID, "R (%d) must equal staged windows (%d) when req_win is NULL", A, W);
    if (req_win && (req_win[0] != 0 || req_win[A] != W)) return fail(e, SONIC_ERR_INVALID, "req_win must cover exactly the staged windows");
    hp.q_off.resize(R); hp.q_len.resize(R); hp.last_row.resize(R); hp.max_new.resize(R);
    for (int r = 0; r < R; ++r) {
        const int w0 = req_win ? req_win[r / fan] : r / fan, w1 = req_win ? req_win[r / fan + 1] : r / fan + 1;
        if (w1 <= w0) return fail(e, SONIC_ERR_INVALID, "request %d has no audio window", r);
        std::vector<int> rows;  // audio rows of this request in order
        for (int w = w0; w < w1; ++w) {
            const int k = keep_rows(d, frames_of(e->n_samples_h[w]));
            for (int j = 0; j < k; ++j) rows.push_back(w * e->Ta + j);
        }
        const int64_t p0 = prompt_off[r], p1 = prompt_off[r + 1];
        const int P = (int)(p1 - p0);
        if (P < 1) return fail(e, SONIC_ERR_INVALID, "request %d has an empty prompt", r);
        if (max_new[r] < 1) return fail(e, SONIC_ERR_INVALID, "max_new_tokens must be >= 1");
        if (P + max_new[r] > e->max_ctx) return fail(e, SONIC_ERR_INVALID, "prompt (%d) + max_new_tokens (%d) exceeds max_ctx (%d)", P, max_new[r], e->max_ctx);
        if (max_new[r] > e->out_cap) return fail(e, SONIC_ERR_INVALID, "max_new_tokens too large");
        size_t used = 0; int n_ph = 0;
        for (int i = 0; i < P; ++i) n_ph += (prompt_ids[p0 + i] == d.audio_token_id);
        if ((size_t)n_ph != rows.size())
            return fail(e, SONIC_ERR_MISMATCH, "Audio features and audio tokens do not match, tokens: %d, features: %zu", n_ph, rows.size());
        hp.q_off[r] = hp.n_tok; hp.q_len[r] = P;
        for (int i = 0; i < P; ++i) {
            const int id = prompt_ids[p0 + i];
            if (id == d.audio_token_id) hp.src.push_back(-(1 + rows[used++]));
            else {
                if (id < 0 || id >= d.vocab) return fail(e, SONIC_ERR_INVALID, "token id %d out of vocabulary", id);
                hp.src.push_back(id);
            }
            hp.tok_seq.push_back(r); hp.tok_pos.push_back(i);
        }
        hp.n_tok += P;
        hp.last_row[r] = hp.n_tok - 1;
        hp.max_new[r] = max_new[r];
        if (P > hp.max_p) hp.max_p = P;
        if (max_new[r] > hp.max_steps) hp.max_steps = max_new[r];
    }
    if (hp.n_tok > e->tok_cap) return fail(e, SONIC_ERR_INVALID, "too many prompt tokens");
    return SONIC_OK;
}

// The prologue of every kind's prefill.  upload_plan: the request plan goes through pinned memory, so the copies are truly asynchronous and nothing here waits for the
// encoder that is still running on this stream (a pageable source forced a stream synchronise between encoder and prefill: a host-dependent bubble in every batch).
// plan_h = the staging buffer run_to_first_token picked for this run (free: the run that used it last has had its copies waited for).
int upload_plan(sonic_engine* e, int R, const HostPlan& hp) {
    const size_t M = (size_t)hp.n_tok;
    int* h = e->plan_h; size_t o = 0;
    auto put = [&](int* dst, const int* srcv, size_t n) -> hipError_t {
        if (o + n > e->plan_cap) return hipErrorInvalidValue;
        memcpy(h + o, srcv, n * 4);
        hipError_t r = hipMemcpyAsync(dst, h + o, n * 4, hipMemcpyHostToDevice, e->st);
        o += n; return r;
    };
    HIPC(e, put(e->src, hp.src.data(), M)); HIPC(e, put(e->tok_seq, hp.tok_seq.data(), M)); HIPC(e, put(e->tok_pos_pf, hp.tok_pos.data(), M));
    HIPC(e, put(e->q_off, hp.q_off.data(), (size_t)R)); HIPC(e, put(e->q_len, hp.q_len.data(), (size_t)R));
    if (hp.rows > R) {      // row forks: the greedy loop's words for all the rows - a fork's are those of the request it shares its prefill with
        const int Rr = hp.rows;
        std::vector<int> kv((size_t)Rr), last((size_t)Rr), mn((size_t)Rr);
        for (int r = 0; r < Rr; ++r) { const int a = hp.fork_src[r]; kv[r] = hp.q_len[a]; last[r] = hp.last_row[a]; mn[r] = hp.max_new[a]; }
        HIPC(e, put(e->kv_len, kv.data(), (size_t)Rr)); HIPC(e, put(e->last_row, last.data(), (size_t)Rr)); HIPC(e, put(e->max_new_d, mn.data(), (size_t)Rr));
        HIPC(e, put(e->n_active, &Rr, 1));
    } else {
        HIPC(e, put(e->kv_len, hp.q_len.data(), (size_t)R));
        HIPC(e, put(e->last_row, hp.last_row.data(), (size_t)R)); HIPC(e, put(e->max_new_d, hp.max_new.data(), (size_t)R));
        HIPC(e, put(e->n_active, &R, 1));
    }
    if (hp.S > 0) {      // option draft_verify: the verify rows' plan, through the pinned mirror that belongs to this staging buffer
        int* dh = e->draft_plan_h[e->plan_idx];
        memcpy(dh, hp.draft.data(), hp.draft.size() * 4);
        HIPC(e, hipMemcpyAsync(e->draft_plan_d, dh, hp.draft.size() * 4, hipMemcpyHostToDevice, e->st));
    }
    HIPC(e, hipEventRecord(e->plan_ev[e->plan_idx], e->st));       // every copy out of this buffer (win_req included) is older than this event
    e->plan_busy[e->plan_idx] = true;
    return SONIC_OK;
}
// ... and the rows' state for the greedy loop that follows: counters, the int8 step's partials, the guards' history, the requests' bias tables and sampling values
int reset_row_state(sonic_engine* e, int R, int n_tok) {
    launch_fill_i32(e->n_new, 0, 64, e->st);
    if (e->amax_att) { launch_fill_i32((int*)e->amax_att, 0, 64 * 4, e->st); launch_fill_i32((int*)e->amax_act, 0, 64 * 4, e->st); launch_fill_i32(e->big_att, 0, 64 * 4, e->st); }   // (partials nobody writes stay 0)
    launch_fill_i32(e->finished, 0, 64, e->st);
    launch_fill_i32(e->step_ctr, 0, 64, e->st);
    if (hist_on(e)) launch_hist_prompt(e->src, e->tok_seq, e->tok_pos_pf, n_tok, e->d.audio_token_id, e->hist, e->max_ctx, e->st);    // the rows' input_ids for the guards / the request bias
    return req_upload(e, R);                                                                                                        // every request's claimed values, or the neutral ones, into its row
}

// Draft-verified decoding (option draft_verify), behind the prefill's last layer: draft position n of request r is decided by the hidden row at
// q_off[r] + P - 1 + n.  The S = sum D_r rows are normalised with the final norm into dhn (free behind the last layer), then, in chunks of score_chunk_rows, multiplied
// by the tied lm_head as one prefill-family GEMM into score_logits and reduced by verify_rows_kernel under the handle's processors; draft_accept_kernel then leaves
// every drafted request where a prefill of prompt || draft[0 .. a) would have left it.  The head that follows is the one of every prefill
static void run_draft_verify(sonic_engine* e, int R, const HostPlan& hp) {
    const sonic_dims& d = e->d;
    const int S = hp.S;
    const int* pd = e->draft_plan_d;
    launch_rmsnorm(e->dx, e->dec_nw, e->dhn, S, d.dec_d, d.dec_rms_eps, pd, e->st, e->dt);
    VerifyArgs va{};
    va.logits = e->score_logits; va.ld = d.vocab; va.V = d.vocab; va.dt = e->dt;
    if (e->gen_on && e->hist) { va.hist = e->hist; va.hist_ld = e->max_ctx; va.rep_penalty = e->gen_penalty; va.ngram = e->gen_ngram; va.suppress = e->gen_suppress_d; va.n_suppress = (int)e->gen_suppress.size(); }
    va.ver_tok = e->ver_tok; va.ver_rec = e->ver_rec; va.topk = (e->opt_token_logprobs && e->out_lp) ? e->opt_top_logprobs : 0;
    va.dump = e->run_logits ? e->dump : nullptr; va.out_ld = e->out_cap; va.R = R;
    const int chunk = std::min(e->opt_score_chunk_rows, e->score_rows_cap);
    for (int c0 = 0; c0 < S; c0 += chunk) {
        const int n = std::min(chunk, S - c0);
        gemm(e, EPI_BIAS, e->dhn + (size_t)c0 * d.dec_d, d.dec_d, e->embed_t, nullptr, (bf16_t*)e->score_logits, d.vocab, n, d.vocab, d.dec_d, nullptr, 0, 1);   // embed_t: launch_tile_weights' tiling, the one GemmArgs.w_tiled reads
        va.n = n; va.target = pd + S + c0; va.rec = pd + 2 * S + c0; va.hrow = pd + 3 * S + c0; va.hlen = pd + 4 * S + c0;
        va.ver_tok = e->ver_tok + c0; va.ver_rec = e->ver_rec + (size_t)c0 * lp_width(e);
        launch_verify_rows(va, e->st);
    }
    DraftAcceptArgs da{};
    da.req = pd + 5 * S; da.draft = pd + S; da.ver_tok = e->ver_tok; da.ver_rec = e->ver_rec; da.lp_w = lp_width(e);
    da.out_ids = e->out_ids; da.out_lp = (e->opt_token_logprobs && e->out_lp) ? e->out_lp : nullptr; da.out_ld = e->out_cap;
    da.n_new = e->n_new; da.kv_len = e->kv_len; da.tok_pos = e->tok_pos; da.step_counter = e->step_ctr; da.last_row = e->last_row; da.accepted = e->draft_acc;
    launch_draft_accept(da, R, e->st);
}

// Row forks: fork_kv_kernel's descriptor from the row -> request map of a forked prefill - per forked request its row, its first fork's row and
// its forks' count (the forks of a request are consecutive rows).  The map comes from fork_claim, which has checked the rows against the handle's
ForkArgs fork_args(sonic_engine* e, int R, const std::vector<int>& fork_src) {
    const sonic_dims& d = e->d;
    ForkArgs a{};
    a.Kc = e->Kc; a.Vc = e->Vc; a.layers = d.dec_layers; a.Bm = e->Bm; a.Hkv = d.dec_kv_heads; a.ctx = e->max_ctx; a.hd = d.dec_head_dim;
    a.kv_len = e->kv_len; a.hist = hist_on(e) ? e->hist : nullptr;
    for (int r = R; r < (int)fork_src.size() && r < e->Bm; ++r) {
        if (a.n_src > 0 && a.src[a.n_src - 1] == fork_src[r]) { a.cnt[a.n_src - 1] += 1; continue; }
        a.src[a.n_src] = fork_src[r]; a.first[a.n_src] = r; a.cnt[a.n_src] = 1; a.n_src += 1;
    }
    return a;
}

// head = false (the parallel forced run): the decoder layers only - its score rows are normalised and multiplied by run_forced_parallel
static int run_prefill(sonic_engine* e, int R, const HostPlan& hp, bool head = true) {
    const sonic_dims& d = e->d;
    const int D = d.dec_d, M = hp.n_tok, dt = e->dt;
    const QGroup grp{e->tok_seq, 1, R};        // one reference call = the prompt rows of one request
    const int Rr = hp.rows > R ? hp.rows : R;      // row forks: the rows of the run; the decoder layers below run over the R requests
    TRY(upload_plan(e, R, hp));
    TRY(reset_row_state(e, Rr, M));
    launch_assemble_embeds(e->src, e->embed, e->pe, e->dx, M, D, e->st);
    e->last_ntok = M;
    if (e->taps_on) {
        if (!e->taps) HIPC(e, hipMalloc((void**)&e->taps, (size_t)(d.dec_layers + 1) * e->tok_cap * D * sizeof(bf16_t)));
        HIPC(e, hipMemcpyAsync(e->taps, e->dx, (size_t)M * D * 2, hipMemcpyDeviceToDevice, e->st));
    }
    for (int l = 0; l < d.dec_layers; ++l) {
        const DecLayerW& L = e->dec[l];
        const size_t kvoff = (size_t)l * e->Bm * d.dec_kv_heads * e->max_ctx * d.dec_head_dim;
        // 16-bit modes: the prefill GEMMs read the decode step's fragment-tiled weights (GemmArgs.w_tiled) - one copy of every decoder projection
        // since round 5 (the row-major ones are freed at load unless SONIC_KEEP_ROWMAJOR=1; option prefill_rowmajor then selects them for the A/B)
        auto lin = [&](int epi, const bf16_t* X, long ldx, const bf16_t* w16, const bf16_t* wt, int gu8, const QW& q, bf16_t* C, long ldc, int N, int K,
                       const bf16_t* Rr, long ldr, bool pq) {
            if (!e->i8 && wt && (!w16 || !e->opt_prefill_rowmajor)) gemm(e, epi, X, ldx, wt, nullptr, C, ldc, M, N, K, Rr, ldr, 1, gu8);
            else qlinear(e, epi, X, ldx, w16, q, nullptr, C, ldc, M, N, K, Rr, ldr, grp, nullptr, 0, 0, pq);
        };
        const bool pq1 = rmsnorm_q(e, e->dx, L.ln1, e->dhn, M, D, d.dec_rms_eps, grp);
        lin(EPI_BIAS, e->dhn, D, L.wqkv, L.wqkv_t, 0, L.qqkv, e->dqkv, e->qkvN, e->qkvN, D, nullptr, 0, pq1);
        const bool tiles = !e->opt_no_rope_tiles;
        launch_rope_append(rope_append_args(e->dqkv, e->dq, e->Kc + kvoff, e->Vc + kvoff, e->Vts, e->max_ctx, e->tok_seq, e->tok_pos_pf, e->dec_cs, d.dec_heads, d.dec_kv_heads,
                                            e->max_ctx, M, dt, tiles ? e->q_off : nullptr, e->q_len, R, hp.max_p), false, e->st);
        if (e->align_live && !e->align_layer_heads[l].empty()) {      // word timestamps: dq and this layer's K cache are valid here, and only here
            const AlignArgs aa = align_probs_args(e, e->dq, e->Kc + kvoff, 128, e->max_ctx * 128L, (long)d.dec_kv_heads * e->max_ctx * 128, e->align_plan_d + 2 * (size_t)e->tok_cap + 4 * 64 + e->align_layer_off[l],
                                                  (int)e->align_layer_heads[l].size(), d.dec_heads, d.dec_kv_heads, nullptr);
            launch_align_probs(aa, e->st);
            launch_align_reduce(aa, e->st);
            e->align_last_heads = aa.n_heads;
        }
        const FlashArgs f = prefill_flash_args(e->dq, e->Kc + kvoff, e->Vts, e->datt, e->q_off, e->q_len, e->q_len, d.dec_heads, d.dec_kv_heads, e->max_ctx, dt);
        launch_flash(f, 128, true, R, hp.max_p, e->st);
        lin(EPI_BIAS_RESID, e->datt, e->QD, L.wo, L.wo_t, 0, L.qo, e->dx, D, D, e->QD, e->dx, D, false);
        const bool pq2 = rmsnorm_q(e, e->dx, L.ln2, e->dhn, M, D, d.dec_rms_eps, grp);
        lin(EPI_SWIGLU, e->dhn, D, L.wgu, L.wgu_t8 ? L.wgu_t8 : L.wgu_t, L.wgu_t8 ? 1 : 0, L.qgu, e->dact, d.dec_ff, 2 * d.dec_ff, D, nullptr, 0, pq2);
        lin(EPI_BIAS_RESID, e->dact, d.dec_ff, L.wdown, L.wdown_t, 0, L.qdown, e->dx, D, D, d.dec_ff, e->dx, D, false);
        if (e->taps_on) HIPC(e, hipMemcpyAsync(e->taps + (size_t)(l + 1) * e->tok_cap * D, e->dx, (size_t)M * D * 2, hipMemcpyDeviceToDevice, e->st));
    }
    if (!head) return SONIC_OK;
    if (hp.S > 0) run_draft_verify(e, R, hp);      // option draft_verify: the rows' state becomes that of a prefill of prompt || accepted draft, last_row included
    if (Rr > R) {      // row forks: every forked request's K / V (and history) into its forks' rows, once, ahead of the head
        const ForkArgs fa = fork_args(e, R, hp.fork_src);
        if (e->fork_ev[0]) (void)hipEventRecord(e->fork_ev[0], e->st);
        launch_fork_kv(fa, hp.max_p, e->st);
        if (e->fork_ev[1]) { (void)hipEventRecord(e->fork_ev[1], e->st); e->fork_timed = true; }
    }
    // logits only for the last prompt position of each request (logits_to_keep=1, generation/utils.py:2612-2616); a fork's row reads its request's position (last_row)
    launch_rmsnorm(e->dx, e->dec_nw, e->shn, Rr, D, d.dec_rms_eps, e->last_row, e->st, dt);
    skinny(e, e->shn, D, e->embed_t, e->lslab, Rr, d.vocab, D, nullptr);
    return SONIC_OK;
}

// log-mel -> encoder -> projector -> prefill -> first greedy token (generation/utils.py:2612-2616, 2876-2943 for the first step)
int run_to_first_token(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                       const int32_t* max_new, bool want_logits) {
    const sonic_dims& d = e->d;
    if (!e->finalized) return fail(e, SONIC_ERR_INVALID, "weights not finalized");
    if (e->W < 1) return fail(e, SONIC_ERR_INVALID, "no PCM staged");
    if (e->svc_on) return fail(e, SONIC_ERR_INVALID, "this handle is decoding continuously (sonic_service_begin): prefill on another slot and splice the rows in");
    if (e->wait_pending) {                                  // rows of the previous batch were spliced into another handle: its copy kernels read this
        HIPC(e, hipStreamWaitEvent(e->st, e->wait_ev, 0));  // engine's KV cache and row state, which this run is about to overwrite
        e->wait_pending = false;
    }
    std::vector<int> fork_src;      // row forks (sonic_load_tensor "request_forks"): the row -> request map of a forked batch (empty: the requests are the rows)
    TRY(fork_claim(e, R, fork_src));
    const int Rr = fork_src.empty() ? R : (int)fork_src.size();      // the rows of the run: what the per-request stages, the head and the greedy loop count
    TRY(req_claim(e, Rr, Rr > R));      // sonic_set_request_bias / _sampling / option request_grammar: this batch consumes what they left whatever becomes of it (ENTER_CONSUME drops it on every other exit)
    HostPlan hp;
    if (R < 1 || R > e->Bm) return fail(e, SONIC_ERR_INVALID, "request count %d out of range 1..%d", R, e->Bm);
    std::vector<int32_t> x_ids, x_left; std::vector<int64_t> x_off; std::vector<int> dlen;      // option draft_verify: the longer sequences prompt || draft (empty dlen: no draft in this batch)
    TRY(draft_extend(e, R, prompt_ids, prompt_off, max_new, x_ids, x_off, x_left, dlen));
    if (dlen.empty()) TRY(plan_requests(e, req_win, R, prompt_ids, prompt_off, max_new, hp));
    else {
        TRY(plan_requests(e, req_win, R, x_ids.data(), x_off.data(), x_left.data(), hp));
        hp.max_steps = 0;
        for (int r = 0; r < R; ++r) { hp.max_new[r] = max_new[r]; hp.max_steps = std::max(hp.max_steps, (int)max_new[r]); hp.S += dlen[r]; }
        TRY(draft_alloc(e));
        // the verify rows (draft_plan_d's layout): hidden row | draft id | record index | request | history length, S of each; then per request D | first row | P | first token
        const int S = hp.S;
        hp.draft.assign((size_t)5 * S + 4 * 64, 0);
        int* w = hp.draft.data(); int* rq = w + (size_t)5 * S;
        for (int r = 0, s = 0; r < R; ++r) {
            const int P = hp.q_len[r] - dlen[r];
            rq[r] = dlen[r]; rq[64 + r] = s; rq[128 + r] = P; rq[192 + r] = hp.q_off[r];
            for (int n = 0; n < dlen[r]; ++n, ++s) { w[s] = hp.q_off[r] + P - 1 + n; w[S + s] = x_ids[(size_t)x_off[r] + P + n]; w[2 * S + s] = r * e->out_cap + n; w[3 * S + s] = r; w[4 * S + s] = P + n; }
        }
    }
    e->draft_last_S = hp.S;
    e->fork_timed = false;
    if (Rr > R) {
        if (d.dec_head_dim % 8) return fail(e, SONIC_ERR_INVALID, "request_forks: a head dimension of %d is not a multiple of 8 elements (the copy moves 16-byte pieces)", d.dec_head_dim);
        hp.rows = Rr; hp.fork_src = fork_src;
        for (int i = 0; i < 2; ++i) if (!e->fork_ev[i]) HIPC(e, hipEventCreate(&e->fork_ev[i]));
    }
    {   // staging buffer of this run: the one used two runs ago; its copies are almost always long done (a blocking wait otherwise)
        const int i = e->plan_idx ^ 1;
        if (e->plan_busy[i]) { HIPC(e, hipEventSynchronize(e->plan_ev[i])); e->plan_busy[i] = false; }
        e->plan_idx = i; e->plan_h = e->plan_buf[i];
    }
    if (e->force_d && (e->force_R != R || e->force_ld < hp.max_steps))
        return fail(e, SONIC_ERR_INVALID, "forced ids are [%d][%d] but the run has %d requests / %d steps", e->force_R, e->force_ld, R, hp.max_steps);
    e->R = Rr; e->max_steps = hp.max_steps; e->last_qlen = hp.q_len; e->last_maxnew = hp.max_new; e->align_last = false;
    for (size_t r = 0; r < dlen.size(); ++r) e->last_qlen[r] -= dlen[r];      // the PROMPT's length: fetch_locked expects kv_len = prompt + tokens - 1
    for (int r = R; r < Rr; ++r) { e->last_qlen.push_back(hp.q_len[fork_src[r]]); e->last_maxnew.push_back(hp.max_new[fork_src[r]]); }      // (a fork's invariants are its request's)
    if (want_logits) {
        // a drafted row's step counter starts at its accepted count and goes on counting with every launch, also once the row has ended: the dump holds the steps
        // the longest draft can add (the fetch reads the first max_steps of them, as always)
        int d_max = 0;
        for (int D : dlen) d_max = std::max(d_max, D);
        const size_t need_n = (size_t)(hp.max_steps + d_max) * Rr * d.vocab;
        if (need_n > e->dump_cap) {
            if (e->dump) (void)hipFree(e->dump);
            e->dump = nullptr; e->dump_cap = 0;
            HIPC(e, hipMalloc((void**)&e->dump, need_n * 4));
            e->dump_cap = need_n;
        }
        e->dump_steps = hp.max_steps;
    } else e->dump_steps = 0;
    e->run_logits = want_logits;

    (void)hipEventRecord(e->ev[0], e->st);
    TRY(run_mel(e, e->W, e->f32));
    (void)hipEventRecord(e->ev[1], e->st);
    if (e->i8) {   // window -> request map (int8 mode: outlier columns are found per request); pinned: the last 64 words of plan_h, beyond what upload_plan uses
        int* h = e->plan_h + e->plan_cap - 64;
        memset(h, 0, 64 * 4);
        for (int r = 0; r < R; ++r) {
            const int w0 = req_win ? req_win[r] : r, w1 = req_win ? req_win[r + 1] : r + 1;
            for (int w = w0; w < w1 && w < 64; ++w) h[w] = r;
        }
        HIPC(e, hipMemcpyAsync(e->win_req, h, 64 * 4, hipMemcpyHostToDevice, e->st));
    }
    TRY(e->f32 ? f32_run_encoder(e, e->W, nullptr, nullptr) : run_encoder(e, e->W, nullptr, nullptr, R));
    (void)hipEventRecord(e->ev[2], e->st);
    TRY(e->f32 ? f32_run_prefill(e, R, hp) : run_prefill(e, R, hp));
    launch_greedy(e->f32 ? f32_greedy_args(e, Rr, want_logits) : greedy_args(e, Rr, want_logits), e->st);
    (void)hipEventRecord(e->ev[3], e->st);
    e->steps_run = 0; e->greedy_calls = 1; e->spliced = 0;
    return SONIC_OK;
}

// A captured chunk of the greedy loop: `n` token steps for `R` rows as ONE hipGraph (kv_len / tok_pos / the token ids live on the device, so
// the steps of a chunk need nothing from the host).
// svc: the chunk belongs to a continuous decode loop (sonic_service_*), i.e. it runs beside a prefill slot and other loops by design - decode_step then
// picks the forms that cost the fewest CU-microseconds rather than the shortest chain (gu64_split_norm).  Same bits either way; cached separately.
int chunk_graph(sonic_engine* e, int R, int n, hipGraphExec_t* out, bool svc) {
    const std::pair<int, int> key{R + (svc ? 4096 : 0) + (e->opt_token_logprobs ? 8192 : 0) + (e->gen_on ? 16384 : 0) + e->opt_top_logprobs * 131072 + req_graph_key(e), n};   // (the LP / GUARD / BIAS / SAMPLE / TOPK / GRAMMAR greedy kernel and its pointers are part of the capture)
    auto it = e->graphs.find(key);
    if (it != e->graphs.end()) { *out = it->second; return SONIC_OK; }
    hipGraph_t g = nullptr; hipGraphExec_t gx = nullptr;
    HIPC(e, hipStreamBeginCapture(e->st, hipStreamCaptureModeThreadLocal));
    e->cap_svc = svc;
    for (int i = 0; i < n; ++i) decode_step(e, R, false);
    e->cap_svc = false;
    HIPC(e, hipStreamEndCapture(e->st, &g));
    hipError_t r = hipGraphInstantiate(&gx, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIPC(e, r);
    e->graphs[key] = gx;
    *out = gx;
    return SONIC_OK;
}

// up to n_steps further token steps of the staged batch (HF:generation/utils.py:2876-2943), in chunks of `decode_chunk` steps: one hipGraph
// launch per chunk (eager under teacher forcing / when the step logits are wanted; a launch costs the host ~4 us, tools/host_cost.py).
// Ragged termination without a host round trip on the critical path: behind every chunk the device's count of running rows is copied to
// pinned memory and an event is recorded; the host reads check k only when chunk k + lookahead is already queued, so the stream never runs
// dry while the host looks, and the loop stops `lookahead` chunks after every row hit EOS / its budget (finished rows are frozen: the
// queued steps rewrite their own cache slot and emit nothing).  lookahead ADAPTS: it is 1 on a host that keeps up (waste at a stop: one
// chunk) and doubles whenever the host, about to launch the next chunk, finds the one it queued last already complete - the stream is empty,
// the device idle: a host that is descheduled for tens of milliseconds at a time (CPU quota shared with other work) or simply behind (a busy
// interpreter) - up to CHK_MAX_AHEAD chunks; a batch without such an observation takes one chunk off again.
int run_decode_steps(sonic_engine* e, int n_steps, int* done_out) {
    const int R = e->R, left = e->max_steps - 1 - e->steps_run;
    if (n_steps > left) n_steps = left;
    const bool want_logits = e->run_logits;
    const bool use_graph = !want_logits && !e->opt_no_graph && !e->force_d && !e->f32;
    const int C = e->opt_decode_chunk > 0 ? e->opt_decode_chunk : 1;
    int done = 0;
    int launched = 0, checked = 0, last_grow = 0;   // chunks queued with a check behind them / checks the host has read
    bool all_stopped = false, starved = false, dev_err = false;
    typedef std::chrono::steady_clock clk;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    auto read_check = [&](bool block) -> int {  // 1: read (all_stopped updated), 0: not complete yet, < 0: error
        const int i = checked % CHK_RING;
        if (!block) { const hipError_t q = hipEventQuery(e->chk_ev[i]); if (q == hipErrorNotReady) { (void)hipGetLastError(); return 0; } if (q != hipSuccess) return -1; }
        else { const auto t_w = clk::now(); if (hipEventSynchronize(e->chk_ev[i]) != hipSuccess) return -1; e->host_wait_ms += ms_since(t_w); }
        if (e->n_active_h[i] <= 0) all_stopped = true;
        if (e->n_active_h[i] < DEV_ERR_ACTIVE) dev_err = true;
        ++checked;
        return 1;
    };
    while (done < n_steps && !all_stopped) {
        const int n = n_steps - done < C ? n_steps - done : C;
        // The chunk queued last is already complete as the next one is about to go out: the stream is empty, the device has been idle since -
        // this thread is late by more than a chunk (descheduled, or behind other host work).  Keep more chunks queued.
        if (launched > 0 && hipEventQuery(e->chk_ev[(launched - 1) % CHK_RING]) == hipSuccess) {
            if (launched - last_grow > e->lookahead && e->lookahead < CHK_MAX_AHEAD) {      // (the deeper queue gets `lookahead` launches to show before it grows again)
                e->lookahead = e->lookahead * 2 < CHK_MAX_AHEAD ? e->lookahead * 2 : CHK_MAX_AHEAD;
                last_grow = launched;
            }
            starved = true;
        }
        (void)hipGetLastError();
        const auto t_l = clk::now();
        if (use_graph) {
            hipGraphExec_t gx = nullptr;
            TRY(chunk_graph(e, R, n, &gx));
            HIPC(e, hipGraphLaunch(gx, e->st));
        } else {
            for (int i = 0; i < n; ++i) decode_step(e, R, want_logits);
        }
        e->host_launch_ms += ms_since(t_l); e->host_launches += 1;
        done += n; e->steps_run += n; e->greedy_calls += n;
        if (e->steps_run + 1 >= e->max_steps) break;           // the budget is exhausted: nothing left to stop early
        const int slot = launched % CHK_RING;
        HIPC(e, hipMemcpyAsync(e->n_active_h + slot, e->n_active, 4, hipMemcpyDeviceToHost, e->st));
        HIPC(e, hipEventRecord(e->chk_ev[slot], e->st));
        ++launched;
        (void)hipGetLastError();
        while (!all_stopped && checked < launched) {           // read what is there; block only for checks older than the lookahead
            const int r = read_check(launched - checked > e->lookahead);
            if (r < 0) return fail(e, SONIC_ERR_HIP, "decode loop: check event failed: %s", hipGetErrorString(hipGetLastError()));
            if (r == 0) break;
        }
    }
    e->run_starved = e->run_starved || starved;
    if (dev_err) return fail(e, SONIC_ERR_HIP, "a decode kernel gave up on an in-kernel wait: the batch's tokens are invalid");
    if (!all_stopped && done >= n_steps && e->steps_run + 1 < e->max_steps) {
        // the caller asked for fewer steps than the budget (sonic_decode_step) and synchronises next: read the outstanding checks now
        while (!all_stopped && checked < launched) if (read_check(true) < 0) return fail(e, SONIC_ERR_HIP, "decode loop: check event failed");
    }
    if (all_stopped) e->steps_run = e->max_steps - 1;
    if (done_out) *done_out = done;
    return SONIC_OK;
}

// what every whole-batch run ends with: the stage times from the events and the decode loop's host figures
static void fill_timings(sonic_engine* e, double host_enqueue_first, int steps_done) {
    const sonic_dims& d = e->d;
    sonic_timings& t = e->tim;
    memset(&t, 0, sizeof t);
    (void)hipEventElapsedTime(&t.mel_ms, e->ev[0], e->ev[1]);
    (void)hipEventElapsedTime(&t.encoder_ms, e->ev[1], e->ev[2]);
    (void)hipEventElapsedTime(&t.prefill_ms, e->ev[2], e->ev[3]);
    (void)hipEventElapsedTime(&t.decode_ms, e->ev[3], e->ev[4]);
    (void)hipEventElapsedTime(&t.total_ms, e->ev[0], e->ev[4]);
    for (int l = 0; l < e->gemm_ev_used; ++l) {
        float ms = 0; (void)hipEventElapsedTime(&ms, e->gemm_ev[8 * l + 4], e->gemm_ev[8 * l + 5]);
        t.gemm_ms += ms; t.gemm_launches += 1;
        const double MT = (double)e->W * e->T, C = d.enc_d, F = d.enc_ff;
        t.gemm_flops += 2.0 * MT * F * C;
        for (int g = 0; g < 4; ++g) { float m2 = 0; (void)hipEventElapsedTime(&m2, e->gemm_ev[8 * l + 2 * g], e->gemm_ev[8 * l + 2 * g + 1]); t.enc_gemm_ms += m2; }
        t.enc_gemm_flops += 2.0 * MT * C * (3 * C) + 2.0 * MT * C * C + 4.0 * MT * F * C;      // QKV, o, fc1, fc2
    }
    t.decode_steps = steps_done;
    t.host_prefill_enqueue_ms = (float)host_enqueue_first; t.host_decode_launch_ms = (float)e->host_launch_ms; t.host_decode_wait_ms = (float)e->host_wait_ms;
    t.host_decode_launches = e->host_launches; t.decode_lookahead = e->lookahead; t.decode_launches_per_layer = e->step_launches_per_layer;
}

// the parallel forced run's buffers, at the first such run of the handle or when score_chunk_rows has grown since: the chunk's logits
// [score_chunk_rows][vocab] in the activation type (fp32 kind: fp32) and the score rows' plan (3 words per row, at most tok_cap rows) on the device and pinned
int score_logits_alloc(sonic_engine* e) {
    const int rows = e->opt_score_chunk_rows;
    const size_t esz = e->f32 ? 4 : 2;
    if (e->score_logits && e->score_rows_cap < rows) {
        unsigned char* p = (unsigned char*)e->score_logits;
        TRY(dfree(e, &p, (size_t)e->score_rows_cap * e->d.vocab * esz));
        e->score_logits = nullptr; e->score_rows_cap = 0;
    }
    if (!e->score_logits) {
        unsigned char* p = nullptr;
        TRY(dalloc(e, &p, (size_t)rows * e->d.vocab * esz, false));
        e->score_logits = p; e->score_rows_cap = rows;
    }
    return SONIC_OK;
}
static int score_alloc(sonic_engine* e) {
    TRY(score_logits_alloc(e));
    if (!e->score_plan_d) TRY(dalloc(e, &e->score_plan_d, (size_t)3 * e->tok_cap));
    if (!e->score_plan_h && hipHostMalloc((void**)&e->score_plan_h, ((size_t)3 * e->tok_cap + 4 * 64) * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(e, SONIC_ERR_OOM, "forced_parallel: pinned host memory exhausted"); }
    return SONIC_OK;
}
// word timestamps (option forced_align): the align run's buffers, at its first run on the handle or when a run needs more than the last one left.
// S score rows (<= tok_cap), A_max audio keys of the longest run, heads_per_layer the most heads any layer contributes
template <typename Tt> static int align_grow(sonic_engine* e, Tt** p, size_t* cap, size_t need) {
    if (*p && *cap >= need) return SONIC_OK;
    if (*p) { TRY(dfree(e, p, *cap)); *cap = 0; }
    TRY(dalloc(e, p, need, false));
    *cap = need;
    return SONIC_OK;
}
int align_alloc(sonic_engine* e, int S, int A_max, int heads_per_layer) {
    size_t tcap = e->align_M_cap;
    TRY(align_grow(e, &e->align_P, &e->align_P_cap, (size_t)2 * heads_per_layer * S * A_max));      // probabilities | filtered z
    e->align_Zoff = (size_t)heads_per_layer * S * A_max;
    TRY(align_grow(e, &e->align_trace, &tcap, (size_t)S * A_max));
    TRY(align_grow(e, &e->align_M, &e->align_M_cap, (size_t)S * A_max));
    if (!e->align_t) TRY(dalloc(e, &e->align_t, (size_t)64 * e->out_cap));
    const size_t plan = (size_t)2 * e->tok_cap + 4 * 64 + ALIGN_MAX_HEADS;
    if (!e->align_plan_d) { TRY(dalloc(e, &e->align_plan_d, plan)); e->align_plan_cap = plan; }
    if (!e->align_plan_h && hipHostMalloc((void**)&e->align_plan_h, plan * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(e, SONIC_ERR_OOM, "forced_align: pinned host memory exhausted"); }
    return SONIC_OK;
}
// The parallel forced run (option forced_parallel with forced ids set; include/sonic_hip.h beside sonic_set_forced_ids).  Under teacher forcing no
// input depends on an output, so the run is ONE prefill: sequence r = prompt || forced[r][0 .. L_r - 1), L_r = 1 + the index of the first EOS id among its budget's
// forced ids (HF's rule; the budget if there is none).  Token n of sequence r is scored by the hidden state at row q_off[r] + P - 1 + n: the S = sum L_r score rows are
// normalised with the final norm into dhn (free behind the last layer), then, in chunks of score_chunk_rows, multiplied by the tied lm_head as one prefill-family
// GEMM into score_logits and reduced by score_rows_kernel (score.hip), which also writes the forced ids to out_ids and, if asked, the rows to the step-logits dump.
// No logits processor is applied.  forced_fanout = N: the R sequences are R / N audio requests (windows, log-mel, encoder, projector once each) with N candidates
// each; the prefill's outlier groups stay per sequence.  The handle is left holding a finished batch.
static int run_forced_parallel(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new, bool want_logits) {
    const sonic_dims& d = e->d;
    const auto t_host0 = std::chrono::steady_clock::now();
    if (!e->finalized) return fail(e, SONIC_ERR_INVALID, "weights not finalized");
    if (e->W < 1) return fail(e, SONIC_ERR_INVALID, "no PCM staged");
    if (e->svc_on) return fail(e, SONIC_ERR_INVALID, "this handle is decoding continuously (sonic_service_begin): prefill on another slot and splice the rows in");
    if (const char* staged = req_claim_none(e))      // consumed, as on every other exit
        return fail(e, SONIC_ERR_INVALID, "forced_parallel: the parallel forced run applies no processors: the staged %s are refused (it scores the raw distribution; run with the option off to force step by step under them)", staged);
    const int N = e->opt_forced_fanout;
    if (R < 1 || R > e->Bm) return fail(e, SONIC_ERR_INVALID, "request count %d out of range 1..%d", R, e->Bm);
    if (R % N) return fail(e, SONIC_ERR_INVALID, "forced_fanout: %d sequences are not a multiple of the fan-out %d", R, N);
    int max_steps = 0;
    for (int r = 0; r < R; ++r) {
        if (max_new[r] < 1) return fail(e, SONIC_ERR_INVALID, "max_new_tokens must be >= 1");
        max_steps = std::max(max_steps, (int)max_new[r]);
    }
    if (e->force_R != R || e->force_ld < max_steps || e->force_h.size() != (size_t)e->force_R * e->force_ld)
        return fail(e, SONIC_ERR_INVALID, "forced ids are [%d][%d] but the run has %d requests / %d steps", e->force_R, e->force_ld, R, max_steps);
    // the longer sequences: prompt || forced[0 .. L - 1); their budget max_new - (L - 1) keeps plan_requests' context check at prompt + max_new
    std::vector<int32_t> ids, left(R), L(R); std::vector<int64_t> off(R + 1, 0);
    long asked = 0;
    for (int r = 0; r < R; ++r) {
        const int* f = e->force_h.data() + (size_t)r * e->force_ld;
        int l = max_new[r];
        for (int n = 0; n < max_new[r]; ++n) {
            bool eos = false;
            for (int k = 0; k < d.n_eos; ++k) eos = eos || f[n] == d.eos[k];
            if (eos) { l = n + 1; break; }
        }
        for (int n = 0; n < l; ++n)
            if (f[n] == d.audio_token_id) return fail(e, SONIC_ERR_INVALID, "forced_parallel: forced id %d of sequence %d is the audio placeholder id %d, which cannot be a target", n, r, d.audio_token_id);
        const int64_t p0 = prompt_off[r], p1 = prompt_off[r + 1];
        if (p1 - p0 < 1) return fail(e, SONIC_ERR_INVALID, "request %d has an empty prompt", r);
        ids.insert(ids.end(), prompt_ids + p0, prompt_ids + p1);
        ids.insert(ids.end(), f, f + l - 1);
        off[r + 1] = (int64_t)ids.size(); L[r] = l; left[r] = max_new[r] - (l - 1);
        asked += (p1 - p0) + l - 1;
    }
    if (asked > e->tok_cap) return fail(e, SONIC_ERR_INVALID, "forced_parallel: the run asks for %ld tokens (prompts and forced ids), %d fit one prefill (tok_cap)", asked, e->tok_cap);
    HostPlan hp;
    TRY(plan_requests(e, req_win, R, ids.data(), off.data(), left.data(), hp, N));
    for (int r = 0; r < R; ++r) hp.max_new[r] = max_new[r];
    hp.max_steps = max_steps;
    if (max_steps > e->out_cap) return fail(e, SONIC_ERR_INVALID, "max_new_tokens too large");
    // word timestamps (option forced_align): every sequence's audio placeholders must be one run [a0, a0 + A), A >= 1, inside its prompt
    const bool align = e->opt_forced_align != 0;
    std::vector<int> al_a0(R, 0), al_A(R, 0);
    int al_S = 0, al_Amax = 0, al_Lmax = 0, al_Hmax = 0;
    if (align) {
        if (e->f32) return fail(e, SONIC_ERR_INVALID, "forced_align: the fp32 kind has no alignment kernels");
        for (int r = 0; r < R; ++r) {
            const int P = (int)(prompt_off[r + 1] - prompt_off[r]);
            const int32_t* pi = prompt_ids + prompt_off[r];
            int first = -1, last = -1, cnt = 0;
            for (int i = 0; i < P; ++i) if (pi[i] == d.audio_token_id) { if (first < 0) first = i; last = i; ++cnt; }
            if (cnt == 0) return fail(e, SONIC_ERR_INVALID, "forced_align: sequence %d has no audio placeholder in its prompt (nothing to align to)", r);
            if (last - first + 1 != cnt) return fail(e, SONIC_ERR_INVALID, "forced_align: the audio placeholders of sequence %d are not one contiguous run (%d of them between positions %d and %d)", r, cnt, first, last);
            if (L[r] > ALIGN_MAX_ROWS) return fail(e, SONIC_ERR_INVALID, "forced_align: sequence %d has %d targets, the DTW kernel holds %d", r, L[r], ALIGN_MAX_ROWS);
            al_a0[r] = first; al_A[r] = cnt; al_S += L[r]; al_Amax = std::max(al_Amax, cnt); al_Lmax = std::max(al_Lmax, (int)L[r]);
        }
        // the selection layer by layer: the caller's list, else every head of the last ceil(dec_layers / 2) layers (Whisper's rule without alignment heads)
        e->align_layer_heads.assign(d.dec_layers, std::vector<int>()); e->align_layer_off.assign(d.dec_layers, 0);
        if (!e->align_heads.empty()) for (int c : e->align_heads) e->align_layer_heads[c >> 8].push_back(c & 255);
        else for (int l = d.dec_layers - (d.dec_layers + 1) / 2; l < d.dec_layers; ++l) for (int h = 0; h < d.dec_heads; ++h) e->align_layer_heads[l].push_back(h);
        int tot = 0;
        for (int l = 0; l < d.dec_layers; ++l) { e->align_layer_off[l] = tot; tot += (int)e->align_layer_heads[l].size(); al_Hmax = std::max(al_Hmax, (int)e->align_layer_heads[l].size()); }
        if (tot > ALIGN_MAX_HEADS) return fail(e, SONIC_ERR_INVALID, "forced_align: the default selection (%d heads) exceeds %d: select heads with option align_head", tot, ALIGN_MAX_HEADS);
        e->align_Htot = tot;
    }
    if (e->wait_pending) { HIPC(e, hipStreamWaitEvent(e->st, e->wait_ev, 0)); e->wait_pending = false; }
    if (align) TRY(align_alloc(e, al_S, al_Amax, al_Hmax));
    TRY(score_alloc(e));
    {   // staging buffer of this run (run_to_first_token)
        const int i = e->plan_idx ^ 1;
        if (e->plan_busy[i]) { HIPC(e, hipEventSynchronize(e->plan_ev[i])); e->plan_busy[i] = false; }
        e->plan_idx = i; e->plan_h = e->plan_buf[i];
    }
    e->R = R; e->max_steps = max_steps; e->last_maxnew = hp.max_new;
    e->last_qlen.resize(R);
    for (int r = 0; r < R; ++r) e->last_qlen[r] = (int)(prompt_off[r + 1] - prompt_off[r]);      // the PROMPT's length: fetch_locked expects kv_len = prompt + tokens - 1
    if (want_logits) {
        const size_t need_n = (size_t)max_steps * R * d.vocab;
        if (need_n > e->dump_cap) {
            if (e->dump) (void)hipFree(e->dump);
            e->dump = nullptr; e->dump_cap = 0;
            HIPC(e, hipMalloc((void**)&e->dump, need_n * 4));
            e->dump_cap = need_n;
        }
        e->dump_steps = max_steps;
    } else e->dump_steps = 0;
    e->run_logits = want_logits;
    // the score rows: hidden-state row | target | record index, S of each, then the rows' closing state (n_new | finished | tok_pos | n_active)
    int S = 0;
    for (int r = 0; r < R; ++r) S += L[r];
    int* ph = e->score_plan_h;
    int* st_h = ph + (size_t)3 * S;
    memset(st_h, 0, (4 * 64) * 4);
    for (int r = 0, s = 0; r < R; ++r) {
        const int P = e->last_qlen[r];
        const int* f = e->force_h.data() + (size_t)r * e->force_ld;
        for (int n = 0; n < L[r]; ++n, ++s) { ph[s] = hp.q_off[r] + P - 1 + n; ph[S + s] = f[n]; ph[2 * S + s] = r * e->out_cap + n; }
        st_h[r] = L[r]; st_h[64 + r] = 1; st_h[128 + r] = P + L[r] - 2;
    }
    for (int r = R; r < 64; ++r) st_h[64 + r] = 0;

    e->align_last = false;
    if (align) {      // the align plan: per score row its query row and sequence, per sequence row0 | L | a0 | A, the heads layer by layer; M starts at zero
        int* ah = e->align_plan_h;
        const size_t tc = (size_t)e->tok_cap;
        for (int r = 0, sr = 0; r < R; ++r) {
            int* sp = ah + 2 * tc + 4 * r;
            sp[0] = sr; sp[1] = L[r]; sp[2] = al_a0[r]; sp[3] = al_A[r];
            for (int n = 0; n < L[r]; ++n, ++sr) { ah[sr] = ph[sr]; ah[tc + sr] = r; }
        }
        int* hh = ah + 2 * tc + 4 * 64;
        for (int l = 0; l < d.dec_layers; ++l) for (size_t i = 0; i < e->align_layer_heads[l].size(); ++i) hh[e->align_layer_off[l] + i] = e->align_layer_heads[l][i];
        HIPC(e, hipMemcpyAsync(e->align_plan_d, ah, (size_t)S * 4, hipMemcpyHostToDevice, e->st));
        HIPC(e, hipMemcpyAsync(e->align_plan_d + tc, ah + tc, (size_t)S * 4, hipMemcpyHostToDevice, e->st));
        HIPC(e, hipMemcpyAsync(e->align_plan_d + 2 * tc, ah + 2 * tc, (size_t)(4 * 64 + ALIGN_MAX_HEADS) * 4, hipMemcpyHostToDevice, e->st));
        e->align_S = S; e->align_nseq = R; e->align_Amax = al_Amax; e->align_Lmax = al_Lmax; e->align_last_heads = 0;
        for (size_t o = 0; o < (size_t)S * al_Amax; o += (size_t)1 << 30) launch_fill_i32((int*)e->align_M + o, 0, (int)std::min((size_t)1 << 30, (size_t)S * al_Amax - o), e->st);
        e->align_live = true;
    }
    struct AlignOff { sonic_engine* e; ~AlignOff() { e->align_live = false; } } align_off{e};      // whatever way the run leaves
    (void)hipEventRecord(e->ev[0], e->st);
    TRY(run_mel(e, e->W, e->f32));
    (void)hipEventRecord(e->ev[1], e->st);
    const int A = R / N;
    if (e->i8) {   // window -> audio request map (run_to_first_token): the encoder's outlier groups are the audio requests, not their candidates
        int* h = e->plan_h + e->plan_cap - 64;
        memset(h, 0, 64 * 4);
        for (int a = 0; a < A; ++a) {
            const int w0 = req_win ? req_win[a] : a, w1 = req_win ? req_win[a + 1] : a + 1;
            for (int w = w0; w < w1 && w < 64; ++w) h[w] = a;
        }
        HIPC(e, hipMemcpyAsync(e->win_req, h, 64 * 4, hipMemcpyHostToDevice, e->st));
    }
    TRY(e->f32 ? f32_run_encoder(e, e->W, nullptr, nullptr) : run_encoder(e, e->W, nullptr, nullptr, A));
    (void)hipEventRecord(e->ev[2], e->st);
    TRY(e->f32 ? f32_run_prefill(e, R, hp, false) : run_prefill(e, R, hp, false));
    HIPC(e, hipMemcpyAsync(e->score_plan_d, ph, (size_t)3 * S * 4, hipMemcpyHostToDevice, e->st));
    if (align) {      // DTW over the finished M: t_n beside the records (rec: the score plan's record indices)
        launch_align_dtw(align_probs_args(e, e->dq, e->Kc, 128, e->max_ctx * 128L, (long)d.dec_kv_heads * e->max_ctx * 128, nullptr, 0, d.dec_heads, d.dec_kv_heads, e->score_plan_d + 2 * S), e->st);
        e->align_live = false; e->align_last = true;
    }
    if (e->f32) f32_score_norm(e, e->score_plan_d, S);
    else launch_rmsnorm(e->dx, e->dec_nw, e->dhn, S, d.dec_d, d.dec_rms_eps, e->score_plan_d, e->st, e->dt);
    ScoreArgs sa{};
    sa.logits = e->score_logits; sa.ld = d.vocab; sa.V = d.vocab; sa.dt = e->f32 ? DT_F32 : e->dt;
    sa.out_ids = e->out_ids; sa.out_lp = (e->opt_token_logprobs && e->out_lp) ? e->out_lp : nullptr; sa.topk = sa.out_lp ? e->opt_top_logprobs : 0;
    sa.dump = want_logits ? e->dump : nullptr; sa.out_ld = e->out_cap; sa.R = R;
    const int chunk = std::min(e->opt_score_chunk_rows, e->score_rows_cap);
    for (int c0 = 0; c0 < S; c0 += chunk) {
        const int n = std::min(chunk, S - c0);
        if (e->f32) f32_score_logits(e, c0, n, (float*)e->score_logits);
        else gemm(e, EPI_BIAS, e->dhn + (size_t)c0 * d.dec_d, d.dec_d, e->embed_t, nullptr, (bf16_t*)e->score_logits, d.vocab, n, d.vocab, d.dec_d, nullptr, 0, 1);   // embed_t: launch_tile_weights' tiling, the one GemmArgs.w_tiled reads
        sa.n = n; sa.target = e->score_plan_d + S + c0; sa.rec = e->score_plan_d + 2 * S + c0;
        launch_score_rows(sa, e->st);
    }
    // the rows' state as a finished batch: n_new = L, finished, tok_pos = kv_len - 1 (kv_len = prompt + L - 1 is what the plan uploaded), nothing running
    HIPC(e, hipMemcpyAsync(e->n_new, st_h, 64 * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(e->finished, st_h + 64, 64 * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(e->tok_pos, st_h + 128, (size_t)R * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(e->n_active, st_h + 192, 4, hipMemcpyHostToDevice, e->st));
    (void)hipEventRecord(e->ev[3], e->st);
    (void)hipEventRecord(e->ev[4], e->st);
    e->steps_run = max_steps - 1; e->greedy_calls = max_steps; e->spliced = 0;      // a finished batch: sonic_decode_step has nothing left to run
    const double host_enqueue_first = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    e->host_launch_ms = e->host_wait_ms = 0; e->host_launches = 0; e->run_starved = false;
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    fill_timings(e, host_enqueue_first, 0);
    return SONIC_OK;
}

int run_all(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
            const int32_t* max_new, bool want_logits) {
    if (e->opt_forced_parallel && e->force_d) return run_forced_parallel(e, req_win, R, prompt_ids, prompt_off, max_new, want_logits);
    const auto t_host0 = std::chrono::steady_clock::now();
    TRY(run_to_first_token(e, req_win, R, prompt_ids, prompt_off, max_new, want_logits));
    const double host_enqueue_first = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    e->host_launch_ms = e->host_wait_ms = 0; e->host_launches = 0; e->run_starved = false;
    int steps_done = 0;
    TRY(run_decode_steps(e, e->max_steps - 1, &steps_done));
    (void)hipEventRecord(e->ev[4], e->st);
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    fill_timings(e, host_enqueue_first, steps_done);
    if (!e->run_starved && e->lookahead > 1) e->lookahead -= 1;       // a batch whose queue never ran dry: one chunk less ahead next time
    return SONIC_OK;
}
