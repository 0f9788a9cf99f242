// sonic_hip engine: the forward pass of the bf16 / fp16 / int8 pipeline on the engine stream - GEMM wrappers, log-mel, encoder, request plan, prefill - and the
// whole-batch run around it: what every run begins and ends with, the run to the first token, run_all.
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
thread_local int g_last_qlinear_defer = 0;
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
    g_last_qlinear_defer = defer;
    launch_gemm(a, epi, e->st);
    if (defer) launch_i8_outlier_side(a, e->st);
    return fuse;
}

// the 16-bit q|k|v GEMM rotates q / k in its epilogue only on the 256x256 tile (launch_gemm sends every eligible EPI_QKV_VT there unless gemm_force128)
bool enc_qkv_fuses_rope(sonic_engine* e, const GemmArgs& a) { return !e->opt_no_fused_rope && !g_opts.gemm_force128 && gemm256_eligible(a, EPI_QKV_VT); }

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
            const bool roped = e->hd_e == 64 && d.enc_rotary_dim == 32 && enc_qkv_fuses_rope(e, a);
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

// ------------------------------------------------------------------------------------------ the prefill's launch descriptors: one builder each (production and the hooks)
// the prefill's causal attention: packed ragged queries, K in cache layout [B][Hkv][ctx_max][128], V^T [B][Hkv][128][ctx_max]
// pre_row / pre_len (option forced_share_prompt): sequence b's keys [0, pre_len[b]) are those of cache row pre_row[b]; null: every sequence reads its own row
FlashArgs prefill_flash_args(const bf16_t* Q, const bf16_t* Kc, const bf16_t* Vt, bf16_t* O, const int* q_off, const int* q_len, const int* kv_len,
                             int Hq, int Hkv, int ctx_max, int dt, const int* pre_row, const int* pre_len) {
    FlashArgs f{}; f.dt = dt; f.pre_row = pre_row; f.pre_len = pre_row ? pre_len : nullptr;
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

// fan (the parallel forced run's forced_fanout; 1 otherwise): sequence r takes its audio rows from audio request r / fan - req_win then has R / fan + 1 entries.
// pos0 (its option forced_share_prompt; null otherwise): sequence r's ids sit at positions pos0[r] on.  pos0[r] > 0: the ids are the suffix behind a prompt another
// sequence packs (pre_row / pre_len are the caller's to fill) - none is an audio placeholder, there may be none at all, and hp.kv_len / hp.q_len tell keys from rows
int plan_requests(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new, HostPlan& hp, int fan, const int32_t* pos0) {
    const sonic_dims& d = e->d;
    const int W = e->W, A = R / fan;
    if (R < 1 || R > e->Bm) return fail(e, SONIC_ERR_INVALID, "request count %d out of range 1..%d", R, e->Bm);
    if (!req_win && A != W) return fail(e, SONIC_ERR_INVALID, "R (%d) must equal staged windows (%d) when req_win is NULL", A, W);
    if (req_win && (req_win[0] != 0 || req_win[A] != W)) return fail(e, SONIC_ERR_INVALID, "req_win must cover exactly the staged windows");
    hp.q_off.resize(R); hp.q_len.resize(R); hp.last_row.resize(R); hp.max_new.resize(R);
    for (int r = 0; r < R; ++r) {
        const int w0 = req_win ? req_win[r / fan] : r / fan, w1 = req_win ? req_win[r / fan + 1] : r / fan + 1;
        if (w1 <= w0) return fail(e, SONIC_ERR_INVALID, "request %d has no audio window", r);
        const int at = pos0 ? pos0[r] : 0;
        std::vector<int> rows;  // audio rows of this request in order
        for (int w = w0; w < w1 && at == 0; ++w) {
            const int k = keep_rows(d, frames_of(e->n_samples_h[w]));
            for (int j = 0; j < k; ++j) rows.push_back(w * e->Ta + j);
        }
        const int64_t p0 = prompt_off[r], p1 = prompt_off[r + 1];
        const int P = (int)(p1 - p0);
        if (P < 1 && at == 0) return fail(e, SONIC_ERR_INVALID, "request %d has an empty prompt", r);
        if (max_new[r] < 1) return fail(e, SONIC_ERR_INVALID, "max_new_tokens must be >= 1");
        if (at + P + max_new[r] > e->max_ctx) return fail(e, SONIC_ERR_INVALID, "prompt (%d) + max_new_tokens (%d) exceeds max_ctx (%d)", at + P, max_new[r], e->max_ctx);
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
            hp.tok_seq.push_back(r); hp.tok_pos.push_back(at + i);
        }
        if (pos0) hp.kv_len.push_back(at + P);
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
// plan_h = the staging buffer run_pick_plan_buffer picked for this run (free: the run that used it last has had its copies waited for).
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
        HIPC(e, put(e->kv_len, hp.pre_row.empty() ? hp.q_len.data() : hp.kv_len.data(), (size_t)R));
        HIPC(e, put(e->last_row, hp.last_row.data(), (size_t)R)); HIPC(e, put(e->max_new_d, hp.max_new.data(), (size_t)R));
        HIPC(e, put(e->n_active, &R, 1));
    }
    if (!hp.pre_row.empty()) { HIPC(e, put(e->pre_row, hp.pre_row.data(), (size_t)R)); HIPC(e, put(e->pre_row + 64, hp.pre_len.data(), (size_t)R)); }      // option forced_share_prompt
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
int run_prefill(sonic_engine* e, int R, const HostPlan& hp, bool head) {
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
            const AlignArgs aa = align_probs_args(e, e->dq, e->Kc + kvoff, 128, e->max_ctx * 128L, (long)d.dec_kv_heads * e->max_ctx * 128, AlignPlan(e->align_plan_d, e->tok_cap).heads + e->align_layer_off[l],
                                                  (int)e->align_layer_heads[l].size(), d.dec_heads, d.dec_kv_heads, nullptr);
            launch_align_probs(aa, e->st);
            launch_align_reduce(aa, e->st);
            e->align_last_heads = aa.n_heads;
        }
        // (a shared plan, option forced_share_prompt: the append above has taken every row's position from tok_pos, in tiles of a sequence's PACKED rows; the attention tells keys from rows)
        const bool shared = !hp.pre_row.empty();
        const FlashArgs f = prefill_flash_args(e->dq, e->Kc + kvoff, e->Vts, e->datt, e->q_off, e->q_len, shared ? e->kv_len : e->q_len, d.dec_heads, d.dec_kv_heads, e->max_ctx, dt,
                                               shared ? e->pre_row : nullptr, shared ? e->pre_row + 64 : nullptr);
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

// ------------------------------------------------------------------------------------------ what every whole-batch run begins and ends with (run_to_first_token / run_all, run_forced_parallel)
int run_refuse_unready(sonic_engine* e) {
    if (!e->finalized) return fail(e, SONIC_ERR_INVALID, "weights not finalized");
    if (e->W < 1) return fail(e, SONIC_ERR_INVALID, "no PCM staged");
    if (e->svc_on) return fail(e, SONIC_ERR_INVALID, "this handle is decoding continuously (sonic_service_begin): prefill on another slot and splice the rows in");
    return SONIC_OK;
}
// rows of the previous batch were spliced into another handle: its copy kernels read this engine's KV cache and row state, which this run is about to overwrite
int run_wait_spliced(sonic_engine* e) {
    if (e->wait_pending) { HIPC(e, hipStreamWaitEvent(e->st, e->wait_ev, 0)); e->wait_pending = false; }
    return SONIC_OK;
}
// staging buffer of this run: the one used two runs ago; its copies are almost always long done (a blocking wait otherwise)
int run_pick_plan_buffer(sonic_engine* e) {
    const int i = e->plan_idx ^ 1;
    if (e->plan_busy[i]) { HIPC(e, hipEventSynchronize(e->plan_ev[i])); e->plan_busy[i] = false; }
    e->plan_idx = i; e->plan_h = e->plan_buf[i];
    return SONIC_OK;
}
// the step-logits dump of a run of `rows` rows: room for cap_steps steps (grown, never shrunk), of which a fetch reads the first dump_steps
int run_reserve_dump(sonic_engine* e, bool want_logits, int dump_steps, int cap_steps, int rows) {
    const size_t need_n = want_logits ? (size_t)cap_steps * rows * e->d.vocab : 0;
    if (need_n > e->dump_cap) {
        if (e->dump) (void)hipFree(e->dump);
        e->dump = nullptr; e->dump_cap = 0;
        HIPC(e, hipMalloc((void**)&e->dump, need_n * 4));
        e->dump_cap = need_n;
    }
    e->dump_steps = want_logits ? dump_steps : 0; e->run_logits = want_logits;
    return SONIC_OK;
}
// window -> group map (int8 mode: the encoder's outlier columns are found per group, the request of the window); pinned: the last 64 words of plan_h, beyond what upload_plan uses
int run_upload_win_req(sonic_engine* e, const int32_t* req_win, int n_groups) {
    if (!e->i8) return SONIC_OK;
    int* h = e->plan_h + e->plan_cap - 64;
    memset(h, 0, 64 * 4);
    for (int r = 0; r < n_groups; ++r) {
        const int w0 = req_win ? req_win[r] : r, w1 = req_win ? req_win[r + 1] : r + 1;
        for (int w = w0; w < w1 && w < 64; ++w) h[w] = r;
    }
    HIPC(e, hipMemcpyAsync(e->win_req, h, 64 * 4, hipMemcpyHostToDevice, e->st));
    return SONIC_OK;
}

// log-mel -> encoder -> projector -> prefill -> first greedy token (generation/utils.py:2612-2616, 2876-2943 for the first step)
int run_to_first_token(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                       const int32_t* max_new, bool want_logits) {
    const sonic_dims& d = e->d;
    TRY(run_refuse_unready(e));
    TRY(run_wait_spliced(e));
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
        // the verify rows (DraftPlan): hidden row | draft id | record index | request | history length, S of each; then per request D | first row | P | first token
        hp.draft.assign(DraftPlan::words(hp.S), 0);
        const DraftPlan w(hp.draft.data(), hp.S);
        for (int r = 0, s = 0; r < R; ++r) {
            const int P = hp.q_len[r] - dlen[r];
            w.dlen[r] = dlen[r]; w.first[r] = s; w.P[r] = P; w.q_off[r] = hp.q_off[r];
            for (int n = 0; n < dlen[r]; ++n, ++s) { w.hidden[s] = hp.q_off[r] + P - 1 + n; w.target[s] = x_ids[(size_t)x_off[r] + P + n]; w.rec[s] = r * e->out_cap + n; w.hrow[s] = r; w.hlen[s] = P + n; }
        }
    }
    e->draft_last_S = hp.S;
    e->fork_timed = false;
    if (Rr > R) {
        if (d.dec_head_dim % 8) return fail(e, SONIC_ERR_INVALID, "request_forks: a head dimension of %d is not a multiple of 8 elements (the copy moves 16-byte pieces)", d.dec_head_dim);
        hp.rows = Rr; hp.fork_src = fork_src;
        for (int i = 0; i < 2; ++i) if (!e->fork_ev[i]) HIPC(e, hipEventCreate(&e->fork_ev[i]));
    }
    TRY(run_pick_plan_buffer(e));
    if (e->force_d && (e->force_R != R || e->force_ld < hp.max_steps))
        return fail(e, SONIC_ERR_INVALID, "forced ids are [%d][%d] but the run has %d requests / %d steps", e->force_R, e->force_ld, R, hp.max_steps);
    e->R = Rr; e->max_steps = hp.max_steps; e->last_qlen = hp.q_len; e->last_maxnew = hp.max_new; e->align_last = false;
    for (size_t r = 0; r < dlen.size(); ++r) e->last_qlen[r] -= dlen[r];      // the PROMPT's length: fetch_locked expects kv_len = prompt + tokens - 1
    for (int r = R; r < Rr; ++r) { e->last_qlen.push_back(hp.q_len[fork_src[r]]); e->last_maxnew.push_back(hp.max_new[fork_src[r]]); }      // (a fork's invariants are its request's)
    // a drafted row's step counter starts at its accepted count and goes on counting with every launch, also once the row has ended: the dump holds the steps
    // the longest draft can add (the fetch reads the first max_steps of them, as always)
    int d_max = 0;
    for (int D : dlen) d_max = std::max(d_max, D);
    TRY(run_reserve_dump(e, want_logits, hp.max_steps, hp.max_steps + d_max, Rr));

    (void)hipEventRecord(e->ev[0], e->st);
    TRY(run_mel(e, e->W, e->f32));
    (void)hipEventRecord(e->ev[1], e->st);
    TRY(run_upload_win_req(e, req_win, R));      // (int8 mode: outlier columns are found per request)
    TRY(e->f32 ? f32_run_encoder(e, e->W, nullptr, nullptr) : run_encoder(e, e->W, nullptr, nullptr, R));
    (void)hipEventRecord(e->ev[2], e->st);
    TRY(e->f32 ? f32_run_prefill(e, R, hp) : run_prefill(e, R, hp));
    lm_prefill_rows(e, Rr);                      // option lm: the rows start at the model's start node, no token pending ...
    lm_step(e, Rr);                              // ... and their vectors stand ahead of the first token's launch
    launch_greedy(e->f32 ? f32_greedy_args(e, Rr, want_logits) : greedy_args(e, Rr, want_logits), e->st);
    (void)hipEventRecord(e->ev[3], e->st);
    e->steps_run = 0; e->greedy_calls = 1; e->spliced = 0;
    return SONIC_OK;
}

// what every whole-batch run ends with (run_close): the stage times from the events and the decode loop's host figures
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

void run_zero_host_figures(sonic_engine* e) { e->host_launch_ms = e->host_wait_ms = 0; e->host_launches = 0; e->run_starved = false; }
int run_close(sonic_engine* e, double host_enqueue_first, int steps_done) {
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    fill_timings(e, host_enqueue_first, steps_done);
    return SONIC_OK;
}

int run_all(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
            const int32_t* max_new, bool want_logits) {
    if (e->opt_forced_parallel && e->force_d) return run_forced_parallel(e, req_win, R, prompt_ids, prompt_off, max_new, want_logits);
    const auto t_host0 = std::chrono::steady_clock::now();
    TRY(run_to_first_token(e, req_win, R, prompt_ids, prompt_off, max_new, want_logits));
    const double host_enqueue_first = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    run_zero_host_figures(e);
    int steps_done = 0;
    TRY(run_decode_steps(e, e->max_steps - 1, &steps_done));
    (void)hipEventRecord(e->ev[4], e->st);
    TRY(run_close(e, host_enqueue_first, steps_done));
    if (!e->run_starved && e->lookahead > 1) e->lookahead -= 1;       // a batch whose queue never ran dry: one chunk less ahead next time
    return SONIC_OK;
}
