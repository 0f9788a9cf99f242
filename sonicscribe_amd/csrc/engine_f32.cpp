// sonic_hip engine: the SONIC_MODE_F32 kind of every stage (test only).
#include "engine_internal.h"

// ------------------------------------------------------------------------------------------ SONIC_MODE_F32 (test only): fp32 stages, f32kind.hip
// The request plan (plan_requests), PCM staging, the log-mel kernel, the control words (kv_len / tok_pos / n_new / finished / out_ids / step logits dump /
// teacher forcing) and the greedy controller (greedy_kernel<float>) are the engine's own; what is different is the arithmetic between them.
int f32_alloc(sonic_engine* e) {
    F32State& f = *e->f;
    const sonic_dims& d = e->d;
    const int Bm = e->Bm, C = d.enc_d;
    const size_t M = (size_t)Bm * e->T, tc = (size_t)e->tok_cap + 64;
    int s;
#define A(x) do { s = (x); if (s != SONIC_OK) return s; } while (0)
    A(dalloc(e, &f.featT, (size_t)Bm * (d.n_frames + 2) * d.n_mels + 4 * (size_t)d.n_mels)); A(dalloc(e, &f.h1, (size_t)Bm * (d.n_frames + 2) * C + 4 * (size_t)C));
    A(dalloc(e, &f.x, M * C)); A(dalloc(e, &f.ln, M * C)); A(dalloc(e, &f.q, M * C)); A(dalloc(e, &f.k, M * C)); A(dalloc(e, &f.v, M * C)); A(dalloc(e, &f.att, M * C));
    A(dalloc(e, &f.ff, M * d.enc_ff)); A(dalloc(e, &f.ph, (size_t)Bm * e->Ta * 2 * d.dec_d)); A(dalloc(e, &f.pe, (size_t)Bm * e->Ta * d.dec_d));
    A(dalloc(e, &f.dx, tc * d.dec_d)); A(dalloc(e, &f.dhn, tc * d.dec_d)); A(dalloc(e, &f.dq, tc * e->QD)); A(dalloc(e, &f.dk, tc * e->KD)); A(dalloc(e, &f.dv, tc * e->KD));
    A(dalloc(e, &f.datt, tc * e->QD)); A(dalloc(e, &f.dg, tc * d.dec_ff)); A(dalloc(e, &f.du, tc * d.dec_ff)); A(dalloc(e, &f.dact, tc * d.dec_ff));
    const size_t kvn = (size_t)d.dec_layers * Bm * e->max_ctx * e->KD;
    A(dalloc(e, &f.Kc, kvn)); A(dalloc(e, &f.Vc, kvn));
    A(dalloc(e, &f.logits, (size_t)64 * d.vocab)); A(dalloc(e, &f.hlast, (size_t)64 * d.dec_d));
#undef A
    return SONIC_OK;
}
int f32_finalize(sonic_engine* e) {
    F32State& f = *e->f;
    const sonic_dims& d = e->d;
    const std::string at = "model.audio_tower.", pj = "model.multi_modal_projector.", lm = "model.language_model.";
    auto get = [&](const std::string& name, float** out) -> int {
        auto it = f.raw.find(name);
        if (it == f.raw.end() || !it->second) return fail(e, SONIC_ERR_INVALID, "missing weight tensor %s", name.c_str());
        *out = it->second;
        return SONIC_OK;
    };
    float *c1 = nullptr, *c2 = nullptr;
    TRY(get(at + "conv1.weight", &c1)); TRY(get(at + "conv2.weight", &c2));
    TRY(dalloc(e, &f.conv1w, (size_t)d.enc_d * d.n_mels * 3, false)); TRY(dalloc(e, &f.conv2w, (size_t)d.enc_d * d.enc_d * 3, false));
    launch_f32_conv_w(c1, f.conv1w, d.enc_d, d.n_mels, e->st); launch_f32_conv_w(c2, f.conv2w, d.enc_d, d.enc_d, e->st);   // [C][Ci][3] -> tap-major [C][3][Ci]
    TRY(get(at + "conv1.bias", &f.conv1b)); TRY(get(at + "conv2.bias", &f.conv2b));
    f.enc.resize(d.enc_layers);
    for (int i = 0; i < d.enc_layers; ++i) {
        const std::string p = at + "layers." + std::to_string(i) + ".";
        F32EncL& L = f.enc[i];
        TRY(get(p + "input_layernorm.weight", &L.ln1w)); TRY(get(p + "input_layernorm.bias", &L.ln1b));
        TRY(get(p + "self_attn.q_proj.weight", &L.wq)); TRY(get(p + "self_attn.q_proj.bias", &L.bq)); TRY(get(p + "self_attn.k_proj.weight", &L.wk));
        TRY(get(p + "self_attn.v_proj.weight", &L.wv)); TRY(get(p + "self_attn.v_proj.bias", &L.bv));
        TRY(get(p + "self_attn.o_proj.weight", &L.wo)); TRY(get(p + "self_attn.o_proj.bias", &L.bo));
        TRY(get(p + "post_attention_layernorm.weight", &L.ln2w)); TRY(get(p + "post_attention_layernorm.bias", &L.ln2b));
        TRY(get(p + "mlp.fc1.weight", &L.w1)); TRY(get(p + "mlp.fc1.bias", &L.b1)); TRY(get(p + "mlp.fc2.weight", &L.w2)); TRY(get(p + "mlp.fc2.bias", &L.b2));
    }
    TRY(get(at + "norm.weight", &f.enc_nw)); TRY(get(at + "norm.bias", &f.enc_nb));
    TRY(get(pj + "linear_1.weight", &f.pj1w)); TRY(get(pj + "linear_1.bias", &f.pj1b)); TRY(get(pj + "linear_2.weight", &f.pj2w)); TRY(get(pj + "linear_2.bias", &f.pj2b));
    TRY(get(lm + "embed_tokens.weight", &f.embed));
    f.dec.resize(d.dec_layers);
    for (int i = 0; i < d.dec_layers; ++i) {
        const std::string p = lm + "layers." + std::to_string(i) + ".";
        F32DecL& L = f.dec[i];
        TRY(get(p + "input_layernorm.weight", &L.ln1)); TRY(get(p + "self_attn.q_proj.weight", &L.wq)); TRY(get(p + "self_attn.k_proj.weight", &L.wk));
        TRY(get(p + "self_attn.v_proj.weight", &L.wv)); TRY(get(p + "self_attn.o_proj.weight", &L.wo)); TRY(get(p + "post_attention_layernorm.weight", &L.ln2));
        TRY(get(p + "mlp.gate_proj.weight", &L.wg)); TRY(get(p + "mlp.up_proj.weight", &L.wu)); TRY(get(p + "mlp.down_proj.weight", &L.wd));
    }
    TRY(get(lm + "norm.weight", &f.dec_nw));
    HIPC(e, stream_sync(e));
    e->finalized = true;
    return SONIC_OK;
}
static void f32_linear(sonic_engine* e, const float* X, long ldx, const float* W, const float* bias, float* Y, long ldy, int M, int N, int K, int epi = F32_EPI_NONE,
                       const float* R = nullptr, long ldr = 0) {
    F32Gemm g{};
    g.A = X; g.lda = ldx; g.W = W; g.C = Y; g.ldc = ldy; g.bias = bias; g.R = R; g.ldr = ldr; g.M = M; g.N = N; g.K = K; g.epi = epi;
    launch_f32_gemm(g, e->st);
}
// feats_f32 [W][n_mels][n_frames] -> pe [W * Ta][dec_d]   (modeling_glmasr.py:313-346, :380-408)
int f32_run_encoder(sonic_engine* e, int W, float* enc_layers_out, float* enc_out_host) {
    F32State& f = *e->f;
    const sonic_dims& d = e->d;
    const int C = d.enc_d, T = e->T, M = W * T, H = d.enc_heads, hd = e->hd_e, NF = d.n_frames;
    launch_f32_feats_tm(e->feats_f32, f.featT, W, d.n_mels, NF, e->st);
    {   // conv stem: rows of the time-major padded input overlap (output t reads padded rows t .. t + 2; stride 2: 2t .. 2t + 2), taps-major weights
        F32Gemm a{};
        a.A = f.featT; a.lda = d.n_mels; a.sA1 = (long)(NF + 2) * d.n_mels; a.W = f.conv1w; a.bias = f.conv1b; a.C = f.h1 + C; a.ldc = C; a.sC1 = (long)(NF + 2) * C;
        a.M = NF; a.N = C; a.K = 3 * d.n_mels; a.nb1 = W; a.epi = F32_EPI_GELU;
        launch_f32_gemm(a, e->st);
        launch_f32_zero_pad_rows(f.h1, W, NF, C, e->st);
        F32Gemm b{};
        b.A = f.h1; b.lda = 2L * C; b.sA1 = (long)(NF + 2) * C; b.W = f.conv2w; b.bias = f.conv2b; b.C = f.x; b.ldc = C; b.sC1 = (long)T * C;
        b.M = T; b.N = C; b.K = 3 * C; b.nb1 = W; b.epi = F32_EPI_GELU;
        launch_f32_gemm(b, e->st);
    }
    for (int l = 0; l < d.enc_layers; ++l) {
        const F32EncL& L = f.enc[l];
        launch_f32_layernorm(f.x, L.ln1w, L.ln1b, f.ln, M, C, d.enc_ln_eps, e->st);
        f32_linear(e, f.ln, C, L.wq, L.bq, f.q, C, M, C, C);
        f32_linear(e, f.ln, C, L.wk, nullptr, f.k, C, M, C, C);                       // k_proj has no bias (modeling_glmasr.py:184)
        f32_linear(e, f.ln, C, L.wv, L.bv, f.v, C, M, C, C);
        launch_f32_rope(f.q, C, M, H, hd, d.enc_rotary_dim, e->enc_cs, nullptr, T, e->st);
        launch_f32_rope(f.k, C, M, H, hd, d.enc_rotary_dim, e->enc_cs, nullptr, T, e->st);
        F32Attn a{};
        a.Q = f.q; a.ldq = C; a.K = f.k; a.V = f.v; a.ldkv = C; a.seq_stride = (long)T * C; a.O = f.att; a.ldo = C; a.seq = nullptr; a.seq_div = T;
        a.pos = nullptr; a.lim_const = T; a.lim_max = T; a.hd = hd; a.grp = 1; a.scale = 1.0f / sqrtf((float)hd);
        launch_f32_attn(a, M, H, e->st);
        f32_linear(e, f.att, C, L.wo, L.bo, f.x, C, M, C, C, F32_EPI_RESID, f.x, C);
        launch_f32_layernorm(f.x, L.ln2w, L.ln2b, f.ln, M, C, d.enc_ln_eps, e->st);
        f32_linear(e, f.ln, C, L.w1, L.b1, f.ff, d.enc_ff, M, d.enc_ff, C, F32_EPI_GELU);
        f32_linear(e, f.ff, d.enc_ff, L.w2, L.b2, f.x, C, M, C, d.enc_ff, F32_EPI_RESID, f.x, C);
        if (enc_layers_out) {
            HIPC(e, stream_sync(e));
            for (int b = 0; b < W; ++b) HIPC(e, d2h(e, enc_layers_out + ((size_t)b * d.enc_layers + l) * T * C, f.x + (size_t)b * T * C, (size_t)T * C * 4));
        }
    }
    launch_f32_layernorm(f.x, f.enc_nw, f.enc_nb, f.ln, M, C, d.enc_ln_eps, e->st);
    if (enc_out_host) { HIPC(e, stream_sync(e)); HIPC(e, d2h(e, enc_out_host, f.ln, (size_t)M * C * 4)); }
    const int Mp = W * e->Ta, PI = C * d.merge, PM = 2 * d.dec_d;                       // the 4-frame merge is a view: [M][C] == [W * Ta][4C]
    f32_linear(e, f.ln, PI, f.pj1w, f.pj1b, f.ph, PM, Mp, PM, PI, F32_EPI_GELU);
    f32_linear(e, f.ph, PM, f.pj2w, f.pj2b, f.pe, d.dec_d, Mp, d.dec_d, PM);
    return SONIC_OK;
}
// the decoder layers over n_tok token rows of f.dx: token t belongs to sequence seq[t] and sits at position pos[t] (prefill: the prompt rows of all
// requests; token step: one row per request).  Keys / values are appended before the attention, which sees positions 0 .. pos[t] (llama:217-324)
static void f32_decoder_layers(sonic_engine* e, int n_tok, const int* seq, const int* pos) {
    F32State& f = *e->f;
    const sonic_dims& d = e->d;
    const int D = d.dec_d, QD = e->QD, KD = e->KD, hd = d.dec_head_dim, FF = d.dec_ff;
    const long seq_stride = (long)e->max_ctx * KD;
    for (int l = 0; l < d.dec_layers; ++l) {
        const F32DecL& L = f.dec[l];
        float* Kl = f.Kc + (size_t)l * e->Bm * seq_stride; float* Vl = f.Vc + (size_t)l * e->Bm * seq_stride;
        launch_f32_rmsnorm(f.dx, L.ln1, f.dhn, n_tok, D, d.dec_rms_eps, nullptr, e->st);
        f32_linear(e, f.dhn, D, L.wq, nullptr, f.dq, QD, n_tok, QD, D);
        f32_linear(e, f.dhn, D, L.wk, nullptr, f.dk, KD, n_tok, KD, D);
        f32_linear(e, f.dhn, D, L.wv, nullptr, f.dv, KD, n_tok, KD, D);
        launch_f32_rope(f.dq, QD, n_tok, d.dec_heads, hd, hd, e->dec_cs, pos, 0, e->st);
        launch_f32_rope(f.dk, KD, n_tok, d.dec_kv_heads, hd, hd, e->dec_cs, pos, 0, e->st);
        launch_f32_kv_append(f.dk, f.dv, Kl, Vl, seq, pos, n_tok, KD, seq_stride, e->st);
        F32Attn a{};
        a.Q = f.dq; a.ldq = QD; a.K = Kl; a.V = Vl; a.ldkv = KD; a.seq_stride = seq_stride; a.O = f.datt; a.ldo = QD; a.seq = seq; a.seq_div = 1;
        a.pos = pos; a.lim_const = 0; a.lim_max = e->max_ctx; a.hd = hd; a.grp = d.dec_heads / d.dec_kv_heads; a.scale = 1.0f / sqrtf((float)hd);
        launch_f32_attn(a, n_tok, d.dec_heads, e->st);
        f32_linear(e, f.datt, QD, L.wo, nullptr, f.dx, D, n_tok, D, QD, F32_EPI_RESID, f.dx, D);
        launch_f32_rmsnorm(f.dx, L.ln2, f.dhn, n_tok, D, d.dec_rms_eps, nullptr, e->st);
        f32_linear(e, f.dhn, D, L.wg, nullptr, f.dg, FF, n_tok, FF, D);
        f32_linear(e, f.dhn, D, L.wu, nullptr, f.du, FF, n_tok, FF, D);
        launch_f32_swiglu(f.dg, f.du, f.dact, (long)n_tok * FF, e->st);
        f32_linear(e, f.dact, FF, L.wd, nullptr, f.dx, D, n_tok, D, FF, F32_EPI_RESID, f.dx, D);
        if (e->taps_on && e->taps) (void)hipMemcpyAsync((float*)e->taps + (size_t)(l + 1) * e->tok_cap * D, f.dx, (size_t)n_tok * D * 4, hipMemcpyDeviceToDevice, e->st);
    }
}
GreedyArgs f32_greedy_args(sonic_engine* e, int R, bool dump) {
    GreedyArgs g = greedy_args(e, R, dump);
    g.logits = e->f->logits; g.ksplit = 1; g.mpad = 64; g.table = (const bf16_t*)e->f->embed; g.x = (bf16_t*)e->f->dx; g.y = nullptr; g.norm_w = nullptr; g.dt = DT_F32;
    g.qo = QuantOut{};
    return g;
}
// final norm of the rows `last_row` (null: rows 0 .. R-1) + tied lm_head -> f.logits [R][vocab]
static void f32_lm_head(sonic_engine* e, int R, const int* last_row) {
    F32State& f = *e->f;
    const sonic_dims& d = e->d;
    launch_f32_rmsnorm(f.dx, f.dec_nw, f.hlast, R, d.dec_d, d.dec_rms_eps, last_row, e->st);
    f32_linear(e, f.hlast, d.dec_d, f.embed, nullptr, f.logits, d.vocab, R, d.vocab, d.dec_d);
}
int f32_run_prefill(sonic_engine* e, int R, const HostPlan& hp, bool head) {
    F32State& f = *e->f;
    const sonic_dims& d = e->d;
    const int D = d.dec_d, M = hp.n_tok;
    TRY(upload_plan(e, R, hp));
    TRY(reset_row_state(e, R, M));
    launch_f32_assemble(e->src, f.embed, f.pe, f.dx, M, D, e->st);
    e->last_ntok = M;
    if (e->taps_on) {
        if (!e->taps) HIPC(e, hipMalloc((void**)&e->taps, (size_t)(d.dec_layers + 1) * e->tok_cap * D * 4));
        HIPC(e, hipMemcpyAsync(e->taps, f.dx, (size_t)M * D * 4, hipMemcpyDeviceToDevice, e->st));
    }
    f32_decoder_layers(e, M, e->tok_seq, e->tok_pos_pf);
    if (head) f32_lm_head(e, R, e->last_row);  // logits of the last prompt position only (logits_to_keep = 1, generation/utils.py:2612-2616)
    return SONIC_OK;
}
// the parallel forced run's tail (run_forced_parallel): the final norm of the S score rows `row_map` names -> dhn [S][d] (free behind the last layer), and the tied
// lm_head over rows row0 .. row0 + n of them -> logits [n][vocab]
void f32_score_norm(sonic_engine* e, const int* row_map, int S) {
    F32State& f = *e->f;
    launch_f32_rmsnorm(f.dx, f.dec_nw, f.dhn, S, e->d.dec_d, e->d.dec_rms_eps, row_map, e->st);
}
void f32_score_logits(sonic_engine* e, int row0, int n, float* logits) {
    F32State& f = *e->f;
    const sonic_dims& d = e->d;
    f32_linear(e, f.dhn + (size_t)row0 * d.dec_d, d.dec_d, f.embed, nullptr, logits, d.vocab, n, d.vocab, d.dec_d);
}
// one token step for R rows (generation/utils.py:2876-2943): the rows' input embeddings are in f.dx (greedy_kernel<float> left them there)
void decode_step_f32(sonic_engine* e, int R, bool dump) {
    f32_decoder_layers(e, R, e->seq_iota, e->tok_pos);
    f32_lm_head(e, R, nullptr);
    lm_step(e, R);
    launch_greedy(f32_greedy_args(e, R, dump), e->st);
}
