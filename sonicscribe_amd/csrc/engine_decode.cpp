// sonic_hip engine: the token step of the bf16 / fp16 / int8 pipeline and its loop - the step's launch builders and its forms, the captured chunk graphs,
// the greedy loop with its pipelined early-stop check.
#include "engine_internal.h"

// ------------------------------------------------------------------------------------------ the token step's launch descriptors: one builder each (production and the hooks)
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

static long long* kt_slot(sonic_engine* e, int l, int slot) { return (e->kt && l == e->kt_layer) ? e->kt + (long)slot * KT_SLOT_BLOCKS * 8 : nullptr; }
void skinny(sonic_engine* e, const bf16_t* X, long ldx, const bf16_t* W, float* P, int M, int N, int K, int* ks_out, long long* kt) {
    SkinnyArgs a = skinny_args(X, ldx, W, P, M, N, K, skinny_pick_ksplit(N, K), e->dt); a.kt = kt;
    if (ks_out) *ks_out = a.ksplit;
    launch_skinny(a, e->st);
}
// int8 decode step: rows X [M][K] x fragment-tiled int8 weights -> int32 slabs (dequantised by the consumer).  amax == null: X holds the quantised rows; else the
// UNQUANTISED fp16 rows with their gathered absmax partials, and the kernel quantises its X slice while staging it.  (The int8 kernels do not read dt.)
int skinny_i8(sonic_engine* e, const void* X, const float* amax, const int8_t* Wt, float* P, int M, int N, int K) {
    SkinnyArgs a = skinny_args((const bf16_t*)X, K, (const bf16_t*)Wt, P, M, N, K, skinny_pick_ksplit_i8(N, K), DT_BF16); a.i8 = 1; a.x_amax = amax;
    launch_skinny(a, e->st);
    return a.ksplit;
}
// ... and how its consumer dequantises the slabs: the rows' statistics and outlier lists as their producer left them (q), the projection's weights in every copy it
// keeps (w), the unquantised rows x16 [.][K].  One row = one reference call = one group.  The step's on-the-fly form sets sca / scan / scan_cnt on the result
DeqInfo deq_info(const sonic_engine* e, const QuantOut& q, const QW& w, int K, const bf16_t* x16, int N) {
    DeqInfo dq{}; dq.sca = q.sca; dq.scb = w.scb; dq.cb = w.cb; dq.cbt = w.cbt; dq.cbk = w.cbk; dq.N = N; dq.K = K; dq.x16 = x16; dq.ldx16 = K; dq.oc_cnt = q.oc_cnt; dq.oc_list = q.oc_list; dq.oc_ld = q.oc_ld;
    dq.row_group = nullptr; dq.group_div = 1; dq.oc_val = q.oc_val; dq.dbg = e->opt_i8_dbg;
    return dq;
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
//   fp8         1 - 4 rows, mode fp8 with its chain on (fp8_weights / fp8_chain) and every shape eligible: the GEMV chain on the e4m3 copies - the same five launches,
//               the same bits as `gemv` on the snapped weights.  Where it is not eligible the snapped model runs the forms below
//   fuse_gu / fuse_o   the fused gate/up kernel, and the fused o_proj in front of it, take the shape (launch_o_gu's forms)
//   pre         <= 2 rows (the B = 1 call shape of BASELINE configs 1 and 5; round 6): no standalone add+RMSNorm launch behind down_proj - the next q|k|v projection
//               (and, behind the last layer, the lm_head) sums the slabs, adds the residual and normalises its rows itself (skinny_xs_kernel<.., PRE>, the same
//               arithmetic statement by statement: same bits).  down_proj then writes its slabs to slab2 (the consumer writes slab while other blocks of it still
//               read) and the residual stream alternates between sx and sx2
//   split_norm  33 .. 64 rows, on request or inside a continuous loop's graph (gu64_split_norm): OGU_SPLIT_NORM.  Never with pre (rows), so its rows are in sx
struct StepForm { bool gemv, fp8, pre, fuse_o, fuse_gu, split_norm; };
static StepForm step_form(sonic_engine* e, int R) {
    const sonic_dims& d = e->d;
    const int D = d.dec_d;
    // wgu_t8 is set for every decoder layer or for none: engine_weights.cpp asks skinny_gu_eligible(1, 2 ff, d) of the model's dims under one lock, the same answer
    // layer after layer (and never in int8 mode) - so layer 0 speaks for all
    const bool gu8 = d.dec_layers > 0 && e->dec[0].wgu_t8;
    StepForm f{};
    f.gemv = e->opt_decode_gemv && R <= GEMV_MAX_ROWS && gu8 && gemv_eligible(R, e->qkvN, D, GEMV_SLAB_NORM) && gemv_eligible(R, D, e->QD, GEMV_RESID) &&
             gemv_eligible(R, 2 * d.dec_ff, D, GEMV_SWIGLU_NORM) && gemv_eligible(R, D, d.dec_ff, GEMV_RESID) && gemv_eligible(R, d.vocab, D, GEMV_SLAB_NORM);
    f.fp8 = fp8_chain_on(e) && R <= GEMV_MAX_ROWS && gu8 && e->dec[0].gu8 && e->embed8 && gemv_fp8_eligible(R, e->qkvN, D, GEMV_SLAB_NORM) && gemv_fp8_eligible(R, D, e->QD, GEMV_RESID) &&
            gemv_fp8_eligible(R, 2 * d.dec_ff, D, GEMV_SWIGLU_NORM) && gemv_fp8_eligible(R, D, d.dec_ff, GEMV_RESID) && gemv_fp8_eligible(R, d.vocab, D, GEMV_SLAB_NORM);
    f.fuse_gu = gu8 && skinny_gu_eligible(R, 2 * d.dec_ff, D);
    f.fuse_o = f.fuse_gu && skinny_o_eligible(R, D, e->QD);
    f.pre = f.fuse_o && !e->opt_no_pre_norm && skinny_pre_eligible(R, e->qkvN, D) && skinny_pre_eligible(R, d.vocab, D) && D % 8 == 0;
    f.split_norm = f.fuse_o && (e->opts.gu64_split_norm > 0 || (e->opts.gu64_split_norm == 0 && e->cap_svc)) && R > 32 && D % 128 == 0 && D <= 2048;
    return f;
}
// 1 - 4 rows, opt-in (gemv.hip): q|k|v (norm inside) -> attention -> o_proj (+ residual) -> gate/up (norm inside, SwiGLU) -> down_proj (+ residual); lm_head (norm inside)
// fp8: the same chain on the e4m3 copies and the rows' scales (gemv_fp8.hip; mode fp8)
static void decode_step_gemv(sonic_engine* e, int R, bool dump, bool fp8) {
    const sonic_dims& d = e->d;
    const int D = d.dec_d, mpad = ((R + 15) / 16) * 16, dt = e->dt;
    auto gv = [&](int mode, const bf16_t* X, long ldx, const bf16_t* W, const unsigned char* W8, const float* sc, int N, int K, const float* nw, float* P, bf16_t* resid, bf16_t* act) {
        GemvArgs g{}; g.X = X; g.ldx = ldx; g.W = W; g.M = R; g.N = N; g.K = K; g.dt = dt; g.norm_w = nw; g.eps = d.dec_rms_eps; g.P = P; g.resid = resid; g.ldr = D; g.act = act;
        if (fp8) launch_gemv_fp8(GemvFp8Args{g, W8, sc}, mode, e->st);
        else launch_gemv(g, mode, e->st);
    };
    for (int l = 0; l < d.dec_layers; ++l) {
        const DecLayerW& L = e->dec[l];
        gv(GEMV_SLAB_NORM, e->sx, D, L.wqkv_t, L.qkv8, L.qkv_sc, e->qkvN, D, L.ln1, e->slab, nullptr, nullptr);
        launch_decode_attn(step_attn_args(e, l, 1, mpad, dt), R, e->st);
        gv(GEMV_RESID, e->satt, e->QD, L.wo_t, L.o8, L.o_sc, D, e->QD, nullptr, nullptr, e->sx, nullptr);
        gv(GEMV_SWIGLU_NORM, e->sx, D, L.wgu_t8, L.gu8, L.gu_sc, 2 * d.dec_ff, D, L.ln2, nullptr, nullptr, e->sact);
        gv(GEMV_RESID, e->sact, d.dec_ff, L.wdown_t, L.down8, L.down_sc, D, d.dec_ff, nullptr, nullptr, e->sx, nullptr);
    }
    gv(GEMV_SLAB_NORM, e->sx, D, e->embed_t, e->embed8, e->embed_sc, d.vocab, D, e->dec_nw, e->lslab, nullptr, nullptr);
    GreedyArgs g = greedy_args(e, R, dump);
    g.ksplit = 1;
    lm_step(e, R);                                                  // option lm: the rows' vectors right ahead of the launch that adds them
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

// int8 mode (asr.py:169-210): every decoder projection is a Linear8bitLt.  In a decode step each row is one reference call, so its
// outlier "columns" are its own elements >= 6.0.  Producers that own whole rows emit them quantised (greedy / add+RMSNorm / SwiGLU
// kernels; the attention output by its own one-block-per-row pass), the skinny int8 GEMM streams the fragment-tiled int8 weights
// (half the bytes of the bf16 step) into exact int32 slabs, and the consumer dequantises them (int8_util.h deq4).
static void decode_step_i8(sonic_engine* e, int R, bool dump) {
    const sonic_dims& d = e->d;
    e->step_launches_per_layer = 8;
    const int D = d.dec_d, FF = d.dec_ff, mpad = ((R + 15) / 16) * 16;
    const QuantOut q_hn{e->hn_q, D, e->sca_hn, e->oc_hn, e->ol_hn, D, e->ov_hn};
    const QuantOut q_att{e->att_q, e->QD, e->sca_att, e->oc_att, e->ol_att, e->QD, e->ov_att};
    const QuantOut q_act{e->act_q, FF, e->sca_act, e->oc_act, e->ol_act, FF, e->ov_act};
    auto deq = [&](const QuantOut& q, const QW& w, int K, const bf16_t* x16, int N) { return deq_info(e, q, w, K, x16, N); };
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
    lm_step(e, R);
    launch_greedy(greedy_args(e, R, dump), e->st);
}

// one decode step for R rows: sx ([R][d]) -> next token (generation/utils.py:2876-2943)
static void decode_step(sonic_engine* e, int R, bool dump) {
    if (e->f32) { decode_step_f32(e, R, dump); return; }
    if (e->i8) { decode_step_i8(e, R, dump); return; }
    const sonic_dims& d = e->d;
    const int D = d.dec_d, mpad = ((R + 15) / 16) * 16, dt = e->dt;
    const StepForm f = step_form(e, R);
    const int ogu = !f.fuse_gu ? OGU_UNFUSED : !f.fuse_o ? OGU_HALF_FUSED : f.split_norm ? OGU_SPLIT_NORM : OGU_FUSED;
    e->step_launches_per_layer = (f.gemv || f.fp8) ? 5 : !f.fuse_o ? 8 : f.pre ? 5 : f.split_norm ? 7 : 6;
    if (f.fp8) { ++e->fp8_step_builds; decode_step_gemv(e, R, dump, true); return; }
    if (f.gemv) { decode_step_gemv(e, R, dump, false); return; }
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
    lm_step(e, R);
    launch_greedy(greedy_args(e, R, dump), e->st);
}

// A captured chunk of the greedy loop: `n` token steps for `R` rows as ONE hipGraph (kv_len / tok_pos / the token ids live on the device, so
// the steps of a chunk need nothing from the host).
// svc: the chunk belongs to a continuous decode loop (sonic_service_*), i.e. it runs beside a prefill slot and other loops by design - decode_step then
// picks the forms that cost the fewest CU-microseconds rather than the shortest chain (gu64_split_norm).  Same bits either way; cached separately.
int chunk_graph(sonic_engine* e, int R, int n, hipGraphExec_t* out, bool svc) {
    const std::pair<int, int> key{R + (svc ? GK_SVC : 0) + (e->opt_token_logprobs ? GK_LP : 0) + (e->gen_on ? GK_GUARD : 0) + e->opt_top_logprobs * GK_TOPK + req_graph_key(e), n};   // (the LP / GUARD / BIAS / SAMPLE / TOPK / GRAMMAR / LM greedy kernel and its pointers are part of the capture)
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
