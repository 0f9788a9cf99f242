// sonic_hip engine: the runs and passes that score GIVEN tokens from a prefill - the parallel forced run with its word timestamps, and the verify pass of a drafted
// prefill; their buffers, the align launches' descriptor and the one score pass both go through.
#include "engine_internal.h"

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
    if (e->opt_forced_share_prompt && !e->pre_row) TRY(dalloc(e, &e->pre_row, 2 * 64));
    if (!e->score_plan_d) TRY(dalloc(e, &e->score_plan_d, ScorePlan::row_words(e->tok_cap)));
    if (!e->score_plan_h && hipHostMalloc((void**)&e->score_plan_h, ScorePlan::words(e->tok_cap) * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(e, SONIC_ERR_OOM, "forced_parallel: pinned host memory exhausted"); }
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
    const size_t plan = AlignPlan::words(e->tok_cap);
    if (!e->align_plan_d) { TRY(dalloc(e, &e->align_plan_d, plan)); e->align_plan_cap = plan; }
    if (!e->align_plan_h && hipHostMalloc((void**)&e->align_plan_h, plan * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(e, SONIC_ERR_OOM, "forced_align: pinned host memory exhausted"); }
    return SONIC_OK;
}
// the word-timestamp launches (align.hip) over the handle's align plan and buffers: Q = the roped query rows, K = the audio keys as the strides say
// (the prefill: a layer's K cache; the hook: caller rows), `heads` = n_heads ascending head ids on the device
AlignArgs align_probs_args(sonic_engine* e, const bf16_t* Q, const bf16_t* K, long k_ld, long k_head_stride, long k_seq_stride, const int* heads, int n_heads, int Hq, int Hkv, const int* rec) {
    AlignArgs a{};
    const AlignPlan ap(e->align_plan_d, e->tok_cap);
    a.Q = Q; a.q_ld = Hq * 128L; a.K = K; a.k_ld = k_ld; a.k_head_stride = k_head_stride; a.k_seq_stride = k_seq_stride;
    a.qrow = ap.qrow; a.rseq = ap.rseq; a.seqp = ap.seq; a.heads = heads; a.rec = rec;
    a.n_heads = n_heads; a.grp = Hq / Hkv; a.S = e->align_S; a.n_seq = e->align_nseq; a.A_max = e->align_Amax; a.L_max = e->align_Lmax; a.dt = e->dt;
    a.scale = 1.0f / sqrtf(128.f); a.h_total = (float)e->align_Htot;
    a.P = e->align_P; a.Z = e->align_P + e->align_Zoff; a.M = e->align_M; a.t_out = e->align_t; a.trace = e->align_trace;
    return a;
}

// The score pass both kinds of run end their prefill with: the final norm of the S hidden rows that row_map names into dhn (free behind the last layer), then, in
// chunks of score_chunk_rows, the tied lm_head as one prefill-family GEMM into score_logits and per_chunk(c0, n), the caller's row kernel over rows c0 .. c0 + n
template <typename F> static void score_pass(sonic_engine* e, const int* row_map, int S, F per_chunk) {
    const sonic_dims& d = e->d;
    if (e->f32) f32_score_norm(e, row_map, S);
    else launch_rmsnorm(e->dx, e->dec_nw, e->dhn, S, d.dec_d, d.dec_rms_eps, row_map, e->st, e->dt);
    const int chunk = std::min(e->opt_score_chunk_rows, e->score_rows_cap);
    for (int c0 = 0; c0 < S; c0 += chunk) {
        const int n = std::min(chunk, S - c0);
        if (e->f32) f32_score_logits(e, c0, n, (float*)e->score_logits);
        else gemm(e, EPI_BIAS, e->dhn + (size_t)c0 * d.dec_d, d.dec_d, e->embed_t, nullptr, (bf16_t*)e->score_logits, d.vocab, n, d.vocab, d.dec_d, nullptr, 0, 1);   // embed_t: launch_tile_weights' tiling, the one GemmArgs.w_tiled reads
        per_chunk(c0, n);
    }
}

// Draft-verified decoding (option draft_verify), behind the prefill's last layer: draft position n of request r is decided by the hidden row at
// q_off[r] + P - 1 + n.  The S = sum D_r rows go through the score pass, reduced by rows_kernel<T, true, ...> (rows.hip) under the handle's processors; draft_accept_kernel then leaves
// every drafted request where a prefill of prompt || draft[0 .. a) would have left it.  The head that follows is the one of every prefill
void run_draft_verify(sonic_engine* e, int R, const HostPlan& hp) {
    const sonic_dims& d = e->d;
    const DraftPlan pd(e->draft_plan_d, hp.S);
    RowsArgs va{};
    va.logits = e->score_logits; va.ld = d.vocab; va.V = d.vocab; va.dt = e->dt;
    if (e->gen_on && e->hist) { va.hist = e->hist; va.hist_ld = e->max_ctx; va.rep_penalty = e->gen_penalty; va.ngram = e->gen_ngram; va.suppress = e->gen_suppress_d; va.n_suppress = (int)e->gen_suppress.size(); }
    va.topk = lp_on(e) ? e->opt_top_logprobs : 0;
    va.dump = e->run_logits ? e->dump : nullptr; va.out_ld = e->out_cap; va.R = R; va.lp_by_row = true;
    score_pass(e, pd.hidden, hp.S, [&](int c0, int n) {
        va.n = n; va.target = pd.target + c0; va.rec = pd.rec + c0; va.hrow = pd.hrow + c0; va.hlen = pd.hlen + c0;
        va.choice = e->ver_tok + c0; va.out_lp = e->ver_rec + (size_t)c0 * lp_width(e);
        launch_rows(va, e->st);
    });
    DraftAcceptArgs da{};
    da.req = pd.req; da.draft = pd.target; da.ver_tok = e->ver_tok; da.ver_rec = e->ver_rec; da.lp_w = lp_width(e);
    da.out_ids = e->out_ids; da.out_lp = lp_on(e) ? e->out_lp : nullptr; da.out_ld = e->out_cap;
    da.n_new = e->n_new; da.kv_len = e->kv_len; da.tok_pos = e->tok_pos; da.step_counter = e->step_ctr; da.last_row = e->last_row; da.accepted = e->draft_acc;
    launch_draft_accept(da, R, e->st);
}

// The parallel forced run (option forced_parallel with forced ids set; include/sonic_hip.h beside sonic_set_forced_ids).  Under teacher forcing no
// input depends on an output, so the run is ONE prefill: sequence r = prompt || forced[r][0 .. L_r - 1), L_r = 1 + the index of the first EOS id among its budget's
// forced ids (HF's rule; the budget if there is none).  Token n of sequence r is scored by the hidden state at row q_off[r] + P - 1 + n: the S = sum L_r score rows are
// the rows of the score pass, reduced by rows_kernel<T, false, ...> (rows.hip), which also writes the forced ids to out_ids and, if asked, the rows to the step-logits dump.
// No logits processor is applied.  forced_fanout = N: the R sequences are R / N audio requests (windows, log-mel, encoder, projector once each) with N candidates
// each; the prefill's outlier groups stay per sequence.  The handle is left holding a finished batch.
int run_forced_parallel(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new, bool want_logits) {
    const sonic_dims& d = e->d;
    const auto t_host0 = std::chrono::steady_clock::now();
    TRY(run_refuse_unready(e));
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
    // option forced_share_prompt: the first sequence of every group of N packs prompt || forced[0 .. L - 1) as ever, the others only their forced[0 .. L - 1),
    // at positions P on of their own cache row - their attention reads keys [0, P) from the first one's row.  The option's own setter has refused the kinds and options
    // that cannot share (engine_options.cpp: forced_align among them, either way round, so `align` below is never true beside it); what is left to check is that a
    // group's prompts ARE one prompt
    const bool share = e->opt_forced_share_prompt != 0;
    for (int r = 0; share && r < R; ++r) {
        const int o = r - r % N;
        const int64_t n = prompt_off[r + 1] - prompt_off[r];
        if (n != prompt_off[o + 1] - prompt_off[o] || memcmp(prompt_ids + prompt_off[r], prompt_ids + prompt_off[o], (size_t)n * 4))
            return fail(e, SONIC_ERR_INVALID, "forced_share_prompt: sequences %d and %d of one group bring different prompts (the candidates of one audio share ONE prompt)", o, r);
    }
    // the longer sequences: prompt || forced[0 .. L - 1); their budget max_new - (L - 1) keeps plan_requests' context check at prompt + max_new
    std::vector<int32_t> ids, left(R), L(R), pos0(R, 0); std::vector<int64_t> off(R + 1, 0);
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
        const bool suffix = share && r % N;
        if (suffix) pos0[r] = (int32_t)(p1 - p0);
        else ids.insert(ids.end(), prompt_ids + p0, prompt_ids + p1);
        ids.insert(ids.end(), f, f + l - 1);
        off[r + 1] = (int64_t)ids.size(); L[r] = l; left[r] = max_new[r] - (l - 1);
        asked += (suffix ? 0 : p1 - p0) + l - 1;
    }
    if (asked > e->tok_cap) return fail(e, SONIC_ERR_INVALID, "forced_parallel: the run asks for %ld tokens (prompts and forced ids), %d fit one prefill (tok_cap)", asked, e->tok_cap);
    HostPlan hp;
    TRY(plan_requests(e, req_win, R, ids.data(), off.data(), left.data(), hp, N, share ? pos0.data() : nullptr));
    if (share) {
        hp.pre_row.resize(R); hp.pre_len = pos0;
        for (int r = 0; r < R; ++r) hp.pre_row[r] = r - r % N;      // (the first of a group reads its own row: pre_len 0)
    }
    e->score_tokens = hp.n_tok;
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
    TRY(run_wait_spliced(e));      // (behind the refusals above: a refused run leaves the wait to the next one)
    if (align) TRY(align_alloc(e, al_S, al_Amax, al_Hmax));
    TRY(score_alloc(e));
    TRY(run_pick_plan_buffer(e));
    e->R = R; e->max_steps = max_steps; e->last_maxnew = hp.max_new;
    e->last_qlen.resize(R);
    for (int r = 0; r < R; ++r) e->last_qlen[r] = (int)(prompt_off[r + 1] - prompt_off[r]);      // the PROMPT's length: fetch_locked expects kv_len = prompt + tokens - 1
    TRY(run_reserve_dump(e, want_logits, max_steps, max_steps, R));
    // the score rows: hidden-state row | target | record index, S of each, then the rows' closing state (n_new | finished | tok_pos | n_active)
    int S = 0;
    for (int r = 0; r < R; ++r) S += L[r];
    const ScorePlan ph(e->score_plan_h, S), pd(e->score_plan_d, S);
    memset(ph.n_new, 0, ScorePlan::state_words() * 4);
    for (int r = 0, s = 0; r < R; ++r) {
        const int P = e->last_qlen[r];
        const int* f = e->force_h.data() + (size_t)r * e->force_ld;
        // (a shared prompt: token 0 of every sequence of a group is scored from the ONE hidden row the prompt ends in - the first sequence's - and token n >= 1 of a suffix from its row n - 1)
        const int o = share ? r - r % N : r, h0 = hp.q_off[o] + P - 1;
        for (int n = 0; n < L[r]; ++n, ++s) { ph.hidden[s] = (o == r || n == 0) ? h0 + n : hp.q_off[r] + n - 1; ph.target[s] = f[n]; ph.rec[s] = r * e->out_cap + n; }
        ph.n_new[r] = L[r]; ph.finished[r] = 1; ph.tok_pos[r] = P + L[r] - 2;
    }
    for (int r = R; r < PLAN_REQ_WORDS; ++r) ph.finished[r] = 0;

    e->align_last = false;
    if (align) {      // the align plan: per score row its query row and sequence, per sequence row0 | L | a0 | A, the heads layer by layer; M starts at zero
        const AlignPlan ah(e->align_plan_h, e->tok_cap), ad(e->align_plan_d, e->tok_cap);
        for (int r = 0, sr = 0; r < R; ++r) {
            int* sp = ah.seq + 4 * r;
            sp[0] = sr; sp[1] = L[r]; sp[2] = al_a0[r]; sp[3] = al_A[r];
            for (int n = 0; n < L[r]; ++n, ++sr) { ah.qrow[sr] = ph.hidden[sr]; ah.rseq[sr] = r; }
        }
        int* hh = ah.heads;
        for (int l = 0; l < d.dec_layers; ++l) for (size_t i = 0; i < e->align_layer_heads[l].size(); ++i) hh[e->align_layer_off[l] + i] = e->align_layer_heads[l][i];
        HIPC(e, hipMemcpyAsync(ad.qrow, ah.qrow, (size_t)S * 4, hipMemcpyHostToDevice, e->st));
        HIPC(e, hipMemcpyAsync(ad.rseq, ah.rseq, (size_t)S * 4, hipMemcpyHostToDevice, e->st));
        HIPC(e, hipMemcpyAsync(ad.seq, ah.seq, AlignPlan::tail_words() * 4, hipMemcpyHostToDevice, e->st));
        e->align_S = S; e->align_nseq = R; e->align_Amax = al_Amax; e->align_Lmax = al_Lmax; e->align_last_heads = 0;
        for (size_t o = 0; o < (size_t)S * al_Amax; o += (size_t)1 << 30) launch_fill_i32((int*)e->align_M + o, 0, (int)std::min((size_t)1 << 30, (size_t)S * al_Amax - o), e->st);
        e->align_live = true;
    }
    struct AlignOff { sonic_engine* e; ~AlignOff() { e->align_live = false; } } align_off{e};      // whatever way the run leaves
    (void)hipEventRecord(e->ev[0], e->st);
    TRY(run_mel(e, e->W, e->f32));
    (void)hipEventRecord(e->ev[1], e->st);
    const int A = R / N;
    TRY(run_upload_win_req(e, req_win, A));      // the encoder's outlier groups are the audio requests, not their candidates
    TRY(e->f32 ? f32_run_encoder(e, e->W, nullptr, nullptr) : run_encoder(e, e->W, nullptr, nullptr, A));
    (void)hipEventRecord(e->ev[2], e->st);
    TRY(e->f32 ? f32_run_prefill(e, R, hp, false) : run_prefill(e, R, hp, false));
    HIPC(e, hipMemcpyAsync(pd.hidden, ph.hidden, ScorePlan::row_words(S) * 4, hipMemcpyHostToDevice, e->st));
    if (align) {      // DTW over the finished M: t_n beside the records (rec: the score plan's record indices)
        launch_align_dtw(align_probs_args(e, e->dq, e->Kc, 128, e->max_ctx * 128L, (long)d.dec_kv_heads * e->max_ctx * 128, nullptr, 0, d.dec_heads, d.dec_kv_heads, pd.rec), e->st);
        e->align_live = false; e->align_last = true;
    }
    RowsArgs sa{};
    sa.logits = e->score_logits; sa.ld = d.vocab; sa.V = d.vocab; sa.dt = e->f32 ? DT_F32 : e->dt;
    sa.out_ids = e->out_ids; sa.out_lp = lp_on(e) ? e->out_lp : nullptr; sa.topk = sa.out_lp ? e->opt_top_logprobs : 0;
    sa.dump = want_logits ? e->dump : nullptr; sa.out_ld = e->out_cap; sa.R = R;
    score_pass(e, pd.hidden, S, [&](int c0, int n) {
        sa.n = n; sa.target = pd.target + c0; sa.rec = pd.rec + c0;
        launch_rows(sa, e->st);
    });
    // the rows' state as a finished batch: n_new = L, finished, tok_pos = kv_len - 1 (kv_len = prompt + L - 1 is what the plan uploaded), nothing running
    HIPC(e, hipMemcpyAsync(e->n_new, ph.n_new, PLAN_REQ_WORDS * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(e->finished, ph.finished, PLAN_REQ_WORDS * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(e->tok_pos, ph.tok_pos, (size_t)R * 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, hipMemcpyAsync(e->n_active, ph.n_active, 4, hipMemcpyHostToDevice, e->st));
    (void)hipEventRecord(e->ev[3], e->st);
    (void)hipEventRecord(e->ev[4], e->st);
    e->steps_run = max_steps - 1; e->greedy_calls = max_steps; e->spliced = 0;      // a finished batch: sonic_decode_step has nothing left to run
    const double host_enqueue_first = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
    run_zero_host_figures(e);
    return run_close(e, host_enqueue_first, 0);
}
