// sonic_hip engine: continuous decoding (splice / service kernels and entry points), the asynchronous worker, the stage entry points (log-mel, encode,
// prefill, decode step, fetch), teacher forcing and timings.
#include "engine_internal.h"

// ---- continuous decoding (VERDICT r3 item 8 "row refill", generalised): one handle decodes forever over a pool of Bm rows, requests join and
// leave row by row.  The reference serialises every decode of every session (backend/connection_manager.py:127-245 awaits one transcribe() at a
// time per connection, backend/transcription_manager.py:58 blocks the event loop); a batch engine makes a request wait for the running batch to
// end and pads every batch to its slowest row.  Here a request is prefilled on ANOTHER handle of the same weights (sonic_prefill on a slot: log-mel,
// encoder, prompt forward, first token), its row - KV cache, control words, next-step input - is copied into a free row of the decoding handle
// between two chunks of its greedy loop, and the row is handed back the moment it hits EOS / its budget.  Rows are independent in every decode
// kernel and sum in a fixed order (batch invariance up to 32 rows), so a request's tokens are the same bits as in a solo run.  (SpliceArgs, the copy's descriptor: engine_internal.h)
__global__ __launch_bounds__(256) void splice_kv_kernel(SpliceArgs a) {
    const int i = blockIdx.x, lh = blockIdx.y, s = a.src[i], d = a.dst[i];
    const int len = min(max(a.kv_len_s[s], 1), a.ctx);
    const long blk = (long)a.ctx * a.hd;
    const long so = ((long)(lh / a.Hkv) * a.Bm + s) * a.Hkv + lh % a.Hkv, dd = ((long)(lh / a.Hkv) * a.Bm + d) * a.Hkv + lh % a.Hkv;
    const uint4* ks = (const uint4*)(a.Ks + so * blk); uint4* kd = (uint4*)(a.Kd + dd * blk);
    const uint4* vs = (const uint4*)(a.Vs + so * blk); uint4* vd = (uint4*)(a.Vd + dd * blk);
    const int n16 = len * a.hd / 8;
    for (int j = threadIdx.x; j < n16; j += 256) { kd[j] = ks[j]; vd[j] = vs[j]; }
}
__global__ __launch_bounds__(256) void splice_state_kernel(SpliceArgs a) {
    const int i = blockIdx.x, s = a.src[i], d = a.dst[i], t = threadIdx.x;
    for (int j = t; j < a.D / 8; j += 256) {
        ((uint4*)(a.sx_d + (long)d * a.D))[j] = ((const uint4*)(a.sx_s + (long)s * a.D))[j];
        ((uint4*)(a.shn_d + (long)d * a.D))[j] = ((const uint4*)(a.shn_s + (long)s * a.D))[j];
    }
    if (a.hq_s) {
        for (int j = t; j < a.D / 16; j += 256) ((uint4*)(a.hq_d + (long)d * a.D))[j] = ((const uint4*)(a.hq_s + (long)s * a.D))[j];
        const int cnt = a.oc_s[s];
        for (int j = t; j < cnt; j += 256) { a.ol_d[(long)d * a.D + j] = a.ol_s[(long)s * a.D + j]; a.ov_d[(long)d * a.D + j] = a.ov_s[(long)s * a.D + j]; }
        if (t == 0) { a.sca_d[d] = a.sca_s[s]; a.oc_d[d] = cnt; }
    }
    if (a.hist_d) {
        const int len = min(max(a.kv_len_s[s], 0) + 1, a.ctx);      // (a row that stopped at its first token kept kv_len = prompt: its token sits at [kv_len])
        for (int j = t; j < len; j += 256) a.hist_d[(long)d * a.ctx + j] = a.hist_s[(long)s * a.ctx + j];
    }
    if (a.bias_d) {
        const int cnt = min(max(a.bias_s[s], 0), BIAS_MAX_ENTRIES);
        if (t == 0) a.bias_d[d] = cnt;
        for (int j = t; j < cnt * BIAS_ENTRY_WORDS; j += 256) a.bias_d[64 + (long)d * BIAS_ROW_WORDS + j] = a.bias_s[64 + (long)s * BIAS_ROW_WORDS + j];
    }
    if (a.samp_d && t < 3) a.samp_d[3 * d + t] = a.samp_s[3 * s + t];
    if (a.trunc_d && t < 3) a.trunc_d[3 * d + t] = a.trunc_s[3 * s + t];
    if (a.lm_d && t == 0) { a.lm_d[d] = a.lm_s[s]; a.lm_d[64 + d] = a.lm_s[64 + s]; }      // the language model's state and pending token
    if (a.gram_d && t == 0) { a.gram_d[d] = a.gram_s[s]; ((int*)(a.gram_d + 64))[d] = ((int*)(a.gram_s + 64))[s]; a.gram_s[s] = 0ull; ((int*)(a.gram_s + 64))[s] = -1; }
    const int cnt = min(max(a.n_new_s[s], 1), a.out_ld);      // the tokens that came out of the prefill: one - or, behind an accepted draft (option draft_verify), several
    if (a.lp_d) for (int j = t; j < cnt * a.lp_w; j += 256) a.lp_d[(long)d * a.out_ld * a.lp_w + j] = a.lp_s[(long)s * a.out_ld * a.lp_w + j];
    for (int j = t; j < cnt; j += 256) a.out_d[(long)d * a.out_ld + j] = a.out_s[(long)s * a.out_ld + j];
    if (t == 0) {
        const int fin = a.fin_s[s];
        a.kv_len_d[d] = a.kv_len_s[s]; a.tok_pos_d[d] = a.tok_pos_s[s]; a.n_new_d[d] = a.n_new_s[s]; a.max_new_d[d] = a.max_new_s[s];
        a.fin_d[d] = fin;
        if (a.mirrored_d) a.mirrored_d[d] = 0;      // the new occupant's tokens are not in the pinned mirror (service_status_kernel copies them when it finds the row finished)
        if (!fin) atomicAdd(a.n_active_d, 1);
    }
}
// a fetched row goes back to the pool: it stays `finished` (frozen: it emits nothing) and looks at one key only until it is reused
// (gram_state, option grammar: the row is free again - its blocks must not read an automaton that may be destroyed once the row's reference is gone)
__global__ void release_row_kernel(int* kv_len, int* tok_pos, int* finished, int row, int* gram_state) { kv_len[row] = 1; tok_pos[row] = 0; finished[row] = 1; if (gram_state) gram_state[row] = -1; }
// the pipelined check of the continuous loop: finished | n_new | n_active -> one record in pinned host memory (a kernel's stores instead of
// three copy commands between every two chunks)
// ... and, in the same launch, the finished rows' mirror: block r < m.rows looks at row r and, in the chunk that finds it finished, copies its n_new ids (and
// log-probability records) from out_ids / out_lp into the pinned arrays the host fetches from (plain vector stores, as the record's); a chunk in which no row
// finishes copies nothing.  The last block writes the record.  The host reads both only behind the chunk's event.  (m.rows == 0: option fetch_stream, no mirror)
struct MirrorArgs { const int* out_ids; const float* out_lp; int* mirrored; int* ids_h; float* lp_h; int out_cap, lp_w, rows; };
__global__ __launch_bounds__(256) void service_status_kernel(const int* finished, const int* n_new, const int* n_active, int* out, MirrorArgs m) {
    const int t = threadIdx.x, row = blockIdx.x;
    if (row < m.rows) {
        if (!finished[row] || m.mirrored[row]) return;      // (the same answer for the whole block)
        const int n = min(max(n_new[row], 0), m.out_cap);
        const long o = (long)row * m.out_cap;
        for (int j = t; j < n; j += 256) m.ids_h[o + j] = m.out_ids[o + j];
        if (m.lp_h) for (int j = t; j < n * m.lp_w; j += 256) m.lp_h[o * m.lp_w + j] = m.out_lp[o * m.lp_w + j];
        __syncthreads();                                    // every thread has read the flag
        if (t == 0) m.mirrored[row] = 1;
        return;
    }
    if (t < 64) { out[t] = finished[t]; out[64 + t] = n_new[t]; }
    if (t == 0) out[128] = *n_active;
}
__global__ void service_reset_kernel(int* kv_len, int* tok_pos, int* n_new, int* finished, int* max_new, int* n_active, int* mirrored) {
    const int b = threadIdx.x;
    if (b < 64) { kv_len[b] = 1; tok_pos[b] = 0; n_new[b] = 0; finished[b] = 1; max_new[b] = 1; mirrored[b] = 1; }      // (a free row has nothing to mirror)
    if (b == 0) *n_active = 0;
}
// the pinned mirror of one continuously decoding handle, at the widths its options ask for now (sonic_service_begin)
static int mirror_alloc(sonic_engine* e) {
    if (!e->svc_out_h) HIPC(e, hipHostMalloc((void**)&e->svc_out_h, (size_t)64 * e->out_cap * 4, hipHostMallocDefault));
    const int w = lp_on(e) ? lp_width(e) : 0;
    if (w != e->svc_lp_w) {
        if (e->svc_lp_h) { (void)hipHostFree(e->svc_lp_h); e->svc_lp_h = nullptr; }
        e->svc_lp_w = 0;
        if (w) { HIPC(e, hipHostMalloc((void**)&e->svc_lp_h, (size_t)64 * e->out_cap * w * 4, hipHostMallocDefault)); e->svc_lp_w = w; }
    }
    return SONIC_OK;
}
// the mirror holds what a fetch of this row asks for: a check newer than the row's splice has shown it finished (and the records are as wide as the handle's)
static inline bool mirror_valid(const sonic_engine* e, int row, bool want_lp) {
    if (e->opt_fetch_stream || !e->svc_out_h || e->svc_checked < 1) return false;
    if (want_lp && !(e->svc_lp_h && e->svc_lp_w == lp_width(e))) return false;
    return e->svc_seq > e->spliced_seq[row] && e->svc_fin[row];
}
// option fetch_stream (A/B): the handle's second stream, as every decoding handle had before the mirror
static int fetch_stream(sonic_engine* e, hipStream_t* st) {
    if (!e->st_io) HIPC(e, hipStreamCreateWithFlags(&e->st_io, hipStreamNonBlocking));
    *st = e->st_io;
    return SONIC_OK;
}

extern "C" int sonic_service_begin(sonic_engine* e) {
    if (e && e->f32) return SONIC_ERR_UNSUPPORTED;
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    if (!e->finalized) return fail(e, SONIC_ERR_INVALID, "weights not finalized");
    if (e->svc_on) return SONIC_OK;
    if (e->opt_forced_parallel) return fail(e, SONIC_ERR_INVALID, "sonic_service_begin: option forced_parallel is on: a scoring handle does not decode continuously");
    TRY(mirror_alloc(e));
    if (e->opt_fetch_stream) { hipStream_t s; TRY(fetch_stream(e, &s)); }      // (A/B: where every decoding handle's second stream used to be created)
    HIPC(e, stream_sync(e));
    hipLaunchKernelGGL(service_reset_kernel, dim3(1), dim3(64), 0, e->st, e->kv_len, e->tok_pos, e->n_new, e->finished, e->max_new_d, e->n_active, e->mirrored);
    if (e->force_d) return fail(e, SONIC_ERR_INVALID, "teacher forcing is set: clear it before continuous decoding");
    req_rows_free(e);                                       // the pool starts with free rows
    hipGraphExec_t gx = nullptr;                            // the chunk graphs exist before the first splice: nothing captures on this stream later
    if (e->Bm >= 2 && !e->i8) TRY(chunk_graph(e, 2, e->opt_decode_chunk > 0 ? e->opt_decode_chunk : 1, &gx, true));   // a pool with at most two occupied rows (round 6: five launches per layer)
    if (e->Bm >= 4 && !e->i8 && (e->opt_decode_gemv || fp8_chain_on(e))) TRY(chunk_graph(e, 4, e->opt_decode_chunk > 0 ? e->opt_decode_chunk : 1, &gx, true));   // ... four, on the GEMV chain (opt-in) or the fp8 chain (mode fp8)
    for (int R = 16; ; R += 16) {                           // one per 16 rows (sonic_service_step runs as many rows as are occupied)
        const int r = R < e->Bm ? R : e->Bm;
        TRY(chunk_graph(e, r, e->opt_decode_chunk > 0 ? e->opt_decode_chunk : 1, &gx, true));
        if (r >= e->Bm) break;
    }
    HIPC(e, stream_sync(e));
    e->svc_launched = e->svc_checked = 0; e->svc_seq = 0; e->svc_active = 0;
    for (int b = 0; b < 64; ++b) { e->svc_fin[b] = 1; e->svc_nn[b] = 0; e->spliced_seq[b] = 0; }
    e->R = 0; e->greedy_calls = 0;
    e->svc_on = true;
    return SONIC_OK;
}
extern "C" int sonic_service_end(sonic_engine* e) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    if (!e->svc_on) return SONIC_OK;
    HIPC(e, stream_sync(e));
    if (getenv("SONIC_SVC_STATS")) fprintf(stderr, "[sonic] continuous loop: %lld chunks queued, %lld launches found the stream empty with rows running, lookahead %d at the end\n",
                                           (long long)e->svc_launched, (long long)e->svc_dry, e->lookahead);
    e->svc_on = false;
    return SONIC_OK;
}
// n rows of `p` (requests 0 .. R-1 of its last sonic_prefill) -> rows dst_rows[] of the continuously decoding handle `d` (free rows: never
// spliced, or fetched since).  Queued on d's stream behind p's prefill; p's next run waits for the copies on the device.  *seq_out = chunks d
// had queued before the splice: checks with a larger sequence number (sonic_service_step) describe the new occupants of these rows.
extern "C" int sonic_splice_rows(sonic_engine* d, sonic_engine* p, int n, const int32_t* src_rows, const int32_t* dst_rows, int64_t* seq_out) {
    if (!d || !p || !src_rows || !dst_rows || d == p) return SONIC_ERR_INVALID;
    std::unique_lock<std::mutex> l1(d->mu, std::defer_lock), l2(p->mu, std::defer_lock);
    std::lock(l1, l2);
    (void)hipGetLastError();
    HIPC(d, hipSetDevice(d->device)); g_opts = d->opts;
    if (d->opt_forced_parallel || p->opt_forced_parallel) return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: option forced_parallel is on for the %s: a scoring handle takes no part in continuous decoding", d->opt_forced_parallel ? "destination" : "source");
    if (!d->svc_on) return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: the destination is not decoding continuously (sonic_service_begin)");
    if ((d->owner ? d->owner : d) != (p->owner ? p->owner : p)) return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: the handles do not share weights");
    if (d->Bm != p->Bm || d->max_ctx != p->max_ctx) return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: the handles differ in max_batch / max_ctx");
    if (d->opt_token_logprobs && !lp_on(p))
        return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: the destination has option token_logprobs on, the source prefilled without it");
    if (d->opt_token_logprobs && d->opt_top_logprobs != p->opt_top_logprobs)
        return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: source and destination differ in option top_logprobs (%d and %d): set it on the owner before its slots are created", p->opt_top_logprobs, d->opt_top_logprobs);
    // (either way round: a row whose first token was chosen with guards must not go on without them, nor the reverse)
    if (d->gen_on != p->gen_on || (d->gen_on && !(p->hist && d->hist && p->gen_penalty == d->gen_penalty && p->gen_ngram == d->gen_ngram && p->gen_suppress == d->gen_suppress)))
        return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: source and destination differ in their generation guards (sonic_set_generation): set them on the owner before its slots are created");
    TRY(req_splice_check(d, p));
    if (n < 1 || n > 64 || p->greedy_calls < 1 || n > p->R) return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: %d rows, the source has %d prefilled requests", n, p->greedy_calls < 1 ? 0 : p->R);
    SpliceArgs a{};
    for (int i = 0; i < n; ++i) {
        if (src_rows[i] < 0 || src_rows[i] >= p->R || dst_rows[i] < 0 || dst_rows[i] >= d->Bm) return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: row out of range");
        for (int j = 0; j < i; ++j) if (dst_rows[j] == dst_rows[i]) return fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: destination row %d named twice", dst_rows[i]);
        a.src[i] = src_rows[i]; a.dst[i] = dst_rows[i];
    }
    const sonic_dims& dm = d->d;
    a.Ks = p->Kc; a.Vs = p->Vc; a.Kd = d->Kc; a.Vd = d->Vc; a.layers = dm.dec_layers; a.Bm = d->Bm; a.Hkv = dm.dec_kv_heads; a.ctx = d->max_ctx; a.hd = dm.dec_head_dim;
    a.kv_len_s = p->kv_len; a.tok_pos_s = p->tok_pos; a.n_new_s = p->n_new; a.fin_s = p->finished; a.max_new_s = p->max_new_d; a.out_s = p->out_ids; a.out_ld = d->out_cap;
    a.kv_len_d = d->kv_len; a.tok_pos_d = d->tok_pos; a.n_new_d = d->n_new; a.fin_d = d->finished; a.max_new_d = d->max_new_d; a.out_d = d->out_ids; a.n_active_d = d->n_active;
    a.sx_s = p->sx; a.shn_s = p->shn; a.sx_d = d->sx; a.shn_d = d->shn; a.D = dm.dec_d;
    a.mirrored_d = d->mirrored;
    if (lp_on(d)) { a.lp_s = p->out_lp; a.lp_d = d->out_lp; a.lp_w = lp_width(d); }
    if (hist_on(d)) { a.hist_s = p->hist; a.hist_d = d->hist; }
    req_splice_args(d, p, a, src_rows, dst_rows, n);      // the per-request stages' rows; a row's grammar reference is handed over with it
    if (d->i8) { a.hq_s = p->hn_q; a.hq_d = d->hn_q; a.sca_s = p->sca_hn; a.sca_d = d->sca_hn; a.oc_s = p->oc_hn; a.oc_d = d->oc_hn; a.ol_s = p->ol_hn; a.ol_d = d->ol_hn; a.ov_s = p->ov_hn; a.ov_d = d->ov_hn; }
    HIPC(d, hipEventRecord(p->xfer_ev, p->st));
    HIPC(d, hipStreamWaitEvent(d->st, p->xfer_ev, 0));
    hipLaunchKernelGGL(splice_kv_kernel, dim3(n, dm.dec_layers * dm.dec_kv_heads), dim3(256), 0, d->st, a);
    hipLaunchKernelGGL(splice_state_kernel, dim3(n), dim3(256), 0, d->st, a);
    HIPC(d, hipEventRecord(d->splice_ev, d->st));
    // (rows of one prefill may go to several decoders: an earlier splice's event is not forgotten, the source's stream takes it on now)
    if (p->wait_pending && p->wait_ev != d->splice_ev) HIPC(d, hipStreamWaitEvent(p->st, p->wait_ev, 0));
    p->wait_ev = d->splice_ev; p->wait_pending = true;
    HIPC(d, hipGetLastError());
    for (int i = 0; i < n; ++i) p->spliced |= 1ull << src_rows[i];      // (gen_busy: a prefill slot whose rows have all left is free again)
    for (int i = 0; i < n; ++i) d->spliced_seq[dst_rows[i]] = d->svc_launched;      // (the mirror of these rows describes their new occupants behind a later check)
    if (seq_out) *seq_out = d->svc_launched;
    return SONIC_OK;
}
// queue n_chunks more chunks of the endless greedy loop over all Bm rows and return the newest check the device has completed: finished[64]
// (1 = the row hit EOS / its budget, or is free), n_new[64] (tokens the row holds), *seq_out = number of the chunk that check followed (0:
// none yet), *n_active_out = rows still running then.  Blocks only while more than `lookahead` chunks are unchecked (adaptive, as the batch loop).
extern "C" int sonic_service_step(sonic_engine* e, int n_chunks, int rows, int32_t* finished_out, int32_t* n_new_out, int64_t* seq_out, int32_t* n_active_out) {
    if (!e || n_chunks < 0) return SONIC_ERR_INVALID;
    ENTER(e);
    if (!e->svc_on) return fail(e, SONIC_ERR_INVALID, "sonic_service_step needs sonic_service_begin");
    const int C = e->opt_decode_chunk > 0 ? e->opt_decode_chunk : 1;
    // rows: the caller's occupied rows all lie below this index (0: all); the chunk runs the next multiple of 16 (graphs captured at
    // sonic_service_begin) - a lightly loaded pool does not pay the step time of a full one (1.15 ms for 1-16 rows, 1.35 for 32, 1.83 for 64)
    int R = rows <= 0 || rows > e->Bm ? e->Bm : (rows + 15) / 16 * 16;
    if (R > e->Bm) R = e->Bm;
    if (rows > 0 && rows <= 2 && e->Bm >= 2 && !e->i8) R = 2;      // one or two sessions' rows: the <= 2-row step (same bits per row as any other row count)
    else if (rows > 0 && rows <= 4 && e->Bm >= 4 && !e->i8 && (e->opt_decode_gemv || fp8_chain_on(e))) R = 4;
    auto read_check = [&](bool block) -> int {
        const int i = (int)(e->svc_checked % CHK_RING);
        if (!block) { const hipError_t q = hipEventQuery(e->chk_ev[i]); if (q == hipErrorNotReady) { (void)hipGetLastError(); return 0; } if (q != hipSuccess) return -1; }
        else if (hipEventSynchronize(e->chk_ev[i]) != hipSuccess) return -1;
        const int* w = e->svc_h + (size_t)i * SVC_WORDS;
        memcpy(e->svc_fin, w, 64 * 4); memcpy(e->svc_nn, w + 64, 64 * 4); e->svc_active = w[128];
        e->svc_seq = ++e->svc_checked;
        if (e->svc_active < DEV_ERR_ACTIVE) return -2;
        return 1;
    };
    for (int c = 0; c <= n_chunks; ++c) {
        if (c < n_chunks) {
            // rows were running at the last check and the chunk queued last is already complete: the device has been idle waiting for this
            // thread (late by more than a chunk: descheduled, or behind other host work - the Python side of 128 sessions is).  Queue deeper.
            if (e->svc_launched > 0 && e->svc_active > 0 && hipEventQuery(e->chk_ev[(e->svc_launched - 1) % CHK_RING]) == hipSuccess) {
                e->lookahead = e->lookahead * 2 < CHK_MAX_AHEAD ? e->lookahead * 2 : CHK_MAX_AHEAD;
                e->svc_calm = 0; ++e->svc_dry;
            } else if (++e->svc_calm >= 64 && e->lookahead > 1) { e->lookahead /= 2; e->svc_calm = 0; }   // ... and shallower again after a calm stretch: a splice waits
                                                                                                            // behind the queue and finished rows are seen that many chunks late
            (void)hipGetLastError();
            hipGraphExec_t gx = nullptr;
            TRY(chunk_graph(e, R, C, &gx, true));
            HIPC(e, hipGraphLaunch(gx, e->st));
            const int slot = (int)(e->svc_launched % CHK_RING);
            int* w = e->svc_h + (size_t)slot * SVC_WORDS;
            MirrorArgs m{};                                 // all Bm rows, whatever the chunk stepped: a row spliced as finished (budget 1) is mirrored by the next chunk too
            if (!e->opt_fetch_stream && e->svc_out_h && e->mirrored) {
                m.out_ids = e->out_ids; m.mirrored = e->mirrored; m.ids_h = e->svc_out_h; m.out_cap = e->out_cap; m.rows = e->Bm;
                if (e->svc_lp_h && e->out_lp) { m.out_lp = e->out_lp; m.lp_h = e->svc_lp_h; m.lp_w = e->svc_lp_w; }
            }
            hipLaunchKernelGGL(service_status_kernel, dim3(m.rows + 1), dim3(256), 0, e->st, e->finished, e->n_new, e->n_active, w, m);
            HIPC(e, hipEventRecord(e->chk_ev[slot], e->st));
            ++e->svc_launched;
        }
        while (e->svc_checked < e->svc_launched) {
            const int r = read_check(e->svc_launched - e->svc_checked > e->lookahead);
            if (r == -2) return fail(e, SONIC_ERR_HIP, "continuous decode loop: a decode kernel gave up on an in-kernel wait, the rows' tokens are invalid");
            if (r < 0) return fail(e, SONIC_ERR_HIP, "continuous decode loop: check event failed: %s", hipGetErrorString(hipGetLastError()));
            if (r == 0) break;
        }
    }
    if (finished_out) memcpy(finished_out, e->svc_fin, 64 * 4);
    if (n_new_out) memcpy(n_new_out, e->svc_nn, 64 * 4);
    if (seq_out) *seq_out = e->svc_seq;
    if (n_active_out) *n_active_out = e->svc_active;
    return SONIC_OK;
}
// the n tokens of a finished row (n from sonic_service_step's n_new), then the row is free for the next splice
extern "C" int sonic_fetch_row(sonic_engine* e, int row, int n, int32_t* out_ids) {
    if (!e || !out_ids) return SONIC_ERR_INVALID;
    ENTER(e);
    if (!e->svc_on) return fail(e, SONIC_ERR_INVALID, "sonic_fetch_row needs sonic_service_begin");
    if (row < 0 || row >= e->Bm || n < 0 || n > e->out_cap) return fail(e, SONIC_ERR_INVALID, "sonic_fetch_row: row %d / %d tokens out of range", row, n);
    // (a row the newest check saw running is running: releasing it would leave the count of running rows one too high for good)
    if (e->svc_checked > 0 && !e->svc_fin[row]) return fail(e, SONIC_ERR_INVALID, "sonic_fetch_row: row %d has not finished (sonic_service_step's finished[])", row);
    if (n > 0 && mirror_valid(e, row, false)) memcpy(out_ids, e->svc_out_h + (size_t)row * e->out_cap, (size_t)n * 4);
    else if (n > 0) {
        // no check has shown this occupant finished (a direct user of the C ABI that fetches without stepping): the copy goes behind everything queued on the
        // handle's stream - slow, rare, correct.  Option fetch_stream: the stream of their own the fetches had before the mirror (a finished row's ids are stable)
        hipStream_t st = e->st;
        if (e->opt_fetch_stream) TRY(fetch_stream(e, &st));
        HIPC(e, hipMemcpyAsync(out_ids, e->out_ids + (size_t)row * e->out_cap, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        HIPC(e, st == e->st ? stream_sync(e) : hipStreamSynchronize(st));
    }
    hipLaunchKernelGGL(release_row_kernel, dim3(1), dim3(1), 0, e->st, e->kv_len, e->tok_pos, e->finished, row, req_release_state(e));
    req_row_release(e, row);                                // (a finished row changes no state and reads no automaton that matters: its reference can go)
    HIPC(e, hipGetLastError());
    return SONIC_OK;
}

// sonic_fetch_row for n rows in one call: the D2H copies go out together, one wait, one release launch - what a block of 32 finished rows costs
// the host drops from 32 lock / copy / wait / launch rounds (about a chunk's worth of time, during which the loop's queue could run dry) to one
__global__ void release_rows_kernel(int* kv_len, int* tok_pos, int* finished, SpliceArgs a, int n, int* gram_state) {
    const int i = threadIdx.x;
    if (i < n) { const int row = a.dst[i]; kv_len[row] = 1; tok_pos[row] = 0; finished[row] = 1; if (gram_state) gram_state[row] = -1; }
}
static int fetch_rows_locked(sonic_engine* e, int n, const int32_t* rows, const int32_t* counts, int32_t* out_ids, int out_ld, float* out_lp) {
    const size_t w = (size_t)lp_width(e);
    if (!e->svc_on) return fail(e, SONIC_ERR_INVALID, "sonic_fetch_rows needs sonic_service_begin");
    if (n < 1 || n > 64) return fail(e, SONIC_ERR_INVALID, "sonic_fetch_rows: %d rows", n);
    SpliceArgs a{};
    for (int i = 0; i < n; ++i) {
        const int row = rows[i], c = counts[i];
        if (row < 0 || row >= e->Bm || c < 0 || c > e->out_cap || c > out_ld) return fail(e, SONIC_ERR_INVALID, "sonic_fetch_rows: row %d / %d tokens out of range", row, c);
        if (e->svc_checked > 0 && !e->svc_fin[row]) return fail(e, SONIC_ERR_INVALID, "sonic_fetch_rows: row %d has not finished (sonic_service_step's finished[])", row);
        for (int j = 0; j < i; ++j) if (rows[j] == row) return fail(e, SONIC_ERR_INVALID, "sonic_fetch_rows: row %d named twice", row);
        a.dst[i] = row;
    }
    // a row a check has shown finished since its splice is in the pinned mirror (service_status_kernel): a memcpy.  The others (fetched without stepping, by a direct
    // user of the C ABI) are copied behind everything queued on the handle's stream - or, with option fetch_stream, every row on the old stream of their own
    hipStream_t st = e->st;
    if (e->opt_fetch_stream) TRY(fetch_stream(e, &st));
    bool queued = false;
    for (int i = 0; i < n; ++i) {
        if (counts[i] <= 0) continue;
        const size_t ro = (size_t)rows[i] * e->out_cap;
        if (mirror_valid(e, rows[i], out_lp != nullptr)) {
            memcpy(out_ids + (size_t)i * out_ld, e->svc_out_h + ro, (size_t)counts[i] * 4);
            if (out_lp) memcpy(out_lp + (size_t)i * out_ld * w, e->svc_lp_h + ro * w, (size_t)counts[i] * w * 4);
            continue;
        }
        HIPC(e, hipMemcpyAsync(out_ids + (size_t)i * out_ld, e->out_ids + ro, (size_t)counts[i] * 4, hipMemcpyDeviceToHost, st));
        if (out_lp) HIPC(e, hipMemcpyAsync(out_lp + (size_t)i * out_ld * w, e->out_lp + ro * w, (size_t)counts[i] * w * 4, hipMemcpyDeviceToHost, st));
        queued = true;
    }
    if (queued) HIPC(e, st == e->st ? stream_sync(e) : hipStreamSynchronize(st));
    hipLaunchKernelGGL(release_rows_kernel, dim3(1), dim3(64), 0, e->st, e->kv_len, e->tok_pos, e->finished, a, n, req_release_state(e));
    for (int i = 0; i < n; ++i) req_row_release(e, rows[i]);
    HIPC(e, hipGetLastError());
    return SONIC_OK;
}
extern "C" int sonic_fetch_rows(sonic_engine* e, int n, const int32_t* rows, const int32_t* counts, int32_t* out_ids, int out_ld) {
    if (!e || !rows || !counts || !out_ids) return SONIC_ERR_INVALID;
    ENTER(e);
    return fetch_rows_locked(e, n, rows, counts, out_ids, out_ld, nullptr);
}
// sonic_fetch_rows with the rows' log-probabilities in the same call (the fetch releases the rows): row i's at out_lp + i * out_ld, as its ids; with option
// top_logprobs = K its records of W = 1 + 2K floats at out_lp + i * out_ld * W
extern "C" int sonic_fetch_rows_lp(sonic_engine* e, int n, const int32_t* rows, const int32_t* counts, int32_t* out_ids, int out_ld, float* out_lp) {
    if (!e || !rows || !counts || !out_ids || !out_lp) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(lp_check(e, "sonic_fetch_rows_lp"));
    return fetch_rows_locked(e, n, rows, counts, out_ids, out_ld, out_lp);
}

// ---- asynchronous form: the batch runs on a worker thread of the engine's own; the caller's thread returns at once and may drive other slots.
// One job per engine (slot) at a time; between sonic_run_staged_async and sonic_wait the handle takes no other call except ring appends.
static int run_staged_entry(sonic_engine* e) {
    const sonic_engine::AsyncJob& j = e->a_job;
    ENTER(e);
    const int rc = run_all(e, j.has_rw ? j.req_win.data() : nullptr, j.R, j.prompt_ids.data(), j.prompt_off.data(), j.max_new.data(), j.want_logits != 0);
    req_drop_pending(e);                                    // (a run that failed ahead of its prefill still consumed what was staged for it)
    return rc;
}
static void async_loop(sonic_engine* e) {
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(e->a_mu);
            e->a_cv.wait(lk, [&] { return e->a_pending || e->a_stop; });
            if (!e->a_pending) return;                       // (a pending job still runs before the thread leaves)
            e->a_pending = false; e->a_running = true;
        }
        const int st = run_staged_entry(e);
        {
            std::lock_guard<std::mutex> lk(e->a_mu);
            e->a_status = st; e->a_running = false; e->a_done = true;
        }
        e->a_cv.notify_all();
    }
}
void async_shutdown(sonic_engine* e) {
    {
        std::lock_guard<std::mutex> lk(e->a_mu);
        if (!e->a_started) return;
        e->a_stop = true;
    }
    e->a_cv.notify_all();
    if (e->a_thread.joinable()) e->a_thread.join();
}
extern "C" int sonic_run_staged_async(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                                      const int32_t* max_new, int want_step_logits) {
    if (!e) return SONIC_ERR_INVALID;
    // (a refusal below drops the tables of sonic_set_request_bias: this call was their consumer; an accepted run consumes them in its prefill)
    ReqDrop drop{e};
    if (!prompt_ids || !prompt_off || !max_new || R < 1 || R > 64) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->a_mu);
    if (e->a_stop) return SONIC_ERR_INVALID;
    if (e->a_pending || e->a_running || e->a_done) {         // (e->err belongs to the engine lock; report through the creating thread's slot)
        return fail(nullptr, SONIC_ERR_INVALID, "sonic_run_staged_async: the previous asynchronous run of this handle has not been waited for (sonic_wait)");
    }
    sonic_engine::AsyncJob& j = e->a_job;
    j.R = R; j.want_logits = want_step_logits; j.has_rw = req_win != nullptr;
    j.req_win.assign(req_win ? req_win : nullptr, req_win ? req_win + R + 1 : nullptr);
    j.prompt_off.assign(prompt_off, prompt_off + R + 1);
    if (prompt_off[0] != 0 || prompt_off[R] < prompt_off[0]) return fail(nullptr, SONIC_ERR_INVALID, "sonic_run_staged_async: prompt_off must start at 0 and ascend");
    j.prompt_ids.assign(prompt_ids, prompt_ids + prompt_off[R]);
    j.max_new.assign(max_new, max_new + R);
    if (!e->a_started) { e->a_thread = std::thread(async_loop, e); e->a_started = true; }
    e->a_pending = true; drop.keep = true;
    e->a_cv.notify_all();
    return SONIC_OK;
}
// blocks until the asynchronous run of this handle is complete and returns ITS status (sonic_last_error(e) has the text); SONIC_OK at once when
// nothing is outstanding.  *busy_out (optional, with block == 0): 1 while the run is still going, and the call returns SONIC_OK without waiting.
extern "C" int sonic_wait(sonic_engine* e, int block, int32_t* busy_out) {
    if (!e) return SONIC_ERR_INVALID;
    std::unique_lock<std::mutex> lk(e->a_mu);
    if (busy_out) *busy_out = 0;
    if (!e->a_pending && !e->a_running && !e->a_done) return SONIC_OK;
    if (!block && !e->a_done) { if (busy_out) *busy_out = 1; return SONIC_OK; }
    e->a_cv.wait(lk, [&] { return e->a_done; });
    e->a_done = false;
    return e->a_status;
}

// [B][n_mels][n_frames] fp32 (HF layout) -> frame-major bf16 with one zero row each side
template <typename T> __global__ void feats_to_fm_kernel(const float* in, T* out, int n_mels, int n_frames) {
    const int b = blockIdx.y;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)n_mels * n_frames) return;
    const int t = e / n_mels, m = e % n_mels;
    out[((long)b * (n_frames + 2) + 1 + t) * n_mels + m] = (T)in[((long)b * n_mels + m) * n_frames + t];   // asr.py:280-301: cast to the model dtype
}

extern "C" int sonic_logmel(sonic_engine* e, const int16_t* pcm, const int64_t* offsets, int B, float* feats_out, int32_t* mask_out) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(stage_pcm_locked(e, pcm, offsets, B));
    TRY(run_mel(e, B, feats_out != nullptr));
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    const sonic_dims& d = e->d;
    if (feats_out) HIPC(e, d2h(e, feats_out, e->feats_f32, (size_t)B * d.n_mels * d.n_frames * 4));
    if (mask_out)
        for (int b = 0; b < B; ++b) {
            const int v = frames_of(e->n_samples_h[b]);
            for (int t = 0; t < d.n_frames; ++t) mask_out[(size_t)b * d.n_frames + t] = t < v ? 1 : 0;   // attention_mask[:, ::160]
        }
    return SONIC_OK;
}

extern "C" int sonic_encode(sonic_engine* e, const float* feats, const int32_t* n_valid_frames, int B,
                            float* embeds_out, int32_t* n_audio_out, float* enc_layers_out, float* enc_out) {
    if (!e || !feats || !n_valid_frames) return SONIC_ERR_INVALID;
    ENTER(e);
    if (!e->finalized) return fail(e, SONIC_ERR_INVALID, "weights not finalized");
    if (B < 1 || B > e->Bm) return fail(e, SONIC_ERR_INVALID, "batch out of range");
    const sonic_dims& d = e->d;
    const size_t n = (size_t)B * d.n_mels * d.n_frames;
    if (e->f32) {
        if (!e->feats_f32) HIPC(e, hipMalloc((void**)&e->feats_f32, (size_t)e->Bm * d.n_mels * d.n_frames * 4));
        HIPC(e, h2d(e, e->feats_f32, feats, n * 4));
        TRY(f32_run_encoder(e, B, enc_layers_out, enc_out));
        HIPC(e, stream_sync(e)); HIPC(e, hipGetLastError());
        if (embeds_out) HIPC(e, d2h(e, embeds_out, e->f->pe, (size_t)B * e->Ta * d.dec_d * 4));
        if (n_audio_out) for (int b = 0; b < B; ++b) n_audio_out[b] = keep_rows(d, n_valid_frames[b]);
        return SONIC_OK;
    }
    float* tmp = nullptr;
    HIPC(e, hipMalloc((void**)&tmp, n * 4));
    hipError_t r = h2d(e, tmp, feats, n * 4);
    if (r != hipSuccess) { (void)hipFree(tmp); HIPC(e, r); }
    const long per = (long)d.n_mels * d.n_frames;
    DT_SWITCH(e->dt, T, hipLaunchKernelGGL(feats_to_fm_kernel<T>, dim3((per + 255) / 256, B), dim3(256), 0, e->st, tmp, (T*)e->feats_fm, d.n_mels, d.n_frames));
    if (e->i8) HIPC(e, hipMemcpyAsync(e->win_req, e->seq_iota, (size_t)B * 4, hipMemcpyDeviceToDevice, e->st));   // every window its own request
    int s = run_encoder(e, B, enc_layers_out, enc_out, B);
    hipError_t r2 = stream_sync(e);
    (void)hipFree(tmp);
    TRY(s); HIPC(e, r2); HIPC(e, hipGetLastError());
    if (embeds_out) {
        float* t2 = nullptr;
        const size_t m = (size_t)B * e->Ta * d.dec_d;
        HIPC(e, hipMalloc((void**)&t2, m * 4));
        launch_bf16_to_f32(e->pe, t2, (long)m, e->st, e->dt);
        hipError_t r3 = stream_sync(e);
        if (r3 == hipSuccess) r3 = d2h(e, embeds_out, t2, m * 4);
        (void)hipFree(t2);
        HIPC(e, r3);
    }
    if (n_audio_out) for (int b = 0; b < B; ++b) n_audio_out[b] = keep_rows(d, n_valid_frames[b]);
    return SONIC_OK;
}

// Stage entry points: the two halves of sonic_run_staged.  sonic_prefill = log-mel, encoder, projector, decoder prefill
// and the first greedy token of every request (generate()'s first forward, HF:generation/utils.py:2612-2616); sonic_decode_step = up to
// n_steps further iterations of the greedy loop (:2876-2943); *n_active_out = rows that are neither at EOS nor at their budget,
// *steps_done_out = steps actually run (fewer than asked once the largest budget is reached).  sonic_fetch_tokens reads the result at any point.
extern "C" int sonic_prefill(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                             const int32_t* max_new, int want_step_logits) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER_CONSUME(e);
    if (!prompt_ids || !prompt_off || !max_new) return SONIC_ERR_INVALID;
    if (e->opt_forced_parallel) return fail(e, SONIC_ERR_INVALID, "sonic_prefill: option forced_parallel is on: a scoring handle runs whole batches (sonic_run_staged / sonic_transcribe_*)");
    TRY(run_to_first_token(e, req_win, R, prompt_ids, prompt_off, max_new, want_step_logits != 0));
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    return SONIC_OK;
}
// sonic_prefill without the closing wait: everything up to the first token is QUEUED on the handle's stream when the call returns.  For the
// pipeline form: sonic_splice_rows orders its copies behind this work on the device, so the host need not come back between prefill and splice.
extern "C" int sonic_prefill_enqueue(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER_CONSUME(e);
    if (!prompt_ids || !prompt_off || !max_new) return SONIC_ERR_INVALID;
    if (e->opt_forced_parallel) return fail(e, SONIC_ERR_INVALID, "sonic_prefill_enqueue: option forced_parallel is on: a scoring handle runs whole batches (sonic_run_staged / sonic_transcribe_*)");
    TRY(run_to_first_token(e, req_win, R, prompt_ids, prompt_off, max_new, false));
    HIPC(e, hipGetLastError());
    return SONIC_OK;
}
extern "C" int sonic_decode_step(sonic_engine* e, int n_steps, int32_t* n_active_out, int32_t* steps_done_out) {
    if (!e || n_steps < 0) return SONIC_ERR_INVALID;
    ENTER(e);
    if (e->R < 1 || e->greedy_calls < 1) return fail(e, SONIC_ERR_INVALID, "sonic_decode_step needs a batch that went through sonic_prefill");
    int done = 0;
    TRY(run_decode_steps(e, n_steps, &done));
    HIPC(e, hipMemcpyAsync(e->n_active_h + CHK_RING, e->n_active, 4, hipMemcpyDeviceToHost, e->st));
    HIPC(e, stream_sync(e));
    HIPC(e, hipGetLastError());
    if (n_active_out) *n_active_out = e->n_active_h[CHK_RING];
    if (steps_done_out) *steps_done_out = done;
    return SONIC_OK;
}

int fetch_locked(sonic_engine* e, int32_t* out_ids, int out_ld, int32_t* out_len, float* step_logits, float* out_lp) {
    const int R = e->R;
    if (R < 1) return fail(e, SONIC_ERR_INVALID, "nothing to fetch");
    std::vector<int> nn(64), kvl(64), tps(64), fin(64);
    int act_err[2] = {0, 0};
    HIPC(e, d2h_async(e, act_err, e->n_active, 2 * 4));
    HIPC(e, d2h_async(e, nn.data(), e->n_new, 64 * 4));
    HIPC(e, d2h_async(e, kvl.data(), e->kv_len, 64 * 4));
    HIPC(e, d2h_async(e, tps.data(), e->tok_pos, 64 * 4));
    HIPC(e, d2h_async(e, fin.data(), e->finished, 64 * 4));
    std::vector<int> acc(64, 0);      // option draft_verify: the tokens a drafted request took from its draft (it has run that many greedy launches fewer)
    if (e->draft_last_S > 0 && e->draft_acc) HIPC(e, d2h_async(e, acc.data(), e->draft_acc, 64 * 4));
    HIPC(e, stream_sync(e));
    if (act_err[1] != 0) return fail(e, SONIC_ERR_HIP, "a decode kernel gave up on an in-kernel wait (device error word %d): the batch's tokens are invalid", act_err[1]);
    // invariants of the greedy controller: a running row's context grows by one per launch; a finished row stopped growing with the
    // launch that finished it (kv_len = prompt + tokens - 1), so no row ever leaves its [max_ctx] cache region
    for (int r = 0; r < R && r < (int)e->last_qlen.size(); ++r) {
        const int want_kv = e->last_qlen[r] + nn[r] - (fin[r] ? 1 : 0);
        const int calls = e->greedy_calls + acc[r];
        const int want_new = calls < e->last_maxnew[r] ? calls : e->last_maxnew[r];
        const bool pos_ok = nn[r] >= 1 && kvl[r] == want_kv && kvl[r] <= e->max_ctx && (tps[r] == kvl[r] - 1 || (fin[r] && nn[r] == 1 + acc[r]));
        if (!pos_ok || nn[r] > e->last_maxnew[r] || (!fin[r] && nn[r] != calls) || (e->d.n_eos == 0 && nn[r] != want_new))
            return fail(e, SONIC_ERR_HIP, "decoder state check failed for request %d: kv_len %d (expected %d), tok_pos %d, n_new %d, finished %d (budget %d, greedy launches %d)",
                        r, kvl[r], want_kv, tps[r], nn[r], fin[r], e->last_maxnew[r], e->greedy_calls);
    }
    for (int r = 0; r < R; ++r) {
        if (out_len) out_len[r] = nn[r];
        if (out_ids) {
            if (nn[r] > out_ld) return fail(e, SONIC_ERR_INVALID, "out_ld too small");
            HIPC(e, d2h_async(e, out_ids + (size_t)r * out_ld, e->out_ids + (size_t)r * e->out_cap, (size_t)nn[r] * 4));
        }
        if (out_lp) {
            const size_t w = (size_t)lp_width(e);            // out_ld counts floats: a token's record holds w of them (option top_logprobs)
            if (e->align_last && e->align_t) {      // an align run's batch: t_n rides behind the record's 1 + 2K floats, which keep their bits
                if ((size_t)nn[r] * (w + 1) > (size_t)out_ld) return fail(e, SONIC_ERR_INVALID, "out_ld too small (an align run's records hold %zu floats)", w + 1);
                std::vector<float> rec((size_t)nn[r] * w), tn((size_t)nn[r]);
                HIPC(e, d2h_async(e, rec.data(), e->out_lp + (size_t)r * e->out_cap * w, rec.size() * 4));
                HIPC(e, d2h_async(e, tn.data(), e->align_t + (size_t)r * e->out_cap, tn.size() * 4));
                HIPC(e, stream_sync(e));
                float* o = out_lp + (size_t)r * out_ld;
                for (int n = 0; n < nn[r]; ++n) { memcpy(o + (size_t)n * (w + 1), rec.data() + (size_t)n * w, w * 4); o[(size_t)n * (w + 1) + w] = tn[n]; }
                continue;
            }
            if ((size_t)nn[r] * w > (size_t)out_ld) return fail(e, SONIC_ERR_INVALID, "out_ld too small");
            HIPC(e, d2h_async(e, out_lp + (size_t)r * out_ld, e->out_lp + (size_t)r * e->out_cap * w, (size_t)nn[r] * w * 4));
        }
    }
    if (!e->svc_on) req_batch_fetched(e, fin.data(), R);      // a batch whose every row has ended lets go of what its rows held
    if (step_logits) {
        if (!e->dump_steps) return fail(e, SONIC_ERR_INVALID, "step logits were not requested for the last run");
        HIPC(e, d2h_async(e, step_logits, e->dump, (size_t)e->dump_steps * R * e->d.vocab * 4));
    }
    HIPC(e, stream_sync(e));
    return SONIC_OK;
}

extern "C" int sonic_fetch_tokens(sonic_engine* e, int32_t* out_ids, int out_ld, int32_t* out_len, float* step_logits) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    return fetch_locked(e, out_ids, out_ld, out_len, step_logits);
}

// the log-probabilities of the tokens sonic_fetch_tokens returns (same rows, same counts: row r's n_new[r] values at out_lp + r * out_ld; entries
// beyond are not written); valid whenever that call is.  With option top_logprobs = K: n_new[r] records of 1 + 2K floats, out_ld counting floats
extern "C" int sonic_fetch_logprobs(sonic_engine* e, float* out_lp, int out_ld) {
    if (!e || !out_lp) return SONIC_ERR_INVALID;
    ENTER(e);
    TRY(lp_check(e, "sonic_fetch_logprobs"));
    return fetch_locked(e, nullptr, out_ld, nullptr, nullptr, out_lp);
}

extern "C" int sonic_transcribe_batch(sonic_engine* e, const int16_t* pcm, const int64_t* offsets, int W, const int32_t* req_win, int R,
                                      const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new,
                                      int32_t* out_ids, int out_ld, int32_t* out_len, float* step_logits) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER_CONSUME(e);
    if (!prompt_ids || !prompt_off || !max_new) return SONIC_ERR_INVALID;
    TRY(stage_pcm_locked(e, pcm, offsets, W));
    TRY(run_all(e, req_win, R, prompt_ids, prompt_off, max_new, step_logits != nullptr));
    return fetch_locked(e, out_ids, out_ld, out_len, step_logits);
}

// Teacher forcing for parity tests (oracle_outputs.force_ids, sonic_oracle.c): while set, every run feeds ids[r][n] as token n of
// request r instead of the argmax (logits are still computed and dumped; EOS / budget rules apply to the forced token).  NULL clears.
extern "C" int sonic_set_forced_ids(sonic_engine* e, const int32_t* ids, int R, int ld) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    HIPC(e, stream_sync(e));
    if (e->force_d) { (void)hipFree(e->force_d); e->force_d = nullptr; e->force_ld = e->force_R = 0; }
    e->force_h.clear();
    if (!ids) return SONIC_OK;
    if (R < 1 || R > e->Bm || ld < 1) return fail(e, SONIC_ERR_INVALID, "forced ids: bad shape [%d][%d]", R, ld);
    for (long i = 0; i < (long)R * ld; ++i)
        if (ids[i] < 0 || ids[i] >= e->d.vocab) return fail(e, SONIC_ERR_INVALID, "forced id %d out of vocabulary", ids[i]);
    HIPC(e, hipMalloc((void**)&e->force_d, (size_t)R * ld * 4));
    HIPC(e, h2d(e, e->force_d, ids, (size_t)R * ld * 4));
    e->force_R = R; e->force_ld = ld; e->force_h.assign(ids, ids + (size_t)R * ld);
    return SONIC_OK;
}

extern "C" int sonic_get_timings(sonic_engine* e, sonic_timings* out) {
    if (!e || !out) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    *out = e->tim;
    return SONIC_OK;
}
