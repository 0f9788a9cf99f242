// sonic_hip engine: what a handle generates with - the log-probability buffer and its width (options token_logprobs / top_logprobs), the generation guards
// (sonic_set_generation), and the three per-request stages: request bias, sampling, grammar (ReqStage, engine_internal.h) with their setters, packers and uploads and
// the grammar registry.  The last section, "the stages at every point of a request's life", is the ONE place that lists the stages: a prefill's claim and upload, the
// greedy launch, the graph key, the splice, a row's release, a slot's inheritance, the destroy.  A fourth per-request value is added there and nowhere else.
#include "engine_internal.h"

// option token_logprobs: the log-probability buffer beside out_ids, allocated by the first handle state that needs it (counted by sonic_memory_info)
int lp_alloc(sonic_engine* e) {
    if (e->out_lp) return SONIC_OK;
    HIPC(e, hipSetDevice(e->device));
    TRY(dalloc(e, &e->out_lp, (size_t)64 * e->out_cap * lp_width(e)));
    HIPC(e, stream_sync(e));
    return SONIC_OK;
}
// option top_logprobs = K: the K best alternatives of every step ride in the token's log-probability record, which grows to 1 + 2K floats.  The
// buffer is exchanged for one of the new width (sonic_memory_info follows), so the records of a finished batch that has not been fetched yet are gone with the
// old one: fetch first (include/sonic_hip.h says so).  The caller holds the lock and has asked gen_busy.
int top_enable(sonic_engine* e, int K) {
    if (K < 0 || K > 8) return fail(e, SONIC_ERR_INVALID, "top_logprobs: %d is outside 0 .. 8", K);
    if (K > 0 && !lp_on(e)) return fail(e, SONIC_ERR_INVALID, "top_logprobs: option token_logprobs must be on first (the alternatives share the log-probability kernels' sum; sonic_set_option(e, \"token_logprobs\", 1))");
    if (K == e->opt_top_logprobs) return SONIC_OK;
    HIPC(e, hipSetDevice(e->device));
    HIPC(e, stream_sync(e));
    const bool had = e->out_lp != nullptr;
    if (had) TRY(dfree(e, &e->out_lp, (size_t)64 * e->out_cap * lp_width(e)));
    e->opt_top_logprobs = K;
    drop_graphs(e);                                      // the greedy kernel and its arguments are part of every captured chunk
    return had ? lp_alloc(e) : SONIC_OK;
}
int lp_check(sonic_engine* e, const char* who) {
    if (lp_on(e)) return SONIC_OK;
    return fail(e, SONIC_ERR_INVALID, "%s: option token_logprobs is off on this handle (sonic_set_option(e, \"token_logprobs\", 1) on the owner before its slots are created)", who);
}
// dispatch.cpp / pipeline.cpp (same library, not exported): does this handle produce log-probabilities
extern "C" int engine_token_logprobs_on(sonic_engine* e) { return e && lp_on(e) ? 1 : 0; }
// ... and how many alternatives ride along (option top_logprobs: its log-probability records hold 1 + 2K floats per token)
extern "C" int engine_top_logprobs(sonic_engine* e) { return e && lp_on(e) ? e->opt_top_logprobs : 0; }
extern "C" int engine_forced_parallel_on(sonic_engine* e) { return e && e->opt_forced_parallel ? 1 : 0; }      // ... and is it a scoring handle (option forced_parallel: the schedulers refuse it)
extern "C" int engine_fail(sonic_engine* e, int code, const char* msg) { std::lock_guard<std::mutex> lk(e->mu); return fail(e, code, "%s", msg); }   // a message on a handle, from outside its calls

// ---- generation guards: validation, the history / suppress buffers on first use, the upload.  The caller holds the lock and has made sure nothing is in flight.
#define GEN_MAX_SUPPRESS 256
int gen_apply(sonic_engine* e, float penalty, int ngram, const int32_t* suppress, int n_suppress) {
    if (!(penalty > 0.f) || !std::isfinite(penalty)) return fail(e, SONIC_ERR_INVALID, "sonic_set_generation: repetition_penalty must be a finite value > 0 (got %g)", (double)penalty);
    if (ngram < 0 || ngram > 64) return fail(e, SONIC_ERR_INVALID, "sonic_set_generation: no_repeat_ngram_size %d is outside 0 .. 64", ngram);
    if (n_suppress < 0 || n_suppress > GEN_MAX_SUPPRESS || (n_suppress > 0 && !suppress))
        return fail(e, SONIC_ERR_INVALID, "sonic_set_generation: suppress_tokens holds %d ids (at most %d)", n_suppress, GEN_MAX_SUPPRESS);
    for (int i = 0; i < n_suppress; ++i)
        if (suppress[i] < 0 || suppress[i] >= e->d.vocab) return fail(e, SONIC_ERR_INVALID, "sonic_set_generation: suppressed token id %d out of vocabulary (%d)", suppress[i], e->d.vocab);
    const bool on = penalty != 1.0f || ngram > 0 || n_suppress > 0;
    if (on && greedy_guard_lds(e->d.vocab) > 60000) return fail(e, SONIC_ERR_UNSUPPORTED, "sonic_set_generation: a vocabulary of %d ids does not fit the guard bitmaps", e->d.vocab);
    HIPC(e, hipSetDevice(e->device));
    HIPC(e, stream_sync(e));
    if (on && !e->hist) { TRY(dalloc(e, &e->hist, (size_t)64 * e->max_ctx)); HIPC(e, stream_sync(e)); }          // (option request_bias may have brought the history already)
    if (on && !e->gen_suppress_d) { TRY(dalloc(e, &e->gen_suppress_d, (size_t)GEN_MAX_SUPPRESS)); HIPC(e, stream_sync(e)); }
    if (n_suppress > 0) HIPC(e, h2d(e, e->gen_suppress_d, suppress, (size_t)n_suppress * 4));
    e->gen_penalty = penalty; e->gen_ngram = ngram; e->gen_suppress.assign(suppress, suppress + n_suppress); e->gen_on = on;
    drop_graphs(e);                                      // the greedy kernel and its arguments are part of every captured chunk
    return SONIC_OK;
}
// Both ways in (sonic_set_generation, the gen_* keys of sonic_set_option) ask this first, under the handle's lock: SONIC_ERR_INVALID while the handle has work in
// hand.  A prefilled batch counts until its decode loop has ended or every one of its rows has been handed to a continuous loop (sonic_splice_rows): a prefill
// slot whose rows were all spliced away is free again.  (No path takes e->mu while it holds a_mu, so the short a_mu section below cannot deadlock.)
int gen_busy(sonic_engine* e, const char* who) {
    { std::lock_guard<std::mutex> lk(e->a_mu); if (e->a_pending || e->a_running) return fail(e, SONIC_ERR_INVALID, "%s: an asynchronous run of this handle is in flight", who); }
    if (e->svc_on) return fail(e, SONIC_ERR_INVALID, "%s: this handle is decoding continuously (sonic_service_end first)", who);
    if (e->R >= 1 && e->greedy_calls >= 1 && e->steps_run + 1 < e->max_steps) {
        const uint64_t all = e->R >= 64 ? ~0ull : (1ull << e->R) - 1;
        if ((e->spliced & all) != all)
            return fail(e, SONIC_ERR_INVALID, "%s: the handle holds a prefilled batch of %d requests whose rows are still running (its decode loop has not ended and they were not all handed to a continuous loop)", who, e->R);
    }
    return SONIC_OK;
}
// ---- values left for the requests of the next prefill (ReqStage, engine_internal.h): what the options request_bias and sampling share.  A setter fills the pinned
// mirror and leaves pending = R; the next prefill claims it (run_to_first_token), uploads it on the stream and marks the mirror busy until those copies are done; every
// other way out of a consuming entry point drops it (ReqDrop).  The caller holds the lock.
// The option's switch (the caller has asked gen_busy): on first use the zero-filled device words - every row starts neutral; `hist`: the rows' input_ids too - the
// pinned mirror and the event.  `opt` names the option in the message
template <typename W> static int stage_enable(sonic_engine* e, ReqStage<W>& s, int on, int* flag, const char* opt, int words, bool hist) {
    HIPC(e, hipSetDevice(e->device));
    HIPC(e, stream_sync(e));
    if (on) {
        if (hist && !e->hist) TRY(dalloc(e, &e->hist, (size_t)64 * e->max_ctx));
        if (!s.dev) TRY(dalloc(e, &s.dev, (size_t)words));
        if (!s.host && hipHostMalloc((void**)&s.host, (size_t)words * sizeof(W), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(e, SONIC_ERR_OOM, "%s: pinned host memory exhausted", opt); }
        if (!s.ev) HIPC(e, hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
        HIPC(e, stream_sync(e));
    }
    *flag = on ? 1 : 0; s.pending = -1; s.take = false;
    drop_graphs(e);                                      // the greedy kernel and its arguments are part of every captured chunk
    return SONIC_OK;
}
// open the mirror for writing (the previous batch's copies out of it are awaited first); the upload's copies are on the stream; the destroy path
template <typename W> static int stage_open(sonic_engine* e, ReqStage<W>& s) { if (s.busy) { HIPC(e, hipEventSynchronize(s.ev)); s.busy = false; } return SONIC_OK; }
template <typename W> static int stage_sent(sonic_engine* e, ReqStage<W>& s) { HIPC(e, hipEventRecord(s.ev, e->st)); s.busy = true; s.take = false; return SONIC_OK; }
template <typename W> static void stage_free(ReqStage<W>& s) { if (s.host) (void)hipHostFree(s.host); if (s.ev) (void)hipEventDestroy(s.ev); }
static int stage_count(sonic_engine* e, int got, int R, const char* setter, const char* what, bool forked = false) {
    if (got < 0 || got == R) return SONIC_OK;
    if (forked) return fail(e, SONIC_ERR_INVALID, "request_forks: %s gave %s for %d rows, the forked batch has %d (per-request values are stated per row, in row order)", setter, what, got, R);
    return fail(e, SONIC_ERR_INVALID, "%s gave %s for %d requests, the batch has %d", setter, what, got, R);
}
// What both setters open with: refused during an asynchronous run (without waiting for the engine lock that run holds), then the lock (`lk`), then refused while
// the option `opt` (flag `on`) is off.  From here on nothing is pending
template <typename W> static int stage_enter(sonic_engine* e, std::unique_lock<std::mutex>& lk, const char* who, const char* opt, const int& on, ReqStage<W>& s) {
    { std::lock_guard<std::mutex> ak(e->a_mu); if (e->a_pending || e->a_running) return fail(nullptr, SONIC_ERR_INVALID, "%s: an asynchronous run of this handle is in flight", who); }
    lk = std::unique_lock<std::mutex>(e->mu);
    (void)hipGetLastError();
    if (!on || !s.dev) return fail(e, SONIC_ERR_INVALID, "%s: option %s is off on this handle (sonic_set_option(e, \"%s\", 1) on the owner before its slots are created)", who, opt, opt);
    s.pending = -1;
    return SONIC_OK;
}
// ---- option request_bias: HF's SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor (generation/logits_process.py) with one table per request -
// the reference's hotwords (backend/asr.py:303-333) as a bias on the scores instead of a sentence in the prompt.  The caller holds the lock and has asked gen_busy.
int bias_enable(sonic_engine* e, int on) {
    if (on && greedy_guard_lds(e->d.vocab, true) > 60000) return fail(e, SONIC_ERR_UNSUPPORTED, "request_bias: a vocabulary of %d ids does not fit the bias bitmaps", e->d.vocab);
    return stage_enable(e, e->bias, on, &e->opt_request_bias, "request_bias", BIAS_TAB_WORDS, true);      // (zero-filled: every row starts without a table)
}
int bias_pack(sonic_engine* e, const char* who, const int32_t* seq_ids, const int32_t* seq_off, const float* bias, int n, int V, int* row, int* count) {
    if (n < 0 || n > BIAS_MAX_ENTRIES) return fail(e, SONIC_ERR_INVALID, "%s: a request's table holds %d entries (at most %d; nothing is truncated)", who, n, BIAS_MAX_ENTRIES);
    if (n > 0 && (!seq_ids || !seq_off || !bias)) return fail(e, SONIC_ERR_INVALID, "%s: null table", who);
    struct Ent { const int32_t* ids; int L; float b; };
    std::vector<Ent> v;
    for (int i = 0; i < n; ++i) {
        const int L = seq_off[i + 1] - seq_off[i];
        if (L < 1 || L > BIAS_MAX_LEN) return fail(e, SONIC_ERR_INVALID, "%s: entry %d has %d ids (1 .. %d)", who, i, L, BIAS_MAX_LEN);
        const int32_t* ids = seq_ids + seq_off[i];
        for (int k = 0; k < L; ++k) if (ids[k] < 0 || ids[k] >= V) return fail(e, SONIC_ERR_INVALID, "%s: token id %d out of vocabulary (%d)", who, ids[k], V);
        if (std::isnan(bias[i]) || bias[i] == INFINITY) return fail(e, SONIC_ERR_INVALID, "%s: entry %d has bias %g (finite values, or -inf for a bad word)", who, i, (double)bias[i]);
        bool dup = false;                                // HF's list -> dict conversion: the last bias of equal sequences wins, at the first one's position
        for (Ent& o : v) if (o.L == L && !memcmp(o.ids, ids, (size_t)L * 4)) { o.b = bias[i]; dup = true; break; }
        if (!dup) v.push_back(Ent{ids, L, bias[i]});
    }
    // grouped by last id; inside a group the length-1 entry first (HF starts from length_1_bias), then list order: the order the kernel's one thread adds in
    std::stable_sort(v.begin(), v.end(), [](const Ent& a, const Ent& b) {
        const int la = a.ids[a.L - 1], lb = b.ids[b.L - 1];
        if (la != lb) return la < lb;
        return (a.L == 1) > (b.L == 1);
    });
    for (size_t i = 0; i < v.size(); ++i) {
        int* w = row + i * BIAS_ENTRY_WORDS;
        w[0] = v[i].ids[v[i].L - 1]; w[1] = v[i].L; memcpy(&w[2], &v[i].b, 4);
        for (int k = 0; k < BIAS_MAX_LEN - 1; ++k) w[3 + k] = k < v[i].L - 1 ? v[i].ids[k] : -1;
    }
    *count = (int)v.size();
    return SONIC_OK;
}
// The tables of the R requests of the next prefill on this handle (sonic_prefill / sonic_prefill_enqueue / sonic_run_staged[_async] / sonic_transcribe_*), which
// consumes them: a later batch starts without tables.  Request r's entries are seq_off[req_off[r]] .. seq_off[req_off[r + 1]] of seq_ids, with bias[req_off[r] ..].
extern "C" int sonic_set_request_bias(sonic_engine* e, const int32_t* seq_ids, const int32_t* seq_off, const float* bias, const int32_t* req_off, int R) {
    if (!e) return SONIC_ERR_INVALID;
    std::unique_lock<std::mutex> lk; TRY(stage_enter(e, lk, "sonic_set_request_bias", "request_bias", e->opt_request_bias, e->bias));
    if (R < 1 || R > e->Bm || R > 64 || !req_off || req_off[0] != 0) return fail(e, SONIC_ERR_INVALID, "sonic_set_request_bias: %d requests (1 .. %d), offsets from 0", R, e->Bm);
    HIPC(e, hipSetDevice(e->device));
    TRY(stage_open(e, e->bias));
    for (int r = 0; r < 64; ++r) e->bias.host[r] = 0;
    for (int r = 0; r < R; ++r) {
        const int a = req_off[r], n = req_off[r + 1] - req_off[r];
        if (n < 0) return fail(e, SONIC_ERR_INVALID, "sonic_set_request_bias: request offsets decrease");
        if (n == 0) continue;
        if (!seq_off || !bias) return fail(e, SONIC_ERR_INVALID, "sonic_set_request_bias: null table");
        TRY(bias_pack(e, "sonic_set_request_bias", seq_ids, seq_off + a, bias + a, n, e->d.vocab, e->bias.host + 64 + (size_t)r * BIAS_ROW_WORDS, &e->bias.host[r]));
    }
    e->bias.pending = R;
    return SONIC_OK;
}
static int bias_upload(sonic_engine* e, int R) {
    if (!e->opt_request_bias) return SONIC_OK;
    if (!e->bias.take && e->opt_bias_fill > 0) {
        // option request_bias_fill = n (drivers that only pass integers: bench.py --opt; tools/ab_request_bias.sh): every request of a batch without tables gets n
        // length-1 entries of bias +0.0 on ids spread over the vocabulary.  s + 0.0 changes no token, but the kernel does all its work for them: the prologue's
        // flags and group sums, n bits in the "biased" map, the list scan at every one of those ids
        TRY(stage_open(e, e->bias));
        const int n = e->opt_bias_fill, V = e->d.vocab;
        for (int r = 0; r < 64; ++r) e->bias.host[r] = r < R ? n : 0;
        for (int r = 0; r < R; ++r)
            for (int k = 0; k < n; ++k) {
                int* w = e->bias.host + 64 + (size_t)r * BIAS_ROW_WORDS + (size_t)k * BIAS_ENTRY_WORDS;
                w[0] = (int)((long)k * V / n); w[1] = 1; w[2] = 0;
                for (int j = 3; j < BIAS_ENTRY_WORDS; ++j) w[j] = -1;
            }
        e->bias.take = true;
    }
    if (!e->bias.take) { launch_fill_i32(e->bias.dev, 0, 64, e->st); return SONIC_OK; }             // a batch without tables: every count 0
    HIPC(e, hipMemcpyAsync(e->bias.dev, e->bias.host, 64 * 4, hipMemcpyHostToDevice, e->st));
    for (int r = 0; r < R; ++r) {
        const size_t o = 64 + (size_t)r * BIAS_ROW_WORDS;
        if (e->bias.host[r] > 0) HIPC(e, hipMemcpyAsync(e->bias.dev + o, e->bias.host + o, (size_t)e->bias.host[r] * BIAS_ENTRY_WORDS * 4, hipMemcpyHostToDevice, e->st));
    }
    return stage_sent(e, e->bias);
}
// ---- option sampling: temperature sampling in the greedy kernel by the Gumbel-max identity, one (temperature, seed) per request - what Whisper's
// decode_with_fallback retries with.  The caller holds the lock and has asked gen_busy.
int samp_enable(sonic_engine* e, int on) {
    if (!on && e->opt_truncation) return fail(e, SONIC_ERR_INVALID, "sampling cannot be switched off while option truncation is on (the filters cut what a sampling row draws from)");
    if (on && !lp_on(e)) return fail(e, SONIC_ERR_INVALID, "sampling: option token_logprobs must be on first (the sampling kernels are log-probability kernels; sonic_set_option(e, \"token_logprobs\", 1))");
    return stage_enable(e, e->samp, on, &e->opt_sampling, "sampling", SAMP_WORDS, false);                  // (zero-filled: every row starts greedy)
}
void samp_pack(unsigned* w, float t, uint64_t seed) { memcpy(&w[0], &t, 4); w[1] = (unsigned)(seed & 0xffffffffull); w[2] = (unsigned)(seed >> 32); }
int samp_check(sonic_engine* e, const char* who, const float* temperature, int n) {
    for (int r = 0; r < n; ++r) {
        const float t = temperature[r];
        if (!(t == 0.f || (t >= 1e-3f && t <= 100.f)))     // (NaN fails every compare)
            return fail(e, SONIC_ERR_INVALID, "%s: temperature %g of request %d is invalid (0 = greedy, or 1e-3 .. 100; nothing is clamped)", who, (double)t, r);
    }
    return SONIC_OK;
}
// The (temperature, seed) of the R requests of the next prefill on this handle (the entry points of sonic_set_request_bias), which consumes them: a later batch
// starts greedy.
extern "C" int sonic_set_request_sampling(sonic_engine* e, const float* temperature, const uint64_t* seed, int R) {
    if (!e) return SONIC_ERR_INVALID;
    std::unique_lock<std::mutex> lk; TRY(stage_enter(e, lk, "sonic_set_request_sampling", "sampling", e->opt_sampling, e->samp));
    if (R < 1 || R > e->Bm || R > 64 || !temperature || !seed) return fail(e, SONIC_ERR_INVALID, "sonic_set_request_sampling: %d requests (1 .. %d), values for each", R, e->Bm);
    TRY(samp_check(e, "sonic_set_request_sampling", temperature, R));
    HIPC(e, hipSetDevice(e->device));
    TRY(stage_open(e, e->samp));
    for (int i = 0; i < SAMP_WORDS; ++i) e->samp.host[i] = 0u;
    for (int r = 0; r < R; ++r) samp_pack(e->samp.host + 3 * r, temperature[r], seed[r]);
    e->samp.pending = R;
    return SONIC_OK;
}
static int samp_upload(sonic_engine* e, int R) {
    if (!e->opt_sampling) return SONIC_OK;
    if (!e->samp.take && e->opt_samp_fill_milli > 0) {
        // option sampling_fill_milli = m (drivers that only pass integers: bench.py --opt; tools/ab_sampling.sh): request r of a batch without values gets temperature
        // m / 1000 and seed r.  A batch is then the same draw every time it runs, on whichever handle: a benchmark can still check its tokens
        TRY(stage_open(e, e->samp));
        const float t = (float)((double)e->opt_samp_fill_milli / 1000.0);
        for (int i = 0; i < SAMP_WORDS; ++i) e->samp.host[i] = 0u;
        for (int r = 0; r < R && r < 64; ++r) samp_pack(e->samp.host + 3 * r, t, (uint64_t)r);
        e->samp.take = true;
    }
    if (!e->samp.take) { launch_fill_i32((int*)e->samp.dev, 0, SAMP_WORDS, e->st); return SONIC_OK; } // a batch without values: every row greedy
    HIPC(e, hipMemcpyAsync(e->samp.dev, e->samp.host, (size_t)SAMP_WORDS * 4, hipMemcpyHostToDevice, e->st));
    return stage_sent(e, e->samp);
}
// ---- option truncation: top_k / top_p / min_p on the temperature-scaled scores of a sampling row - HF's TopK / TopP / MinP warpers - with the cut
// found inside the greedy kernel (truncsel.h).  The caller holds the lock and has asked gen_busy.
int trunc_enable(sonic_engine* e, int on) {
    if (on && !(e->opt_sampling && e->samp.dev)) return fail(e, SONIC_ERR_INVALID, "truncation: option sampling must be on first (the filters cut what a sampling row draws from; sonic_set_option(e, \"sampling\", 1))");
    if (on && greedy_guard_lds(e->d.vocab, true) + greedy_trunc_lds() > 60000) return fail(e, SONIC_ERR_UNSUPPORTED, "truncation: a vocabulary of %d ids does not fit the select's histogram beside the guard and bias bitmaps", e->d.vocab);
    return stage_enable(e, e->trunc, on, &e->opt_truncation, "truncation", TRUNC_STAGE_WORDS, false);      // (zero-filled: every row starts with the three filters off)
}
int trunc_pack(sonic_engine* e, const char* who, const float* v, int row, unsigned* w) {
    const float k = v[0], p = v[1], m = v[2];
    if (!(k >= 0.f && k <= 16777216.f) || k != floorf(k)) return fail(e, SONIC_ERR_INVALID, "%s: top_k %g of row %d is invalid (an integer in 0 .. 2^24, 0 = off; nothing is clamped)", who, (double)k, row);
    if (!(p > 0.f && p <= 1.f)) return fail(e, SONIC_ERR_INVALID, "%s: top_p %g of row %d is invalid (a value in (0, 1], 1 = off; nothing is clamped)", who, (double)p, row);
    if (!(m >= 0.f && m <= 1.f)) return fail(e, SONIC_ERR_INVALID, "%s: min_p %g of row %d is invalid (a value in [0, 1], 0 = off; nothing is clamped)", who, (double)m, row);
    w[0] = (unsigned)k;
    w[1] = 0u; if (p < 1.f) memcpy(&w[1], &p, 4);
    w[2] = 0u; if (m > 0.f) { const float lnm = m < 1.f ? (float)log((double)m) : -0.f; memcpy(&w[2], &lnm, 4); }      // (ln 1 travels as -0.0: y_max + -0.0 = y_max, and the word is not the "off" word)
    return SONIC_OK;
}
static int trunc_rows_check(const char* who, int dtype, const int64_t* shape, int ndim, int max_rows, sonic_engine* e) {
    if (dtype != SONIC_DTYPE_F32 || ndim != 2 || shape[0] < 1 || shape[1] != 3) return fail(e, SONIC_ERR_INVALID, "%s: the values are float32 rows [top_k | top_p | min_p], one per row of the batch (SONIC_DTYPE_F32, shape {R, 3})", who);
    if (shape[0] > max_rows || shape[0] > 64) return fail(e, SONIC_ERR_INVALID, "%s: %lld rows (1 .. %d)", who, (long long)shape[0], max_rows < 64 ? max_rows : 64);
    return SONIC_OK;
}
// sonic_load_tensor(e, "request_truncation", values, SONIC_DTYPE_F32, {R, 3}, 2): (top_k, top_p, min_p) of the R rows of the next prefill on this handle (the entry
// points of sonic_set_request_bias), which consumes them: a later batch starts with the filters off.  Stated per row under forks, as every per-request value
int trunc_stage_rows(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim) {
    std::unique_lock<std::mutex> lk; TRY(stage_enter(e, lk, "request_truncation", "truncation", e->opt_truncation, e->trunc));
    TRY(trunc_rows_check("request_truncation", dtype, shape, ndim, e->Bm, e));
    unsigned w[TRUNC_STAGE_WORDS] = {0u};
    for (int r = 0; r < (int)shape[0]; ++r) TRY(trunc_pack(e, "request_truncation", (const float*)data + 3 * r, r, w + 3 * r));
    HIPC(e, hipSetDevice(e->device));
    TRY(stage_open(e, e->trunc));
    memcpy(e->trunc.host, w, sizeof w);
    e->trunc.pending = (int)shape[0];
    return SONIC_OK;
}
int trunc_hook_arm(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim) {
    TRY(trunc_rows_check("truncation.hook", dtype, shape, ndim, 64, nullptr));
    std::vector<unsigned> w((size_t)TRUNC_STAGE_WORDS, 0u);
    for (int r = 0; r < (int)shape[0]; ++r) TRY(trunc_pack(nullptr, "truncation.hook", (const float*)data + 3 * r, r, w.data() + 3 * r));
    std::lock_guard<std::mutex> lk(e->mu);
    e->hook_trunc.swap(w);
    return SONIC_OK;
}
static int trunc_upload(sonic_engine* e, int R) {
    if (!e->opt_truncation) return SONIC_OK;
    if (!e->trunc.take && e->opt_trunc_fill) {
        // option truncation_fill (drivers that only pass integers: bench.py --opt; tools/ab_truncation.sh): every request of a batch without values gets top_k = 50, top_p = 0.9
        TRY(stage_open(e, e->trunc));
        const float v[3] = {50.f, 0.9f, 0.f};
        for (int i = 0; i < TRUNC_STAGE_WORDS; ++i) e->trunc.host[i] = 0u;
        for (int r = 0; r < R && r < 64; ++r) TRY(trunc_pack(e, "truncation_fill", v, r, e->trunc.host + 3 * r));
        e->trunc.take = true;
    }
    if (!e->trunc.take) { launch_fill_i32((int*)e->trunc.dev, 0, TRUNC_STAGE_WORDS, e->st); return SONIC_OK; } // a batch without values: every filter off
    HIPC(e, hipMemcpyAsync(e->trunc.dev, e->trunc.host, (size_t)TRUNC_STAGE_WORDS * 4, hipMemcpyHostToDevice, e->st));
    return stage_sent(e, e->trunc);
}
// dispatch.cpp (same library, not exported): one request's (top_k, top_p, min_p) checked at its submit, the message to the calling thread's sonic_last_error(NULL)
extern "C" int engine_truncation_validate(const float* row) { unsigned w[3]; return trunc_pack(nullptr, "truncation", row, 0, w); }
extern "C" int engine_truncation_on(sonic_engine* e) { return e && e->opt_truncation && e->trunc.dev ? 1 : 0; }
extern "C" int engine_sampling_on(sonic_engine* e) { return e && e->opt_sampling && e->samp.dev ? 1 : 0; }
// ---- option grammar: a request's transcript restricted to the paths of a deterministic token automaton - HF's prefix_allowed_tokens_fn
// (PrefixConstrainedLogitsProcessor), Vosk's `grammar` - with the mask and the state transition inside the greedy kernel.  Grammars live on the weight owner.
// the automaton's arrays validated by the contract's rules (SONIC_ERR_INVALID, the message - on e, or the calling thread's for e = NULL - names `who` and the cause) and
// packed into the device blob's words: GRAM_HEAD + N + 1 + 2E of them
static int gram_pack(sonic_engine* e, const char* who, const int32_t* node_off, const int32_t* edge_tok, const int32_t* edge_next, int N, int E, int vocab, int audio_id, std::vector<int>* out) {
    if (!node_off || !edge_tok || !edge_next) return fail(e, SONIC_ERR_INVALID, "%s: null array", who);
    if (N < 1 || N > GRAM_MAX_NODES) return fail(e, SONIC_ERR_INVALID, "%s: %d nodes (1 .. %d; nothing is truncated)", who, N, GRAM_MAX_NODES);
    if (E < 1 || E > GRAM_MAX_EDGES) return fail(e, SONIC_ERR_INVALID, "%s: %d edges (1 .. %d; nothing is truncated)", who, E, GRAM_MAX_EDGES);
    if (node_off[0] != 0) return fail(e, SONIC_ERR_INVALID, "%s: node_off[0] is %d, not 0", who, node_off[0]);
    if (node_off[N] != E) return fail(e, SONIC_ERR_INVALID, "%s: node_off[%d] is %d, not the edge count %d", who, N, node_off[N], E);
    for (int n = 0; n < N; ++n) {
        const int a = node_off[n], b = node_off[n + 1];
        if (b < a || a < 0 || b > E) return fail(e, SONIC_ERR_INVALID, "%s: node_off is not monotone at node %d (%d then %d)", who, n, a, b);
        if (b == a) return fail(e, SONIC_ERR_INVALID, "%s: node %d has no edge (a transcript ends through an EOS edge, never by running dry)", who, n);
        for (int k = a; k < b; ++k) {
            if (edge_tok[k] < 0 || edge_tok[k] >= vocab) return fail(e, SONIC_ERR_INVALID, "%s: token id %d of node %d is out of vocabulary (%d)", who, edge_tok[k], n, vocab);
            if (edge_tok[k] == audio_id) return fail(e, SONIC_ERR_INVALID, "%s: token id %d of node %d is the audio placeholder, which cannot be emitted", who, edge_tok[k], n);
            if (edge_next[k] < 0 || edge_next[k] >= N) return fail(e, SONIC_ERR_INVALID, "%s: edge %d of node %d leads to node %d (0 .. %d)", who, k - a, n, edge_next[k], N - 1);
            if (k > a && edge_tok[k] <= edge_tok[k - 1]) return fail(e, SONIC_ERR_INVALID, "%s: the edges of node %d are not sorted and unique by token id (%d after %d)", who, n, edge_tok[k], edge_tok[k - 1]);
        }
    }
    out->resize((size_t)GRAM_HEAD + N + 1 + 2 * (size_t)E);
    int* w = out->data();
    w[0] = N; w[1] = E;
    memcpy(w + GRAM_HEAD, node_off, (size_t)(N + 1) * 4);
    memcpy(w + GRAM_HEAD + N + 1, edge_tok, (size_t)E * 4);
    memcpy(w + GRAM_HEAD + N + 1 + E, edge_next, (size_t)E * 4);
    return SONIC_OK;
}
// the packed words [N | E | node_off[N + 1] | edge_tok[E] | edge_next[E]] taken apart again: SONIC_ERR_INVALID when the counts do not fit the length
static int gram_unpack(const char* who, const int* w, int64_t n, const int** off, const int** tok, const int** nxt, int* N, int* E) {
    if (!w || n < GRAM_HEAD) return fail(nullptr, SONIC_ERR_INVALID, "%s: %lld words do not hold the automaton's two counts", who, (long long)n);
    *N = w[0]; *E = w[1];
    if (*N < 1 || *N > GRAM_MAX_NODES) return fail(nullptr, SONIC_ERR_INVALID, "%s: %d nodes (1 .. %d; nothing is truncated)", who, *N, GRAM_MAX_NODES);
    if (*E < 1 || *E > GRAM_MAX_EDGES) return fail(nullptr, SONIC_ERR_INVALID, "%s: %d edges (1 .. %d; nothing is truncated)", who, *E, GRAM_MAX_EDGES);
    if (n != (int64_t)GRAM_HEAD + *N + 1 + 2 * (int64_t)*E) return fail(nullptr, SONIC_ERR_INVALID, "%s: %lld words, %d nodes and %d edges need %lld", who, (long long)n, *N, *E, (long long)GRAM_HEAD + *N + 1 + 2 * (long long)*E);
    *off = w + GRAM_HEAD; *tok = *off + *N + 1; *nxt = *tok + *E;
    return SONIC_OK;
}
// sonic_load_tensor(e, "grammar:<id>", words, SONIC_DTYPE_I32, {n}, 1): created once on a weight owner (a slot's call lands on its owner) under an id the caller
// chooses (1 .. 65535) and shared by every handle of it; n = 0 destroys it - refused by name while a staged or running request refers to it; what is left when the owner
// goes is freed with it.  Does not take the engine lock, so a server can compile a grammar while its handles decode.  The message of a refusal is the calling thread's
int gram_create(sonic_engine* e, int id, const int* words, int64_t n) {
    sonic_engine* root = e->owner ? e->owner : e;
    if (!root->finalized) return fail(nullptr, SONIC_ERR_INVALID, "grammar: the engine's weights are not finalized");
    if (id < 1 || id > 65535) return fail(nullptr, SONIC_ERR_INVALID, "grammar: id %d is outside 1 .. 65535", id);
    if (n == 0) {
        sonic_grammar* g = nullptr;
        {
            std::lock_guard<std::mutex> lk(root->gram_mu);
            auto it = std::find_if(root->grammars.begin(), root->grammars.end(), [&](sonic_grammar* x) { return x->id == id; });
            if (it == root->grammars.end()) return fail(nullptr, SONIC_ERR_INVALID, "grammar: %d is not a live grammar of this engine", id);
            g = *it;
            const int r = g->refs.load();
            if (r > 0) return fail(nullptr, SONIC_ERR_INVALID, "grammar: %d is in use: %d staged or running request%s refer%s to it (fetch or release their rows first)", id, r, r == 1 ? "" : "s", r == 1 ? "s" : "");
            root->grammars.erase(it);
        }
        root->gram_bytes -= g->bytes;
        (void)hipSetDevice(root->device);
        (void)hipDeviceSynchronize();                         // launches queued while a row still referred to it (a finished row's block reads its node until the row is released)
        (void)hipFree(g->dev);
        delete g;
        return SONIC_OK;
    }
    const int *off, *tok, *nxt; int N, E;
    TRY(gram_unpack("grammar", words, n, &off, &tok, &nxt, &N, &E));
    std::vector<int> w;
    TRY(gram_pack(nullptr, "grammar", off, tok, nxt, N, E, root->d.vocab, root->d.audio_token_id, &w));
    if (hipSetDevice(root->device) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, SONIC_ERR_HIP, "grammar: hipSetDevice failed"); }
    sonic_grammar* g = new sonic_grammar();
    g->root = root; g->id = id; g->N = N; g->E = E; g->bytes = (int64_t)w.size() * 4;
    if (hipMalloc((void**)&g->dev, w.size() * 4) != hipSuccess) { (void)hipGetLastError(); delete g; return fail(nullptr, SONIC_ERR_OOM, "HIP out of memory (grammar of %d nodes and %d edges)", N, E); }
    if (hipMemcpy(g->dev, w.data(), w.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(g->dev); delete g; return fail(nullptr, SONIC_ERR_HIP, "grammar: upload failed"); }
    {
        std::lock_guard<std::mutex> lk(root->gram_mu);
        for (sonic_grammar* x : root->grammars) if (x->id == id) { (void)hipFree(g->dev); delete g; return fail(nullptr, SONIC_ERR_INVALID, "grammar: id %d is taken by a live grammar of this engine", id); }
        root->grammars.push_back(g);
    }
    root->gram_bytes += g->bytes;
    return SONIC_OK;
}
// the kernel hooks' automaton (engine_hooks.cpp test_greedy), validated as a grammar is, against the hook's own vocabulary V
int gram_hook_arm(sonic_engine* e, int V, const int* words, int64_t n) {
    const int *off, *tok, *nxt; int N, E;
    if (V < 4 || V > (1 << 24)) return fail(nullptr, SONIC_ERR_INVALID, "grammar.hook: vocabulary %d", V);
    TRY(gram_unpack("grammar.hook", words, n, &off, &tok, &nxt, &N, &E));
    std::vector<int> w;
    TRY(gram_pack(nullptr, "grammar.hook", off, tok, nxt, N, E, V, -1, &w));
    std::lock_guard<std::mutex> lk(e->mu);
    e->hook_gram.swap(w); e->hook_eos.clear();
    for (int b = 0; b < 64; ++b) e->hook_state_in[b] = -1;
    return SONIC_OK;
}
static void gram_unref(sonic_grammar* g) { if (g) g->refs.fetch_sub(1); }
static void gram_drop_staged(sonic_engine* e) {
    for (int r = 0; r < 64; ++r) { gram_unref(e->gram_staged[r]); e->gram_staged[r] = nullptr; }
    e->gram.pending = -1;
}
static inline int* gram_state_of(const sonic_engine* e) { return (int*)(e->gram.dev + 64); }   // the rows' state words behind their references
static void gram_row_release(sonic_engine* e, int row) { if (row >= 0 && row < 64) { gram_unref(e->gram_row[row]); e->gram_row[row] = nullptr; } }
// a live grammar of `root` gains a reference (under the registry's lock: a concurrent destroy either sees it or has already removed the grammar)
static bool gram_ref(sonic_engine* root, sonic_grammar* g) {
    std::lock_guard<std::mutex> lk(root->gram_mu);
    if (std::find(root->grammars.begin(), root->grammars.end(), g) == root->grammars.end()) return false;
    g->refs.fetch_add(1);
    return true;
}
static sonic_grammar* gram_ref_id(sonic_engine* root, int id) {
    std::lock_guard<std::mutex> lk(root->gram_mu);
    for (sonic_grammar* g : root->grammars) if (g->id == id) { g->refs.fetch_add(1); return g; }
    return nullptr;
}
int gram_enable(sonic_engine* e, int on) {
    if (on && e->opt_lm) return fail(e, SONIC_ERR_INVALID, "grammar: option lm is on: a grammar decides and a language model weighs - the kernels hold one of the two (weighted grammars are not built)");
    if (on && !lp_on(e)) return fail(e, SONIC_ERR_INVALID, "grammar: option token_logprobs must be on first (the grammar kernels are log-probability kernels; sonic_set_option(e, \"token_logprobs\", 1))");
    if (on && greedy_guard_lds(e->d.vocab) > 60000) return fail(e, SONIC_ERR_UNSUPPORTED, "grammar: a vocabulary of %d ids does not fit the guard bitmaps", e->d.vocab);
    if (!on && e->opt_grammar) { gram_drop_staged(e); for (int r = 0; r < 64; ++r) gram_row_release(e, r); }
    TRY(stage_enable(e, e->gram, on, &e->opt_grammar, "grammar", GRAM_STAGE_WORDS, true));
    if (on) { launch_fill_i32((int*)e->gram.dev, 0, 128, e->st); launch_fill_i32(gram_state_of(e), -1, 64, e->st); HIPC(e, stream_sync(e)); }      // every row starts free
    return SONIC_OK;
}
// The grammars of the R requests of the next prefill on this handle (the entry points of sonic_set_request_bias), which consumes them.  Options of the handle:
// request_grammar_begin = R stages R free requests, request_grammar = request << 16 | grammar id then names a request's grammar.  The caller holds the lock
static void gram_stage_words(sonic_engine* e) {
    int* st = (int*)(e->gram.host + 64);
    for (int r = 0; r < 64; ++r) { e->gram.host[r] = e->gram_staged[r] ? (unsigned long long)(uintptr_t)e->gram_staged[r]->dev : 0ull; st[r] = e->gram_staged[r] ? 0 : -1; }
}
int gram_stage_begin(sonic_engine* e, int R) {
    if (!e->opt_grammar || !e->gram.dev) return fail(e, SONIC_ERR_INVALID, "request_grammar_begin: option grammar is off on this handle (sonic_set_option(e, \"grammar\", 1) on the owner before its slots are created)");
    gram_drop_staged(e);
    if (R < 1 || R > e->Bm || R > 64) return fail(e, SONIC_ERR_INVALID, "request_grammar_begin: %d requests (1 .. %d)", R, e->Bm);
    HIPC(e, hipSetDevice(e->device));
    TRY(stage_open(e, e->gram));
    gram_stage_words(e);
    e->gram.pending = R;
    return SONIC_OK;
}
int gram_stage_row(sonic_engine* e, int value) {
    const int r = value >> 16, id = value & 0xffff, R = e->gram.pending.load();
    if (!e->opt_grammar || !e->gram.dev) return fail(e, SONIC_ERR_INVALID, "request_grammar: option grammar is off on this handle (sonic_set_option(e, \"grammar\", 1) on the owner before its slots are created)");
    if (R < 0) return fail(e, SONIC_ERR_INVALID, "request_grammar: no batch is staged (option request_grammar_begin first)");
    if (value < 0 || r >= R) { gram_drop_staged(e); return fail(e, SONIC_ERR_INVALID, "request_grammar: request %d of a staged batch of %d", r, R); }
    sonic_grammar* g = gram_ref_id(e->owner ? e->owner : e, id);
    if (!g) { gram_drop_staged(e); return fail(e, SONIC_ERR_INVALID, "request_grammar: %d is not a live grammar of this handle's weight owner (a grammar serves the engine it was created on and its slots)", id); }
    gram_unref(e->gram_staged[r]);
    e->gram_staged[r] = g;
    gram_stage_words(e);
    return SONIC_OK;
}
// dispatch.cpp (same library, not exported): a batch's grammars by pointer (NULL: a free request), under the handle's lock
extern "C" int engine_set_request_grammar(sonic_engine* e, sonic_grammar* const* grammars, int R) {
    if (!e || !grammars) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipGetLastError();
    TRY(gram_stage_begin(e, R));
    sonic_engine* root = e->owner ? e->owner : e;
    for (int r = 0; r < R; ++r) {
        if (!grammars[r]) continue;
        if (!gram_ref(root, grammars[r])) { gram_drop_staged(e); return fail(e, SONIC_ERR_INVALID, "request_grammar: the grammar of request %d is not a live grammar of this handle's weight owner", r); }
        e->gram_staged[r] = grammars[r];
    }
    gram_stage_words(e);
    return SONIC_OK;
}
static int gram_upload(sonic_engine* e, int R) {
    (void)R;
    if (!e->opt_grammar) return SONIC_OK;
    for (int r = 0; r < 64; ++r) gram_row_release(e, r);                  // the rows' former occupants are gone (or were spliced away with references of their own)
    if (!e->gram.take) {                                                   // a batch without grammars: every row free
        gram_drop_staged(e);
        launch_fill_i32((int*)e->gram.dev, 0, 128, e->st); launch_fill_i32(gram_state_of(e), -1, 64, e->st);
        return SONIC_OK;
    }
    for (int r = 0; r < 64; ++r) { e->gram_row[r] = e->gram_staged[r]; e->gram_staged[r] = nullptr; }
    HIPC(e, hipMemcpyAsync(e->gram.dev, e->gram.host, (size_t)GRAM_STAGE_WORDS * 8, hipMemcpyHostToDevice, e->st));
    return stage_sent(e, e->gram);
}
// dispatch.cpp (same library, not exported): the option on a handle; a submitted request's reference (the registry's lock, never the engine lock: a decoding handle
// holds that one for a chunk at a time) and its return
extern "C" int engine_grammar_on(sonic_engine* e) { return e && e->opt_grammar && e->gram.dev ? 1 : 0; }
extern "C" sonic_grammar* engine_grammar_ref_id(sonic_engine* e, int id) { return e ? gram_ref_id(e->owner ? e->owner : e, id) : nullptr; }
extern "C" void engine_grammar_unref(sonic_grammar* g) { gram_unref(g); }
extern "C" int engine_sampling_validate(float temperature) { return samp_check(nullptr, "sampling", &temperature, 1); }
// dispatch.cpp (same library, not exported): is the option on for a handle; is one request's table well-formed for it (the message lands on the handle)
extern "C" int engine_request_bias_on(sonic_engine* e) { return e && e->opt_request_bias && e->bias.dev ? 1 : 0; }
// (the handle is only read for its vocabulary: the message goes to the calling thread's sonic_last_error(NULL), no lock is needed)
extern "C" int engine_bias_validate(sonic_engine* e, const int32_t* seq_ids, const int32_t* seq_off, const float* bias, int n) {
    if (!e) return SONIC_ERR_INVALID;
    std::vector<int> row((size_t)BIAS_ROW_WORDS); int cnt = 0;
    return bias_pack(nullptr, "request_bias", seq_ids, seq_off, bias, n, e->d.vocab, row.data(), &cnt);
}
extern "C" int engine_thread_fail(int code, const char* msg) { return fail(nullptr, code, "%s", msg); }

// ---- option draft_verify (include/sonic_hip.h beside sonic_set_forced_ids): HF generate()'s assisted / prompt-lookup decoding with the draft given by
// the caller.  The caller holds the lock and has asked gen_busy.  No buffer comes with the option: draft_alloc brings them at the handle's first drafted prefill
int draft_enable(sonic_engine* e, int on) {
    if (on && e->opt_lm) return fail(e, SONIC_ERR_INVALID, "draft_verify: option lm is on: the verify pass (rows_kernel) knows no language model");
    if (on && e->i8) return fail(e, SONIC_ERR_INVALID, "draft_verify: the int8 kind refuses it (its prefill finds the outlier columns over the rows of a request: a draft would change the group, and with it the prompt's own values)");
    if (on && e->f32) return fail(e, SONIC_ERR_INVALID, "draft_verify: the fp32 test kind has no verify kernels; use a bf16 or fp16 handle");
    if (on && e->opt_forced_parallel) return fail(e, SONIC_ERR_INVALID, "draft_verify: option forced_parallel is on: a scoring handle decodes nothing a draft could shorten");
    e->opt_draft_verify = on ? 1 : 0; e->draft_pending = -1; e->draft_take = false;
    if (!on) e->draft_last_S = 0;
    return SONIC_OK;
}
// sonic_load_tensor(e, "request_draft", words, SONIC_DTYPE_I32, {n}, 1), words = [R | off[0 .. R] | ids]: the drafts of the R requests of the next prefill on this handle
// (the entry points of sonic_set_request_bias), which consumes them on success and on failure alike.  Refused during an asynchronous run without waiting for its lock
int draft_stage_words(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim) {
    { std::lock_guard<std::mutex> ak(e->a_mu); if (e->a_pending || e->a_running) return fail(nullptr, SONIC_ERR_INVALID, "request_draft: an asynchronous run of this handle is in flight"); }
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipGetLastError();
    e->draft_pending = -1;
    if (!e->opt_draft_verify) return fail(e, SONIC_ERR_INVALID, "request_draft: option draft_verify is off on this handle (sonic_set_option(e, \"draft_verify\", 1) on the owner before its slots are created)");
    if (dtype != SONIC_DTYPE_I32 || ndim != 1 || shape[0] < 3) return fail(e, SONIC_ERR_INVALID, "request_draft: the drafts are one row of int32 words [R | off[0 .. R] | ids] (SONIC_DTYPE_I32, ndim 1)");
    const int* w = (const int*)data; const int64_t n = shape[0];
    const int R = w[0];
    if (R < 1 || R > e->Bm || R > 64 || n < (int64_t)R + 2) return fail(e, SONIC_ERR_INVALID, "request_draft: %d requests (1 .. %d), %lld words", R, e->Bm, (long long)n);
    const int* off = w + 1; const int* ids = w + R + 2;
    if (off[0] != 0 || (int64_t)off[R] != n - (R + 2)) return fail(e, SONIC_ERR_INVALID, "request_draft: the offsets run from %d to %d, the words hold %lld ids", off[0], off[R], (long long)(n - (R + 2)));
    for (int r = 0; r < R; ++r) {
        if (off[r + 1] < off[r]) return fail(e, SONIC_ERR_INVALID, "request_draft: request offsets decrease at request %d", r);
        for (int k = off[r]; k < off[r + 1]; ++k) {
            const int id = ids[k];
            if (id < 0 || id >= e->d.vocab) return fail(e, SONIC_ERR_INVALID, "request_draft: token id %d of request %d is out of vocabulary (%d)", id, r, e->d.vocab);
            if (id == e->d.audio_token_id) return fail(e, SONIC_ERR_INVALID, "request_draft: token id %d of request %d is the audio placeholder, which cannot be emitted", id, r);
            for (int q = 0; q < e->d.n_eos; ++q)
                if (id == e->d.eos[q]) return fail(e, SONIC_ERR_INVALID, "request_draft: token id %d of request %d is an EOS id of this handle (a draft ends in front of it; nothing is truncated)", id, r);
        }
    }
    e->draft_stage.assign(w, w + n);
    e->draft_pending = R;
    return SONIC_OK;
}
int draft_extend(sonic_engine* e, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new,
                 std::vector<int32_t>& ids, std::vector<int64_t>& off, std::vector<int32_t>& left, std::vector<int>& dlen) {
    dlen.clear();
    if (!e->draft_take) return SONIC_OK;
    const int* doff = e->draft_stage.data() + 1; const int* dids = e->draft_stage.data() + R + 2;
    if (doff[R] == 0) return SONIC_OK;                       // every draft is empty: the prefill of today
    if (e->force_d) return fail(e, SONIC_ERR_INVALID, "request_draft: forced ids are set on this handle (sonic_set_forced_ids): teacher forcing decides every token, a draft has nothing to offer");
    const int* gst = e->gram.take ? (const int*)(e->gram.host + 64) : nullptr;
    long asked = 0;
    for (int r = 0; r < R; ++r) {
        const int D = doff[r + 1] - doff[r];
        if (prompt_off[r + 1] - prompt_off[r] < 1) return fail(e, SONIC_ERR_INVALID, "request %d has an empty prompt", r);
        if (max_new[r] < 1) return fail(e, SONIC_ERR_INVALID, "max_new_tokens must be >= 1");
        if (D > max_new[r] - 1) return fail(e, SONIC_ERR_INVALID, "request_draft: the draft of request %d holds %d ids, its budget of %d tokens leaves room for %d (the last token is the model's own; nothing is truncated)", r, D, max_new[r], max_new[r] - 1);
        if (D > 0 && e->bias.take && e->bias.host[r] > 0) return fail(e, SONIC_ERR_INVALID, "request_draft: request %d carries a draft and a request bias table (sonic_set_request_bias): the verify pass applies the handle's processors only", r);
        if (D > 0 && e->samp.take && e->samp.host[3 * r] != 0u) return fail(e, SONIC_ERR_INVALID, "request_draft: request %d carries a draft and a temperature > 0 (sonic_set_request_sampling): a sampled token is not the argmax a draft is checked against", r);
        if (D > 0 && gst && gst[r] != -1) return fail(e, SONIC_ERR_INVALID, "request_draft: request %d carries a draft and a grammar (option request_grammar): the verify pass applies the handle's processors only", r);
        asked += (prompt_off[r + 1] - prompt_off[r]) + D;
    }
    if (asked > e->tok_cap) return fail(e, SONIC_ERR_INVALID, "request_draft: the batch asks for %ld tokens (prompts and drafts), %d fit one prefill (tok_cap)", asked, e->tok_cap);
    off.assign(R + 1, 0); left.resize(R); dlen.resize(R);
    for (int r = 0; r < R; ++r) {
        const int D = doff[r + 1] - doff[r];
        ids.insert(ids.end(), prompt_ids + prompt_off[r], prompt_ids + prompt_off[r + 1]);
        ids.insert(ids.end(), dids + doff[r], dids + doff[r + 1]);
        off[r + 1] = (int64_t)ids.size(); dlen[r] = D; left[r] = max_new[r] - D;      // (plan_requests' context check stays at prompt + max_new)
    }
    return SONIC_OK;
}
int draft_alloc(sonic_engine* e) {
    TRY(score_logits_alloc(e));
    const size_t plan = DraftPlan::words(e->tok_cap);
    if (!e->draft_plan_d) TRY(dalloc(e, &e->draft_plan_d, plan));
    for (int i = 0; i < 2; ++i)
        if (!e->draft_plan_h[i] && hipHostMalloc((void**)&e->draft_plan_h[i], plan * 4, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(e, SONIC_ERR_OOM, "draft_verify: pinned host memory exhausted"); }
    if (!e->ver_tok) TRY(dalloc(e, &e->ver_tok, (size_t)e->tok_cap));
    if (e->ver_rec && e->ver_rec_w != lp_width(e)) TRY(dfree(e, &e->ver_rec, (size_t)e->tok_cap * e->ver_rec_w));
    if (!e->ver_rec) { TRY(dalloc(e, &e->ver_rec, (size_t)e->tok_cap * lp_width(e))); e->ver_rec_w = lp_width(e); }
    if (!e->draft_acc) TRY(dalloc(e, &e->draft_acc, (size_t)64));
    return SONIC_OK;
}
// dispatch.cpp (same library, not exported): one request's draft checked at its submit against the handle's model (which is only read: no lock; the message goes to the
// calling thread's sonic_last_error(NULL)); the tokens one prefill of a handle holds
extern "C" int engine_draft_validate(sonic_engine* e, const int32_t* ids, int n) {
    if (!e || !ids) return SONIC_ERR_INVALID;
    for (int k = 0; k < n; ++k) {
        const int id = ids[k];
        if (id < 0 || id >= e->d.vocab) return fail(nullptr, SONIC_ERR_INVALID, "draft: token id %d is out of vocabulary (%d)", id, e->d.vocab);
        if (id == e->d.audio_token_id) return fail(nullptr, SONIC_ERR_INVALID, "draft: token id %d is the audio placeholder, which cannot be emitted", id);
        for (int q = 0; q < e->d.n_eos; ++q)
            if (id == e->d.eos[q]) return fail(nullptr, SONIC_ERR_INVALID, "draft: token id %d is an EOS id of this handle (a draft ends in front of it; nothing is truncated)", id);
    }
    return SONIC_OK;
}
extern "C" int engine_tok_cap(sonic_engine* e) { return e ? e->tok_cap : 0; }
// ---- row forks (include/sonic_hip.h beside sonic_load_tensor): one prefilled request becomes several rows - Whisper's best_of draws its N samples
// from one encoder pass and one prefill.  No option and no buffer: the counts are staged as a draft's words are, and consumed or dropped with them.
// sonic_load_tensor(e, "request_forks", counts, SONIC_DTYPE_I32, {A}, 1): request a of the next prefill on this handle (the entry points of sonic_set_request_bias)
// becomes counts[a] >= 1 rows.  Refused by name on the int8 and fp32 kinds and on a scoring handle, for a count below 1 and for more rows than the handle has
int fork_stage_counts(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim) {
    { std::lock_guard<std::mutex> ak(e->a_mu); if (e->a_pending || e->a_running) return fail(nullptr, SONIC_ERR_INVALID, "request_forks: an asynchronous run of this handle is in flight"); }
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipGetLastError();
    e->fork_pending = -1;
    if (e->i8) return fail(e, SONIC_ERR_INVALID, "request_forks: the int8 kind refuses it (its decode step keeps quantised rows and outlier lists per row that the prefill's head leaves for the sources alone)");
    if (e->f32) return fail(e, SONIC_ERR_INVALID, "request_forks: the fp32 test kind has no fork kernel; use a bf16 or fp16 handle");
    if (e->opt_lm) return fail(e, SONIC_ERR_INVALID, "request_forks: option lm is on: the fork copies no language-model state");
    if (e->opt_forced_parallel) return fail(e, SONIC_ERR_INVALID, "request_forks: option forced_parallel is on: a scoring handle decodes nothing a fork could sample");
    if (dtype != SONIC_DTYPE_I32 || ndim != 1 || shape[0] < 1) return fail(e, SONIC_ERR_INVALID, "request_forks: the counts are one row of int32 words, one per request (SONIC_DTYPE_I32, ndim 1)");
    const int64_t A = shape[0]; const int* w = (const int*)data;
    if (A > e->Bm || A > 64) return fail(e, SONIC_ERR_INVALID, "request_forks: %lld requests (1 .. %d)", (long long)A, e->Bm);
    long rows = 0;
    for (int a = 0; a < (int)A; ++a) {
        if (w[a] < 1) return fail(e, SONIC_ERR_INVALID, "request_forks: request %d has a fork count of %d (at least 1: the request itself)", a, w[a]);
        rows += w[a];
    }
    if (rows > e->Bm || rows > 64) return fail(e, SONIC_ERR_INVALID, "request_forks: the counts add up to %ld rows, the handle has %d (max_batch)", rows, e->Bm);
    e->fork_stage.assign(w, w + A);
    e->fork_pending = (int)A;
    return SONIC_OK;
}
int fork_claim(sonic_engine* e, int R, std::vector<int>& fork_src) {
    fork_src.clear();
    const int A = e->fork_pending.exchange(-1);
    if (A < 0) return SONIC_OK;
    if (A != R) return fail(e, SONIC_ERR_INVALID, "request_forks: the counts were given for %d requests, the batch has %d", A, R);
    if (e->force_d) return fail(e, SONIC_ERR_INVALID, "request_forks: forced ids are set on this handle (sonic_set_forced_ids): teacher forcing decides every token, forks would all be the same row");
    int rows = 0;
    for (int a = 0; a < A; ++a) rows += e->fork_stage[a];
    if (rows == A) return SONIC_OK;                          // every count 1: the prefill of today
    for (int a = 0; a < A; ++a) fork_src.push_back(a);
    for (int a = 0; a < A; ++a) for (int j = 1; j < e->fork_stage[a]; ++j) fork_src.push_back(a);
    return SONIC_OK;
}

extern "C" int engine_draft_verify_on(sonic_engine* e) { return e && e->opt_draft_verify ? 1 : 0; }      // (pipeline.cpp too: the bulk pipeline refuses such a handle)

// HF generate()'s logits processors for greedy decoding, as the checkpoint's generation_config.json (or the caller) sets them: repetition_penalty (1.0 = none),
// no_repeat_ngram_size (0 = none), suppress_tokens (n_suppress = 0: none; at most 256 ids).  The neutral values switch the guards off: the engine then launches
// the kernels it launched before.  Set it on the owner before slots are created (they copy it).  SONIC_ERR_INVALID for a value out of range, and while the handle
// has work in hand (gen_busy): a prefilled batch whose decode loop has not ended, an asynchronous run, a continuous loop (sonic_service_begin).  The first check
// below is the same one without the engine lock, which an asynchronous run holds until it ends: the call answers at once instead of waiting for it.
extern "C" int sonic_set_generation(sonic_engine* e, float repetition_penalty, int no_repeat_ngram_size, const int32_t* suppress, int n_suppress) {
    if (!e) return SONIC_ERR_INVALID;
    { std::lock_guard<std::mutex> lk(e->a_mu); if (e->a_pending || e->a_running) return fail(nullptr, SONIC_ERR_INVALID, "sonic_set_generation: an asynchronous run of this handle is in flight"); }
    std::lock_guard<std::mutex> lk(e->mu);
    (void)hipGetLastError();
    TRY(gen_busy(e, "sonic_set_generation"));
    return gen_apply(e, repetition_penalty, no_repeat_ngram_size, suppress, n_suppress);
}
// what is in force on this handle (get_model_info, tests): *n_suppress = ids copied to suppress[0 .. cap)
extern "C" int sonic_get_generation(sonic_engine* e, float* repetition_penalty, int32_t* no_repeat_ngram_size, int32_t* suppress, int cap, int32_t* n_suppress) {
    if (!e) return SONIC_ERR_INVALID;
    std::lock_guard<std::mutex> lk(e->mu);
    if (repetition_penalty) *repetition_penalty = e->gen_penalty;
    if (no_repeat_ngram_size) *no_repeat_ngram_size = e->gen_ngram;
    const int n = (int)e->gen_suppress.size();
    if (n_suppress) *n_suppress = n;
    if (suppress) for (int i = 0; i < n && i < cap; ++i) suppress[i] = e->gen_suppress[i];
    return SONIC_OK;
}

// ---- options lm / lm_weight: shallow fusion with a backoff n-gram language model over the model's own tokens - NeMo's n-gram fusion for BPE models, ESPnet's
// ngram_weight - as a weighted automaton on the device: lm_step_kernel (lm.hip) turns a row's state into its additive vector right ahead of every greedy launch, the
// greedy kernel's LM instantiations add it.  Models live on the weight owner, as grammars do; a handle's option names one by id.
// The validation, rule by rule in the words of sonicscribe_amd/ngram.py (NGramLM.validate); the message is the calling thread's (sonic_last_error(NULL))
int lm_check(const char* who, const int* w, int64_t n, int vocab) {
    if (n < LM_WIRE_HEAD) return fail(nullptr, SONIC_ERR_INVALID, "%s: %lld words do not hold the header [V | N | E | order | start]", who, (long long)n);
    const int V = w[0], N = w[1], E = w[2], order = w[3], start = w[4];
    if (V < 1 || N < 1 || E < 0 || n != (int64_t)LM_WIRE_HEAD + V + ((int64_t)N + 1) + 2 * (int64_t)N + 3 * (int64_t)E)
        return fail(nullptr, SONIC_ERR_INVALID, "%s: %lld words, the header (V %d, N %d, E %d) asks for %lld", who, (long long)n, V, N, E, (long long)((int64_t)LM_WIRE_HEAD + V + ((int64_t)N + 1) + 2 * (int64_t)N + 3 * (int64_t)E));
    if (V != vocab) return fail(nullptr, SONIC_ERR_INVALID, "%s: the automaton's vocabulary is %d, the model's %d", who, V, vocab);
    if (order < 1 || order > LM_MAX_ORDER) return fail(nullptr, SONIC_ERR_INVALID, "%s: order %d is outside 1 .. %d", who, order, LM_MAX_ORDER);
    if (N > LM_MAX_NODES) return fail(nullptr, SONIC_ERR_INVALID, "%s: %d nodes (1 .. %d; nothing is truncated)", who, N, LM_MAX_NODES);
    if (E > LM_MAX_EDGES) return fail(nullptr, SONIC_ERR_INVALID, "%s: %d edges (0 .. %d; nothing is truncated)", who, E, LM_MAX_EDGES);
    if (start < 0 || start >= N) return fail(nullptr, SONIC_ERR_INVALID, "%s: start node %d (0 .. %d)", who, start, N - 1);
    const int* uni = w + LM_WIRE_HEAD; const int* off = uni + V; const int* bo_next = off + N + 1; const int* bo_w = bo_next + N;
    const int* tok = bo_w + N; const int* nxt = tok + E; const int* ew = nxt + E;
    auto finite = [](int bits) { return (bits & 0x7f800000) != 0x7f800000; };
    for (int i = 0; i < V; ++i) if (!finite(uni[i])) return fail(nullptr, SONIC_ERR_INVALID, "%s: uni[%d] is not finite", who, i);
    if (off[0] != 0) return fail(nullptr, SONIC_ERR_INVALID, "%s: node_off[0] is %d, not 0", who, off[0]);
    if (off[N] != E) return fail(nullptr, SONIC_ERR_INVALID, "%s: node_off[%d] is %d, not the edge count %d", who, N, off[N], E);
    for (int i = 0; i < N; ++i) if (off[i + 1] < off[i]) return fail(nullptr, SONIC_ERR_INVALID, "%s: node_off is not monotone at node %d", who, i);
    if (bo_next[0] != -1) return fail(nullptr, SONIC_ERR_INVALID, "%s: bo_next[0] is %d, not -1 (node 0 is the root)", who, bo_next[0]);
    for (int i = 1; i < N; ++i) if (bo_next[i] < 0 || bo_next[i] >= i) return fail(nullptr, SONIC_ERR_INVALID, "%s: bo_next[%d] is %d (0 .. %d: nodes are numbered by context length)", who, i, bo_next[i], i - 1);
    {
        std::vector<unsigned char> depth((size_t)N, 0);
        for (int i = 1; i < N; ++i) {
            depth[i] = (unsigned char)(depth[bo_next[i]] + 1);
            if (depth[i] > order - 1) return fail(nullptr, SONIC_ERR_INVALID, "%s: the backoff chain of node %d has %d links (at most order - 1 = %d)", who, i, (int)depth[i], order - 1);
        }
    }
    for (int i = 0; i < N; ++i) if (!finite(bo_w[i])) return fail(nullptr, SONIC_ERR_INVALID, "%s: bo_w[%d] is not finite", who, i);
    for (int k = 0; k < E; ++k) if (tok[k] < 0 || tok[k] >= V) return fail(nullptr, SONIC_ERR_INVALID, "%s: token id %d is out of vocabulary (%d)", who, tok[k], V);
    for (int i = 0; i < N; ++i) for (int k = off[i] + 1; k < off[i + 1]; ++k) if (tok[k] <= tok[k - 1]) return fail(nullptr, SONIC_ERR_INVALID, "%s: the edges of node %d are not sorted and unique by token id", who, i);
    for (int k = 0; k < E; ++k) if (nxt[k] < 0 || nxt[k] >= N) return fail(nullptr, SONIC_ERR_INVALID, "%s: an edge leads to node %d (0 .. %d)", who, nxt[k], N - 1);
    for (int k = 0; k < E; ++k) if (!finite(ew[k])) return fail(nullptr, SONIC_ERR_INVALID, "%s: edge_w[%d] is not finite", who, k);
    for (int k = 0; k < off[1]; ++k) if (ew[k] != uni[tok[k]]) return fail(nullptr, SONIC_ERR_INVALID, "%s: root edge %d (token %d) does not carry the bits of uni[%d]", who, k, tok[k], tok[k]);
    return SONIC_OK;
}
void lm_to_device_words(const int* w, std::vector<int>& out) {
    const int64_t n = (int64_t)LM_WIRE_HEAD + w[0] + ((int64_t)w[1] + 1) + 2 * (int64_t)w[1] + 3 * (int64_t)w[2];
    out.assign((size_t)(n - LM_WIRE_HEAD + LM_HEAD), 0);
    memcpy(out.data(), w, LM_WIRE_HEAD * 4);
    memcpy(out.data() + LM_HEAD, w + LM_WIRE_HEAD, (size_t)(n - LM_WIRE_HEAD) * 4);
}
// sonic_load_tensor(e, "lm:<id>", words, SONIC_DTYPE_I32, {n}, 1): created once on a weight owner (a slot's call lands on its owner) under an id the caller chooses;
// n = 0 destroys it, refused by name while a handle's option lm refers to it; what is left when the owner goes is freed with it.  Takes the owner's registry lock,
// not the engine lock, as gram_create
int lm_create(sonic_engine* e, int id, const int* words, int64_t n) {
    sonic_engine* root = e->owner ? e->owner : e;
    if (!root->finalized) return fail(nullptr, SONIC_ERR_INVALID, "lm: the engine's weights are not finalized");
    if (id < 1 || id > 65535) return fail(nullptr, SONIC_ERR_INVALID, "lm: id %d is outside 1 .. 65535", id);
    if (n == 0) {
        sonic_lm* m = nullptr;
        {
            std::lock_guard<std::mutex> lk(root->gram_mu);
            auto it = std::find_if(root->lms.begin(), root->lms.end(), [&](sonic_lm* x) { return x->id == id; });
            if (it == root->lms.end()) return fail(nullptr, SONIC_ERR_INVALID, "lm: %d is not a live language model of this engine", id);
            m = *it;
            const int r = m->refs.load();
            if (r > 0) return fail(nullptr, SONIC_ERR_INVALID, "lm: %d is in use: option lm of %d handle%s refer%s to it (set it to 0 there, or destroy the handles, first)", id, r, r == 1 ? "" : "s", r == 1 ? "s" : "");
            root->lms.erase(it);
        }
        root->gram_bytes -= m->bytes;
        if (hipSetDevice(root->device) == hipSuccess) (void)hipFree(m->dev);
        (void)hipGetLastError();
        delete m;
        return SONIC_OK;
    }
    TRY(lm_check("lm", words, n, root->d.vocab));
    std::vector<int> w; lm_to_device_words(words, w);
    if (hipSetDevice(root->device) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, SONIC_ERR_HIP, "lm: hipSetDevice failed"); }
    sonic_lm* m = new sonic_lm();
    m->root = root; m->id = id; m->V = words[0]; m->N = words[1]; m->E = words[2]; m->order = words[3]; m->start = words[4]; m->bytes = (int64_t)w.size() * 4;
    if (hipMalloc((void**)&m->dev, w.size() * 4) != hipSuccess) { (void)hipGetLastError(); delete m; return fail(nullptr, SONIC_ERR_OOM, "HIP out of memory (language model of %d nodes and %d edges)", words[1], words[2]); }
    if (hipMemcpy(m->dev, w.data(), w.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(m->dev); delete m; return fail(nullptr, SONIC_ERR_HIP, "lm: upload failed"); }
    {
        std::lock_guard<std::mutex> lk(root->gram_mu);
        for (sonic_lm* x : root->lms) if (x->id == id) { (void)hipFree(m->dev); delete m; return fail(nullptr, SONIC_ERR_INVALID, "lm: id %d is taken by a live language model of this engine", id); }
        root->lms.push_back(m);
    }
    root->gram_bytes += m->bytes;
    return SONIC_OK;
}
static void lm_unref(sonic_engine* e) { if (e->lm) { e->lm->refs.fetch_sub(1); e->lm = nullptr; } e->opt_lm = 0; }
// option lm = id (0: off).  The caller holds the lock and has asked gen_busy
int lm_select(sonic_engine* e, int id, sonic_engine* owner) {
    if (id == 0) { lm_unref(e); drop_graphs(e); return SONIC_OK; }
    if (id < 1 || id > 65535) return fail(e, SONIC_ERR_INVALID, "lm: id %d is outside 0 .. 65535", id);
    if (!lp_on(e)) return fail(e, SONIC_ERR_INVALID, "lm: option token_logprobs must be on first (the language model's kernels are log-probability kernels; sonic_set_option(e, \"token_logprobs\", 1))");
    if (e->opt_grammar) return fail(e, SONIC_ERR_INVALID, "lm: option grammar is on: a grammar decides and a language model weighs - the kernels hold one of the two (weighted grammars are not built)");
    if (e->opt_draft_verify) return fail(e, SONIC_ERR_INVALID, "lm: option draft_verify is on: the verify pass (rows_kernel) knows no language model");
    if (greedy_guard_lds(e->d.vocab, true) + greedy_trunc_lds() > 60000) return fail(e, SONIC_ERR_UNSUPPORTED, "lm: a vocabulary of %d ids does not fit the guard bitmaps", e->d.vocab);
    sonic_engine* root = owner ? owner : e->owner ? e->owner : e;      // (owner: a slot under construction, which does not know its owner yet)
    sonic_lm* m = nullptr;
    {
        std::lock_guard<std::mutex> lk(root->gram_mu);
        for (sonic_lm* x : root->lms) if (x->id == id) { x->refs.fetch_add(1); m = x; break; }
    }
    if (!m) return fail(e, SONIC_ERR_INVALID, "lm: %d is not a live language model of this handle's weight owner (sonic_load_tensor \"lm:<id>\" first)", id);
    HIPC(e, hipSetDevice(e->device));
    HIPC(e, stream_sync(e));
    int s = SONIC_OK;
    if (!e->hist) s = dalloc(e, &e->hist, (size_t)64 * e->max_ctx);
    if (s == SONIC_OK && !e->lm_words) s = dalloc(e, &e->lm_words, (size_t)128);
    if (s == SONIC_OK && !e->lm_add) s = dalloc(e, &e->lm_add, (size_t)e->Bm * e->d.vocab);
    if (s != SONIC_OK) { m->refs.fetch_sub(1); return s; }
    lm_unref(e);
    e->lm = m; e->opt_lm = id;
    launch_fill_i32(e->lm_words, m->start, 64, e->st); launch_fill_i32(e->lm_words + 64, -1, 64, e->st);
    HIPC(e, stream_sync(e));
    drop_graphs(e);                                      // the kernels and their arguments are part of every captured chunk
    return SONIC_OK;
}
int lm_set_weight(sonic_engine* e, int bits) {
    float w; memcpy(&w, &bits, 4);
    if (!std::isfinite(w) || w < 0.f || (bits & 0x80000000)) return fail(e, SONIC_ERR_INVALID, "lm_weight: the value carries the bits of an fp32 weight, finite and >= 0 (got %g)", (double)w);
    e->lm_weight = w;
    drop_graphs(e);                                      // (an argument of the captured lm_step_kernel launches)
    return SONIC_OK;
}
void lm_prefill_rows(sonic_engine* e, int R) {
    if (!lm_live(e)) return;
    launch_fill_i32(e->lm_words, e->lm->start, R, e->st); launch_fill_i32(e->lm_words + 64, -1, R, e->st);
}
void lm_step(sonic_engine* e, int R) {
    if (!lm_live(e)) return;
    launch_lm_step(LmArgs{e->lm->dev, e->lm_words, e->lm_words + 64, e->finished, e->lm_add, e->lm_weight, R}, e->st);
}
extern "C" int engine_lm_on(sonic_engine* e) { return e && e->opt_lm ? 1 : 0; }      // (pipeline.cpp: the bulk pipeline refuses such a handle)

// ---- the stages at every point of a request's life.  Each function below names bias, samp, gram and trunc once, in that order; no other unit names them together.  (No
// descriptor table: the stages' words differ in type - int, unsigned, 64-bit - so a table would erase the types to save one line in three per function.)
int req_claim(sonic_engine* e, int R, bool forked) {
    const int bias_R = e->bias.claim(), samp_R = e->samp.claim(), gram_R = e->gram.claim(), trunc_R = e->trunc.claim();
    TRY(stage_count(e, bias_R, R, "sonic_set_request_bias", "tables", forked));
    TRY(stage_count(e, samp_R, R, "sonic_set_request_sampling", "values", forked));
    TRY(stage_count(e, gram_R, R, "option request_grammar_begin", "grammars", forked));
    TRY(stage_count(e, trunc_R, R, "sonic_load_tensor \"request_truncation\"", "values", forked));
    e->bias.take = bias_R >= 0; e->samp.take = samp_R >= 0; e->gram.take = gram_R >= 0; e->trunc.take = trunc_R >= 0;      // (read by req_upload alone, which only a prefill that got past this reaches)
    const int draft_R = e->draft_pending.exchange(-1);      // the drafts (option draft_verify) are no stage - their words become part of the prefill's plan - but are claimed and dropped with them
    e->draft_take = false;
    if (forked && draft_R >= 0) return fail(e, SONIC_ERR_INVALID, "request_forks: the same prefill was given drafts (sonic_load_tensor \"request_draft\"): a drafted request takes its first tokens from the verify pass, its forks would have none to share");
    TRY(stage_count(e, draft_R, R, "sonic_load_tensor \"request_draft\"", "drafts"));
    e->draft_take = draft_R >= 0;
    return SONIC_OK;
}
const char* req_claim_none(sonic_engine* e) {
    const int bias_R = e->bias.claim(), samp_R = e->samp.claim(), gram_R = e->gram.claim(), trunc_R = e->trunc.claim();      // (claim leaves `take` false: the run's upload writes the neutral values)
    if (gram_R >= 0) gram_drop_staged(e);
    e->draft_pending = -1; e->draft_take = false;      // (the option is refused on a scoring handle: nothing can be staged)
    e->fork_pending = -1;                              // (fork counts likewise)
    return bias_R >= 0 ? "request bias tables (sonic_set_request_bias)" : samp_R >= 0 ? "sampling values (sonic_set_request_sampling)" : gram_R >= 0 ? "grammars (option request_grammar)" : trunc_R >= 0 ? "truncation values (sonic_load_tensor \"request_truncation\")" : nullptr;
}
void req_drop_pending(sonic_engine* e) { e->bias.pending = -1; e->samp.pending = -1; e->trunc.pending = -1; if (e->opt_grammar) gram_drop_staged(e); e->draft_pending = -1; e->fork_pending = -1; }
int req_upload(sonic_engine* e, int R) {      // (in this order: the copies and fills go onto the stream in it)
    TRY(bias_upload(e, R));                   // every request's table, or a zero count, into its row
    TRY(gram_upload(e, R));                   // every request's grammar at its start node, or a free row
    TRY(samp_upload(e, R));                   // every request's (temperature, seed), or zeros: greedy
    return trunc_upload(e, R);                // every row's (top_k, top_p, min_p), or zeros: the filters off
}
void req_greedy_args(const sonic_engine* e, GreedyArgs& g) {
    if (e->opt_request_bias) g.bias_tab = e->bias.dev;
    if (e->opt_sampling && g.out_lp) g.samp = e->samp.dev;      // (the option is refused without token_logprobs, and token_logprobs cannot leave while it is on)
    if (e->opt_truncation && g.samp) g.trunc = e->trunc.dev;   // (the option is refused without sampling, and sampling cannot leave while it is on)
    if (e->opt_grammar && g.out_lp && g.hist) { g.gram_ref = e->gram.dev; g.gram_state = gram_state_of(e); }      // (likewise; the option brought the history)
    if (lm_live(e) && g.out_lp && g.hist) { g.lm_add = e->lm_add; g.lm_tok = e->lm_words + 64; }      // (option lm - no stage: a handle's option - rides here with the families' other pointers)
}
int req_graph_key(const sonic_engine* e) { return (e->opt_request_bias ? GK_BIAS : 0) + (e->opt_sampling ? GK_SAMPLE : 0) + (e->opt_grammar ? GK_GRAMMAR : 0) + (e->opt_truncation ? GK_TRUNC : 0) + (e->opt_lm ? GK_LM : 0); }
int req_splice_check(sonic_engine* d, sonic_engine* p) {
    const char* opt = nullptr;
    if (d->opt_request_bias != p->opt_request_bias || (d->opt_request_bias && !(p->bias.dev && d->bias.dev && p->hist && d->hist))) opt = "request_bias";
    else if (d->opt_sampling != p->opt_sampling || (d->opt_sampling && !(p->samp.dev && d->samp.dev))) opt = "sampling";
    else if (d->opt_truncation != p->opt_truncation || (d->opt_truncation && !(p->trunc.dev && d->trunc.dev))) opt = "truncation";
    else if (d->opt_grammar != p->opt_grammar || (d->opt_grammar && !(p->gram.dev && d->gram.dev))) opt = "grammar";
    else if (d->opt_draft_verify != p->opt_draft_verify) opt = "draft_verify";
    else if (d->opt_lm != p->opt_lm || (d->opt_lm && !(lm_live(p) && lm_live(d)))) opt = "lm";
    else if (d->opt_lm && memcmp(&d->lm_weight, &p->lm_weight, 4)) opt = "lm_weight";
    return opt ? fail(d, SONIC_ERR_INVALID, "sonic_splice_rows: source and destination differ in option %s: set it on the owner before its slots are created", opt) : SONIC_OK;
}
void req_splice_args(sonic_engine* d, sonic_engine* p, SpliceArgs& a, const int32_t* src_rows, const int32_t* dst_rows, int n) {
    if (d->opt_request_bias) { a.bias_s = p->bias.dev; a.bias_d = d->bias.dev; }
    if (d->opt_sampling) { a.samp_s = p->samp.dev; a.samp_d = d->samp.dev; }
    if (d->opt_truncation) { a.trunc_s = p->trunc.dev; a.trunc_d = d->trunc.dev; }
    if (lm_live(d)) { a.lm_s = p->lm_words; a.lm_d = d->lm_words; }
    if (d->opt_grammar) {
        a.gram_s = p->gram.dev; a.gram_d = d->gram.dev;
        for (int i = 0; i < n; ++i) {                      // the row is handed over and its reference with it: the source row is free (the kernel resets its words)
            sonic_grammar* g = p->gram_row[src_rows[i]];
            p->gram_row[src_rows[i]] = nullptr;
            gram_row_release(d, dst_rows[i]);
            d->gram_row[dst_rows[i]] = g;
        }
    }
}
void req_rows_free(sonic_engine* e) {
    if (e->opt_grammar) { launch_fill_i32(gram_state_of(e), -1, 64, e->st); for (int r = 0; r < 64; ++r) gram_row_release(e, r); }
}
int* req_release_state(const sonic_engine* e) { return e->opt_grammar ? gram_state_of(e) : nullptr; }
void req_row_release(sonic_engine* e, int row) { gram_row_release(e, row); }      // (a finished row changes no state and reads no automaton that matters: its reference can go)
void req_batch_fetched(sonic_engine* e, const int* fin, int R) {
    if (!e->opt_grammar) return;
    bool ended = true;                   // (state -1: a later sonic_decode_step reads no automaton)
    for (int r = 0; r < R; ++r) ended = ended && fin[r];
    bool any = false;
    for (int r = 0; r < 64; ++r) any = any || e->gram_row[r];
    if (ended && any) {
        launch_fill_i32((int*)e->gram.dev, 0, 128, e->st); launch_fill_i32(gram_state_of(e), -1, 64, e->st);
        for (int r = 0; r < 64; ++r) gram_row_release(e, r);
    }
}
// sonic_slot_create: a slot generates as its owner does.  Set the options on the owner before its slots are created
int gen_inherit(sonic_engine* e, const sonic_engine* root) {
    e->opt_token_logprobs = root->opt_token_logprobs; e->opt_top_logprobs = root->opt_token_logprobs ? root->opt_top_logprobs : 0;      // (before lp_alloc: the buffer comes at its width)
    if (e->opt_token_logprobs) TRY(lp_alloc(e));
    if (root->gen_on) TRY(gen_apply(e, root->gen_penalty, root->gen_ngram, root->gen_suppress.data(), (int)root->gen_suppress.size()));
    if (root->opt_request_bias) TRY(bias_enable(e, 1));
    e->opt_bias_fill = root->opt_bias_fill;
    if (root->opt_sampling) TRY(samp_enable(e, 1));
    e->opt_samp_fill_milli = root->opt_samp_fill_milli;
    if (root->opt_truncation) TRY(trunc_enable(e, 1));
    e->opt_trunc_fill = root->opt_trunc_fill;
    if (root->opt_grammar) TRY(gram_enable(e, 1));
    e->opt_forced_parallel = root->opt_forced_parallel; e->opt_forced_fanout = root->opt_forced_fanout; e->opt_score_chunk_rows = root->opt_score_chunk_rows;      // (the buffers come with the slot's first parallel run)
    e->opt_forced_align = root->opt_forced_align; e->align_heads = root->align_heads;      // (likewise)
    e->opt_forced_share_prompt = root->opt_forced_share_prompt;      // (likewise)
    if (root->opt_lm) { e->lm_weight = root->lm_weight; TRY(lm_select(e, root->opt_lm, const_cast<sonic_engine*>(root))); }
    e->opt_draft_verify = root->opt_draft_verify;      // (the buffers come with the slot's first drafted prefill)
    return SONIC_OK;
}
// sonic_destroy (the stream is drained): the references of this handle's staged requests and rows, the grammars the caller left on an owner (its slots are gone:
// nothing refers to them), the stages' pinned mirrors and events.  (Their device words are in e->allocs.)
void gen_release(sonic_engine* e) {
    gram_drop_staged(e);
    for (int r = 0; r < 64; ++r) gram_row_release(e, r);
    for (sonic_grammar* g : e->grammars) { (void)hipFree(g->dev); delete g; }
    lm_unref(e);
    for (sonic_lm* m : e->lms) { (void)hipFree(m->dev); delete m; }
    e->lms.clear();
    e->grammars.clear();
    stage_free(e->bias); stage_free(e->samp); stage_free(e->gram); stage_free(e->trunc);
    for (int i = 0; i < 2; ++i) if (e->draft_plan_h[i]) (void)hipHostFree(e->draft_plan_h[i]);
    for (int i = 0; i < 2; ++i) if (e->fork_ev[i]) (void)hipEventDestroy(e->fork_ev[i]);
}
