// sonic_hip engine: the experiment knobs (sonic_set_option) and the debug read-back (sonic_debug_read, sonic_debug_ktrace).
#include "engine_internal.h"

void drop_graphs(sonic_engine* e) { for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.second); e->graphs.clear(); }
// ---- the knobs that do more than store an integer (OptRow::apply)
static int opt_token_logprobs(sonic_engine* e, const char*, int value) {      // per-token log-probabilities beside the ids (greedy_kernel<T, true>)
    const int v = value ? 1 : 0;
    if (!v && e->opt_sampling) return fail(e, SONIC_ERR_INVALID, "token_logprobs cannot be switched off while option sampling is on (its kernels are log-probability kernels)");
    if (!v && e->opt_grammar) return fail(e, SONIC_ERR_INVALID, "token_logprobs cannot be switched off while option grammar is on (its kernels are log-probability kernels)");
    if (!v && e->opt_lm) return fail(e, SONIC_ERR_INVALID, "token_logprobs cannot be switched off while option lm is on (its kernels are log-probability kernels)");
    if (!v && e->opt_top_logprobs) return fail(e, SONIC_ERR_INVALID, "token_logprobs cannot be switched off while option top_logprobs is on (its kernels are log-probability kernels)");
    e->opt_token_logprobs = v; drop_graphs(e);
    return v ? lp_alloc(e) : SONIC_OK;      // first use: 64 x out_cap fp32
}
// the K best alternatives of every step beside the token's log-probability (greedy_kernel<T, true, ., ., ., true>): K in 0 .. 8, on the owner before its
// slots are created (they copy it), after token_logprobs (refused by name otherwise).  Refused while the handle has work in hand, by sonic_set_generation's rule
static int opt_top_logprobs(sonic_engine* e, const char* key, int value) { TRY(gen_busy(e, key)); return top_enable(e, value); }
// the generation guards one integer at a time, for drivers that only speak key = value (bench.py --opt; tools/ab_generation_guards.sh): the penalty in
// thousandths, the n-gram size, ONE suppressed id (-1: none).  Same rules and refusals as sonic_set_generation; the other two values stay as they are
static int opt_gen(sonic_engine* e, const char* key, int value) {
    float p = e->gen_penalty; int n = e->gen_ngram; std::vector<int> sup = e->gen_suppress;
    if (!strcmp(key, "gen_repetition_penalty_milli")) p = (float)((double)value / 1000.0);
    else if (!strcmp(key, "gen_no_repeat_ngram_size")) n = value;
    else { sup.clear(); if (value >= 0) sup.push_back(value); }      // gen_suppress_token
    TRY(gen_busy(e, key));
    return gen_apply(e, p, n, sup.data(), (int)sup.size());
}
// temperature sampling (sonic_set_request_sampling): on the owner before its slots are created (they copy it), after token_logprobs (refused by
// name otherwise); allocates the rows' (temperature, seed) words.  Refused while the handle has work in hand, by sonic_set_generation's rule
static int opt_sampling(sonic_engine* e, const char* key, int value) { TRY(gen_busy(e, key)); return samp_enable(e, value ? 1 : 0); }
static int opt_sampling_fill_milli(sonic_engine* e, const char* key, int value) {    // measurement aid (samp_upload, engine_generation.cpp): 0 (off) or 1 .. 100000 thousandths, for every request without values
    if (value != 0 && (value < 1 || value > 100000)) return fail(e, SONIC_ERR_INVALID, "sampling_fill_milli: %d is outside 0, 1 .. 100000", value);
    TRY(gen_busy(e, key)); e->opt_samp_fill_milli = value; return SONIC_OK;
}
// grammar-constrained decoding (options request_grammar_begin / request_grammar): on the owner before its slots are created (they copy it), after token_logprobs (refused by
// name otherwise); allocates the rows' history, if nothing else has, and their references and state words.  Refused while the handle has work in hand
// top_k / top_p / min_p (sonic_load_tensor "request_truncation"): on the owner before its slots are created (they copy it), after sampling (refused by name
// otherwise); allocates the rows' words.  Refused while the handle has work in hand.  truncation_fill: measurement aid (trunc_upload, engine_generation.cpp)
static int opt_truncation(sonic_engine* e, const char* key, int value) { TRY(gen_busy(e, key)); return trunc_enable(e, value ? 1 : 0); }
static int opt_truncation_fill(sonic_engine* e, const char* key, int value) { TRY(gen_busy(e, key)); e->opt_trunc_fill = value ? 1 : 0; return SONIC_OK; }
static int opt_grammar(sonic_engine* e, const char* key, int value) { TRY(gen_busy(e, key)); return gram_enable(e, value ? 1 : 0); }
// shallow fusion: lm = the id of a language model of the weight owner (sonic_load_tensor "lm:<id>"; 0: off), lm_weight = the bits of the fp32 weight, finite
// and >= 0.  On the owner before its slots are created (they copy both), after token_logprobs (refused by name otherwise; also beside grammar and draft_verify);
// allocates the rows' history, if nothing else has, their state words and the vector buffer.  Refused while the handle has work in hand
static int opt_lm(sonic_engine* e, const char* key, int value) { TRY(gen_busy(e, key)); return lm_select(e, value); }
static int opt_lm_weight(sonic_engine* e, const char* key, int value) { TRY(gen_busy(e, key)); return lm_set_weight(e, value); }
// the kernel hooks' rows (an armed "lm.hook:<V>"): hook_lm_state = row << 24 | state, hook_lm_tok = row << 24 | (token + 1) (0: none pending), hook_lm_weight = the bits
static int opt_hook_lm(sonic_engine* e, const char* key, int value) {
    if (!e->hook_lm || !e->hook_lm_V) return fail(e, SONIC_ERR_INVALID, "%s: arm a hook language model first (sonic_load_tensor \"lm.hook:<V>\")", key);
    if (!strcmp(key, "hook_lm_weight")) { float w; memcpy(&w, &value, 4); if (!std::isfinite(w) || value < 0) return fail(e, SONIC_ERR_INVALID, "hook_lm_weight: the bits of a finite fp32 >= 0"); e->hook_lm_weight = w; return SONIC_OK; }
    const int b = (value >> 24) & 63, v = value & 0xffffff;
    if (value < 0) return fail(e, SONIC_ERR_INVALID, "%s: row %d, value %d", key, b, v);
    if (!strcmp(key, "hook_lm_state")) { if (v >= e->hook_lm_N) return fail(e, SONIC_ERR_INVALID, "hook_lm_state: row %d, state %d of %d nodes", b, v, e->hook_lm_N); e->hook_lm_in[b] = v; }
    else e->hook_lm_in[64 + b] = v - 1;      // (a token outside the vocabulary is the kernel's to handle)
    return SONIC_OK;
}
// ... and the values that travel through the options, since the feature adds no entry point: the grammars of the requests of the next prefill (begin = R requests, all
// free; then request << 16 | grammar id per constrained request), the kernel hooks' row states and EOS ids
static int opt_request_grammar_begin(sonic_engine* e, const char*, int value) { return gram_stage_begin(e, value); }
static int opt_request_grammar(sonic_engine* e, const char*, int value) { return gram_stage_row(e, value); }
static int opt_hook_grammar_state(sonic_engine* e, const char*, int value) {      // row << 20 | (state + 2)
    const int b = value >> 20, st = (value & 0xfffff) - 2;
    if (value < 0 || b > 63 || e->hook_gram.empty() || st >= e->hook_gram[0]) return fail(e, SONIC_ERR_INVALID, "hook_grammar_state: row %d, state %d (arm a hook grammar first: sonic_load_tensor \"grammar.hook:<V>\")", b, st);
    e->hook_state_in[b] = st; return SONIC_OK;
}
static int opt_hook_grammar_eos(sonic_engine* e, const char*, int value) {
    if (value < 0 || e->hook_gram.empty() || e->hook_eos.size() >= 8) return fail(e, SONIC_ERR_INVALID, "hook_grammar_eos: id %d (at most 8 ids, behind an armed hook grammar)", value);
    e->hook_eos.push_back(value); return SONIC_OK;
}
// per-request sequence bias (sonic_set_request_bias): on the owner before its slots are created (they copy it); allocates the rows' history, if the
// guards have not, and their tables.  Refused while the handle has work in hand, by sonic_set_generation's rule
static int opt_request_bias(sonic_engine* e, const char* key, int value) { TRY(gen_busy(e, key)); return bias_enable(e, value ? 1 : 0); }
static int opt_request_bias_fill(sonic_engine* e, const char* key, int value) {      // measurement aid (bias_upload, engine_generation.cpp): 0 .. min(256, vocabulary) neutral entries for every request without a table
    if (value < 0 || value > BIAS_MAX_ENTRIES || value > e->d.vocab) return fail(e, SONIC_ERR_INVALID, "request_bias_fill: %d is outside 0 .. %d", value, BIAS_MAX_ENTRIES);
    TRY(gen_busy(e, key)); e->opt_bias_fill = value; return SONIC_OK;
}
// the parallel forced run (include/sonic_hip.h beside sonic_set_forced_ids).  forced_parallel: on the owner (its slots copy it) or on a slot alone;
// refused while the handle has work in hand, as the options above.  forced_fanout = N: the run's R sequences are R / N audio requests with N candidates each
static int opt_forced_parallel(sonic_engine* e, const char* key, int value) {
    TRY(gen_busy(e, key));
    if (value && e->opt_draft_verify) return fail(e, SONIC_ERR_INVALID, "forced_parallel: option draft_verify is on: a scoring handle decodes nothing a draft could shorten");
    if (!value && e->opt_forced_align) return fail(e, SONIC_ERR_INVALID, "forced_parallel cannot be switched off while option forced_align is on (the alignment rides on the parallel forced run)");
    if (!value && e->opt_forced_share_prompt) return fail(e, SONIC_ERR_INVALID, "forced_parallel cannot be switched off while option forced_share_prompt is on (the shared prompt is the parallel forced run's)");
    e->opt_forced_parallel = value ? 1 : 0; return SONIC_OK;
}
// forced_share_prompt: the forced_fanout candidates of one audio share ONE prefill of their prompt - only on a scoring handle of the bf16 / fp16 kinds
// without forced_align; refused while the handle has work in hand.  (Read by a parallel run as it starts, which also checks that a group's prompts are one prompt.)
static int opt_forced_share_prompt(sonic_engine* e, const char* key, int value) {
    TRY(gen_busy(e, key));
    if (value && !e->opt_forced_parallel) return fail(e, SONIC_ERR_INVALID, "forced_share_prompt: option forced_parallel must be on first (the shared prompt is the parallel forced run's; sonic_set_option(e, \"forced_parallel\", 1))");
    if (value && e->i8) return fail(e, SONIC_ERR_INVALID, "forced_share_prompt: not on an int8 handle (its prefill finds outlier columns per sequence - one sequence = one reference call - and a shared prompt belongs to several)");
    if (value && e->f32) return fail(e, SONIC_ERR_INVALID, "forced_share_prompt: the fp32 kind has no shared-prefix attention kernel; use a bf16 or fp16 handle");
    if (value && e->opt_forced_align) return fail(e, SONIC_ERR_INVALID, "forced_share_prompt: option forced_align is on (the alignment kernels read a sequence's audio keys from its own row)");
    e->opt_forced_share_prompt = value ? 1 : 0; return SONIC_OK;
}
static int opt_forced_fanout(sonic_engine* e, const char* key, int value) {
    if (value < 1 || value > e->Bm) return fail(e, SONIC_ERR_INVALID, "forced_fanout: %d is outside 1 .. %d (max_batch)", value, e->Bm);
    e->opt_forced_fanout = value; return SONIC_OK;      // (only read by a parallel run as it starts)
}
// draft-verified decoding (sonic_load_tensor "request_draft"): on the owner before its slots are created (they copy it); refused by name on the int8 and
// fp32 kinds, on a scoring handle and while the handle has work in hand
static int opt_draft_verify(sonic_engine* e, const char* key, int value) { TRY(gen_busy(e, key)); return draft_enable(e, value ? 1 : 0); }
// word timestamps on the parallel forced run (include/sonic_hip.h beside sonic_set_forced_ids).  forced_align: only on a scoring handle, never on the
// fp32 kind (its prefill keeps no roped queries), refused while the handle has work in hand.  align_head = l * 256 + h adds head h of decoder layer l to the selection
// (-1: back to the default, every head of the last ceil(dec_layers / 2) layers)
static int opt_forced_align(sonic_engine* e, const char* key, int value) {
    TRY(gen_busy(e, key));
    if (value && e->f32) return fail(e, SONIC_ERR_INVALID, "forced_align: the fp32 kind has no alignment kernels (its prefill keeps no roped queries); use a bf16 or int8-mode handle");
    if (value && e->opt_forced_share_prompt) return fail(e, SONIC_ERR_INVALID, "forced_align: option forced_share_prompt is on (the alignment kernels read a sequence's audio keys from its own row); switch it off first");
    if (value && !e->opt_forced_parallel) return fail(e, SONIC_ERR_INVALID, "forced_align: option forced_parallel must be on first (the alignment rides on the parallel forced run; sonic_set_option(e, \"forced_parallel\", 1))");
    e->opt_forced_align = value ? 1 : 0;
    if (!value) e->align_last = false;
    return SONIC_OK;
}
static int opt_align_head(sonic_engine* e, const char* key, int value) {
    TRY(gen_busy(e, key));
    if (value == -1) { e->align_heads.clear(); return SONIC_OK; }
    const int l = value >> 8, h = value & 255;
    if (value < 0 || l >= e->d.dec_layers || h >= e->d.dec_heads) return fail(e, SONIC_ERR_INVALID, "align_head: %d (layer %d, head %d) is outside %d layers x %d heads", value, l, h, e->d.dec_layers, e->d.dec_heads);
    if (std::find(e->align_heads.begin(), e->align_heads.end(), value) != e->align_heads.end()) return SONIC_OK;
    if (e->align_heads.size() >= ALIGN_MAX_HEADS) return fail(e, SONIC_ERR_INVALID, "align_head: the list already holds %d heads", ALIGN_MAX_HEADS);
    e->align_heads.insert(std::upper_bound(e->align_heads.begin(), e->align_heads.end(), value), value);      // sorted: layer by layer, heads ascending
    return SONIC_OK;
}
// fetch_stream (A/B, default 0): 1 = finished rows leave as before the pinned mirror (engine_service.cpp) - copy commands on a stream of the handle's own, created by
// sonic_service_begin, and a wait - and the bulk pipeline queues a chunk ahead of every fetch again.  Same ids either way.  On the owner before its slots are
// created (they copy it); refused while the handle decodes continuously (its loop mirrors rows or does not, from sonic_service_begin on)
static int opt_fetch_stream(sonic_engine* e, const char* key, int value) {
    if (e->svc_on) return fail(e, SONIC_ERR_INVALID, "%s: this handle is decoding continuously (sonic_service_end first)", key);
    e->opt_fetch_stream = value ? 1 : 0; return SONIC_OK;
}
extern "C" int engine_fetch_stream_on(sonic_engine* e) { return e && e->opt_fetch_stream ? 1 : 0; }      // (pipeline.cpp: the order of chunk and fetch at a hand-over)
// mode fp8: matrix m of the snapped set - layer * 4 + {0 q|k|v, 1 o_proj, 2 gate/up, 3 down_proj}, 4 * layers = the tied lm_head - as the bf16 tiles,
// the e4m3 copy and the scales' slots of this handle with its shape; false past the last one
struct Fp8Mat { bf16_t* wt; unsigned char** w8; float** sc; int N, K; };
static bool fp8_mat(sonic_engine* e, int m, Fp8Mat* out) {
    const sonic_dims& d = e->d;
    if (m < 0 || m > 4 * d.dec_layers) return false;
    if (m == 4 * d.dec_layers) { *out = Fp8Mat{e->embed_t, &e->embed8, &e->embed_sc, d.vocab, d.dec_d}; return true; }
    DecLayerW& L = e->dec[m / 4];
    switch (m % 4) {
        case 0: *out = Fp8Mat{L.wqkv_t, &L.qkv8, &L.qkv_sc, e->qkvN, d.dec_d}; break;
        case 1: *out = Fp8Mat{L.wo_t, &L.o8, &L.o_sc, d.dec_d, e->QD}; break;
        case 2: *out = Fp8Mat{L.wgu_t8 ? L.wgu_t8 : L.wgu_t, &L.gu8, &L.gu_sc, 2 * d.dec_ff, d.dec_d}; break;
        default: *out = Fp8Mat{L.wdown_t, &L.down8, &L.down_sc, d.dec_d, d.dec_ff}; break;
    }
    return true;
}
// fp8_weights = 1: every decoder matrix and the embedding of a finalized bf16 weight owner are snapped onto their rows' e4m3 grids in place (fp8_snap_kernel), the
// e4m3 copies and scales are allocated beside them (N K + 4 N bytes each, part of weight_bytes and of sonic_memory_info), the graphs are dropped and fp8_chain goes
// on.  Once, before the owner's slots exist (they share the weights and copy both values); 0 after 1 is refused: the weights cannot be un-snapped
static int opt_fp8_weights(sonic_engine* e, const char* key, int value) {
    if (e->i8 || e->f32 || e->dt != DT_BF16) return fail(e, SONIC_ERR_INVALID, "%s: only on a bf16 handle (this one is of the %s kind): the e4m3 grid is snapped into bf16 weights", key, e->i8 ? "int8" : e->f32 ? "fp32" : "fp16");
    if (e->owner) return fail(e, SONIC_ERR_INVALID, "%s: this handle is a slot: set the option on the weight owner before its slots are created (they share its weights)", key);
    if (!e->slots.empty()) return fail(e, SONIC_ERR_INVALID, "%s: the owner already has %d slot(s): set the option before sonic_slot_create (the slots share the weights and copy the option)", key, (int)e->slots.size());
    TRY(gen_busy(e, key));      // an asynchronous run, a continuous loop, a batch in hand: they read the weights
    if (!value) return e->opt_fp8_weights ? fail(e, SONIC_ERR_INVALID, "%s cannot be switched off: the weights were snapped in place and cannot be un-snapped (option fp8_chain = 0 runs the snapped model on the default chains)", key) : (int)SONIC_OK;
    if (e->opt_fp8_weights) return SONIC_OK;
    if (!e->finalized) return fail(e, SONIC_ERR_INVALID, "%s: the weights are not finalized", key);
    const int n_mat = 4 * e->d.dec_layers + 1;
    Fp8Mat mt{};
    for (int m = 0; m < n_mat; ++m) {
        fp8_mat(e, m, &mt);
        if (!mt.wt) return fail(e, SONIC_ERR_INVALID, "%s: decoder matrix %d has no fragment-tiled copy", key, m);
        if (mt.N % 16 || mt.K % 64) return fail(e, SONIC_ERR_INVALID, "%s: decoder matrix %d is %d x %d: the e4m3 tiling needs rows in 16s and K in 64s", key, m, mt.N, mt.K);
    }
    for (const DecLayerW& L : e->dec)
        if (L.wqkv || L.wo || L.wgu || L.wdown) return fail(e, SONIC_ERR_INVALID, "%s: this handle keeps row-major decoder weights (SONIC_KEEP_ROWMAJOR), which the snap does not rewrite", key);
    HIPC(e, hipSetDevice(e->device));
    for (int m = 0; m < n_mat; ++m) {      // everything is allocated before anything is rewritten: out of memory leaves the bf16 model as it was
        fp8_mat(e, m, &mt);
        if (!*mt.w8) TRY(dalloc(e, mt.w8, (size_t)mt.N * mt.K, false));
        if (!*mt.sc) TRY(dalloc(e, mt.sc, (size_t)mt.N, false));
    }
    for (int m = 0; m < n_mat; ++m) {
        fp8_mat(e, m, &mt);
        launch_fp8_snap(mt.wt, *mt.w8, *mt.sc, m == n_mat - 1 ? e->embed : nullptr, mt.N, mt.K, e->st);      // the token lookup's row-major embedding takes the lm_head's W' too
        e->weight_bytes += (int64_t)mt.N * mt.K + (int64_t)mt.N * 4;
    }
    HIPC(e, hipGetLastError());
    HIPC(e, stream_sync(e));
    e->opt_fp8_weights = 1; e->opt_fp8_chain = 1; e->fp8_step_builds = 0;
    drop_graphs(e);
    return SONIC_OK;
}
// fp8_chain (the A/B of mode fp8): 1 = token steps of <= 4 rows stream the e4m3 copies, 0 = the snapped model on the default chains (full batch invariance, no byte saving)
static int opt_fp8_chain(sonic_engine* e, const char* key, int value) {
    if (!e->opt_fp8_weights) return fail(e, SONIC_ERR_INVALID, "%s: option fp8_weights must be on first (sonic_set_option(e, \"fp8_weights\", 1) on the weight owner)", key);
    if (value != 0 && value != 1) return fail(e, SONIC_ERR_INVALID, "%s: %d is neither 0 nor 1", key, value);
    if (e->svc_on) return fail(e, SONIC_ERR_INVALID, "%s: this handle is decoding continuously (sonic_service_end first)", key);
    e->opt_fp8_chain = value; drop_graphs(e);
    return SONIC_OK;
}
// the two knobs that do device work
static int opt_ktrace(sonic_engine* e, const char*, int value) {              // diagnostics: record in-kernel timestamps of decoder layer `value` (-1: off); sonic_debug_ktrace reads them
    HIPC(e, hipSetDevice(e->device));
    if (value >= 0 && !e->kt) { TRY(dalloc(e, &e->kt, (size_t)8 * KT_SLOT_BLOCKS * 8)); }
    if (e->kt) zero_fill(e, e->kt, (size_t)8 * KT_SLOT_BLOCKS * 8 * 8);
    e->kt_layer = value; drop_graphs(e); return SONIC_OK;
}
static int opt_inject_dev_err(sonic_engine* e, const char*, int value) {      // tests: set (1) / clear (0) the device error word a decode kernel raises when it gives up on an in-kernel wait
    HIPC(e, hipSetDevice(e->device));
    const int v = value ? 1 : 0;
    HIPC(e, hipMemcpyAsync(e->n_active + 1, &v, 4, hipMemcpyHostToDevice, e->st));
    HIPC(e, stream_sync(e));
    return SONIC_OK;
}

// The experiment knobs of sonic_set_option, one row each: the key, where the value lives (a member of the engine, or of its LaunchOpts - common.h
// describes those), whether the captured decode graphs of the engine are dropped (the knob changes the captured kernels), and the clamp of the value.
// A row with `apply` names a function above instead, which does the row's whole job.
struct OptRow { const char* key; int sonic_engine::* field; int LaunchOpts::* lfield; bool drop_graphs; int (*clamp)(int); int (*apply)(sonic_engine*, const char* key, int value); };
#define ENG(m) &sonic_engine::m, nullptr
#define LOP(m) nullptr, &LaunchOpts::m
#define APPLY(f) nullptr, nullptr, false, nullptr, f
static const OptRow OPTIONS[] = {
    {"skinny_variant", LOP(skinny_variant), true, nullptr},
    {"gemm_force128", LOP(gemm_force128), false, nullptr},
    {"no_fused_gu", LOP(no_fused_gu), true, nullptr},
    {"no_fused_gu64", LOP(no_fused_gu64), true, nullptr},
    {"gu64_two_pass", LOP(gu64_two_pass), true, nullptr},
    {"gu64_split_norm", LOP(gu64_split_norm), true, nullptr},
    {"ktrace_wave", LOP(ktrace_wave), true, nullptr},
    {"no_skinny768", LOP(no_skinny768), true, nullptr},
    {"no_skinny48", LOP(no_skinny48), true, nullptr},
    {"o64_16rows", LOP(o64_16rows), true, nullptr},
    {"i8_no_lnq", ENG(opt_i8_no_lnq), false, nullptr},              // int8 encoder: LayerNorm does not quantise its rows (A/B)
    {"i8_no_qkv_fuse", ENG(opt_i8_no_qkv_fuse), false, nullptr},    // int8 encoder: RoPE and V^T as their own passes (A/B)
    {"i8_dbg", ENG(opt_i8_dbg), true, nullptr},                     // timing experiments (wrong results)
    {"i8_no_xq", ENG(opt_i8_no_xq), true, nullptr},
    {"gemm_small_eff", LOP(gemm_small_eff), false, nullptr},
    {"gemm128_shallow", LOP(gemm128_shallow), false, nullptr},
    {"no_skinny_i8_wide", LOP(no_skinny_i8_wide), true, nullptr},
    {"gemm256_stagger", LOP(gemm256_stagger), false, nullptr},
    {"flash_variant", LOP(flash_variant), false, nullptr},
    {"flash_enc", LOP(flash_enc), false, nullptr},                  // 0: rounds 1-4's encoder attention; v > 0: flash_enc_kernel mode v - 1
    {"gemm256_persist", LOP(gemm256_persist), false, nullptr},
    {"gemm256_persist_cus", LOP(gemm256_persist_cus), false, [](int v) { return v > 0 ? v : 256; }},
    {"gemm256_gm", LOP(gemm256_gm), false, [](int v) { return v > 0 ? v : 8; }},   // raster group height of the 256x256 GEMM (experiments)
    {"i8_defer_thr", ENG(opt_i8_defer_thr), false, nullptr},        // int8: outlier lists longer than this go to the dense side product (-1: never)
    {"decode_prefetch", LOP(decode_prefetch), true, nullptr},       // idle-CU weight prefetch (experiment)
    {"decode_attn_occ2", LOP(decode_attn_occ2), true, nullptr},     // decode attention at 128 VGPRs (two blocks per CU can co-reside; A/B)
    {"decode_attn_v1", LOP(decode_attn_v1), true, nullptr},         // round 2's VALU P.V decode attention (A/B)
    {"prefill_taps", ENG(taps_on), false, nullptr},
    {"no_pre_norm", ENG(opt_no_pre_norm), true, nullptr},           // <= 2 rows: standalone add+RMSNorm launches as for more rows (A/B, same bits)
    {"decode_gemv", ENG(opt_decode_gemv), true, nullptr},
    {"f32_synth_bf16", ENG(opt_f32_synth_bf16), false, nullptr},
    {"no_graph", ENG(opt_no_graph), false, nullptr},                // eager decode loop (debugging)
    {"decode_lookahead", ENG(lookahead), false, [](int v) { return v < 1 ? 1 : (v > CHK_MAX_AHEAD ? CHK_MAX_AHEAD : v); }},   // start value (it adapts)
    {"decode_chunk", ENG(opt_decode_chunk), false, [](int v) { return v > 0 ? (v > 64 ? 64 : v) : 1; }},   // token steps per graph launch / early-stop check
    {"prefill_rowmajor", ENG(opt_prefill_rowmajor), false, nullptr},   // prefill GEMMs read the row-major decoder weights (kept only under SONIC_KEEP_ROWMAJOR=1; A/B)
    {"no_rope_tiles", ENG(opt_no_rope_tiles), false, nullptr},      // prefill RoPE + KV append per token (rounds 1-4) instead of per 16-position tile (A/B)
    {"gemm_trace", ENG(opt_gemm_trace), false, nullptr},            // sonic_bench_gemm prints an in-kernel timeline of one launch to stderr
    {"gemm_timing", ENG(opt_gemm_timing), false, nullptr},          // HIP events around every encoder-layer GEMM launch
    {"no_fused_rope", ENG(opt_no_fused_rope), false, nullptr},      // encoder RoPE as its own pass (A/B against the fused epilogue)
    {"no_gelu_lut", ENG(opt_no_gelu_lut), false, nullptr},          // GELU by arithmetic instead of the LDS table (A/B)
    {"token_logprobs", APPLY(opt_token_logprobs)},
    {"top_logprobs", APPLY(opt_top_logprobs)},
    {"gen_repetition_penalty_milli", APPLY(opt_gen)},
    {"gen_no_repeat_ngram_size", APPLY(opt_gen)},
    {"gen_suppress_token", APPLY(opt_gen)},
    {"sampling", APPLY(opt_sampling)},
    {"sampling_fill_milli", APPLY(opt_sampling_fill_milli)},
    {"truncation", APPLY(opt_truncation)},
    {"truncation_fill", APPLY(opt_truncation_fill)},
    {"grammar", APPLY(opt_grammar)},
    {"lm", APPLY(opt_lm)},
    {"lm_weight", APPLY(opt_lm_weight)},
    {"hook_lm_state", APPLY(opt_hook_lm)},
    {"hook_lm_tok", APPLY(opt_hook_lm)},
    {"hook_lm_weight", APPLY(opt_hook_lm)},
    {"request_grammar_begin", APPLY(opt_request_grammar_begin)},
    {"request_grammar", APPLY(opt_request_grammar)},
    {"hook_grammar_state", APPLY(opt_hook_grammar_state)},
    {"hook_grammar_eos", APPLY(opt_hook_grammar_eos)},
    {"request_bias", APPLY(opt_request_bias)},
    {"request_bias_fill", APPLY(opt_request_bias_fill)},
    {"forced_parallel", APPLY(opt_forced_parallel)},
    {"forced_fanout", APPLY(opt_forced_fanout)},
    {"forced_share_prompt", APPLY(opt_forced_share_prompt)},
    {"forced_align", APPLY(opt_forced_align)},
    {"align_head", APPLY(opt_align_head)},
    {"draft_verify", APPLY(opt_draft_verify)},
    {"fetch_stream", APPLY(opt_fetch_stream)},
    {"fp8_weights", APPLY(opt_fp8_weights)},
    {"fp8_chain", APPLY(opt_fp8_chain)},
    {"score_chunk_rows", ENG(opt_score_chunk_rows), false, [](int v) { return v < 16 ? 16 : (v > 4096 ? 4096 : v); }},   // score rows per lm_head GEMM + row-kernel launch (the buffer follows at the next parallel run)
    {"ktrace", APPLY(opt_ktrace)},
    {"inject_dev_err", APPLY(opt_inject_dev_err)},
};
extern "C" int sonic_set_option(sonic_engine* e, const char* key, int value) {
    if (!e || !key) return SONIC_ERR_INVALID;
    if (!strncmp(key, "request_grammar", 15)) {      // as the other per-request setters: refused during an asynchronous run, without waiting for the lock that run holds
        std::lock_guard<std::mutex> ak(e->a_mu);
        if (e->a_pending || e->a_running) return fail(nullptr, SONIC_ERR_INVALID, "%s: an asynchronous run of this handle is in flight", key);
    }
    std::lock_guard<std::mutex> lk(e->mu);
    // knobs live in the engine: two engines in one process do not see each other's settings; captured decode graphs of THIS engine
    // are dropped whenever a knob that changes the captured kernels moves
    for (const OptRow& r : OPTIONS) {
        if (strcmp(key, r.key)) continue;
        if (r.apply) return r.apply(e, key, value);
        const int v = r.clamp ? r.clamp(value) : value;
        if (r.field) e->*r.field = v; else e->opts.*r.lfield = v;
        if (r.drop_graphs) drop_graphs(e);
        return SONIC_OK;
    }
    return fail(e, SONIC_ERR_INVALID, "unknown option %s", key);
}

// The buffers sonic_debug_read serves, one row each: the name, the elements it holds, and where it lives on a 16-bit handle and on the fp32 kind (null: that kind
// has no such buffer).  Rows with an index (n_idx: how many the buffer holds, each `cap` elements): prefill_tap - tap `index` of the taps option prefill_taps
// recorded - and kcache / vcache - decoder layer `index` of the KV cache, [Bm][Hkv][max_ctx][head_dim]
struct DbgRow { const char* name; size_t (*cap)(const sonic_engine*); const bf16_t* (*src16)(const sonic_engine*); const float* (*src32)(const sonic_engine*);
                const float* (*f32_on_16)(const sonic_engine*) = nullptr;         // f32_on_16: a buffer that is fp32 on a 16-bit handle too (read as it is)
                int (*n_idx)(const sonic_engine*) = nullptr; };
#define CAP(x) [](const sonic_engine* e) -> size_t { return x; }
#define S16(m) [](const sonic_engine* e) -> const bf16_t* { return e->m; }
#define S32(m) [](const sonic_engine* e) -> const float* { return e->f->m; }
static const DbgRow DEBUG_BUFS[] = {
    {"prefill_tap", CAP((size_t)e->tok_cap * e->d.dec_d), S16(taps), [](const sonic_engine* e) -> const float* { return (const float*)e->taps; }, nullptr, [](const sonic_engine* e) -> int { return e->d.dec_layers + 1; }},
    {"kcache", CAP((size_t)e->Bm * e->d.dec_kv_heads * e->max_ctx * e->d.dec_head_dim), S16(Kc), nullptr, nullptr, [](const sonic_engine* e) -> int { return e->d.dec_layers; }},
    {"vcache", CAP((size_t)e->Bm * e->d.dec_kv_heads * e->max_ctx * e->d.dec_head_dim), S16(Vc), nullptr, nullptr, [](const sonic_engine* e) -> int { return e->d.dec_layers; }},
    {"pe", CAP((size_t)e->Bm * e->Ta * e->d.dec_d), S16(pe), S32(pe)},
    {"dx", CAP((size_t)e->tok_cap * e->d.dec_d), S16(dx), S32(dx)},
    {"dqkv", CAP((size_t)e->tok_cap * e->qkvN), S16(dqkv), nullptr},
    {"dq", CAP((size_t)e->tok_cap * e->QD), S16(dq), nullptr},
    {"datt", CAP((size_t)e->tok_cap * e->QD), S16(datt), nullptr},
    {"dact", CAP((size_t)e->tok_cap * e->d.dec_ff), S16(dact), nullptr},
    {"enc_x", CAP((size_t)e->Bm * e->T * e->d.enc_d), S16(ln), S32(ln)},
    {"h1", CAP((size_t)e->Bm * (e->d.n_frames + 2) * e->d.enc_d), nullptr, S32(h1)},
    {"shn", CAP((size_t)64 * e->d.dec_d), S16(shn), nullptr},          // decode-step buffers as the last step left them
    {"satt", CAP((size_t)64 * e->QD), S16(satt), nullptr},
    {"sact", CAP((size_t)64 * e->d.dec_ff), S16(sact), nullptr},
    // the last align run: the last selected layer's probabilities [its heads][S][A_max] and M [S][A_max], fp32
    {"align_probs", CAP(e->align_P ? (size_t)e->align_last_heads * e->align_S * e->align_Amax : 0), nullptr, nullptr, [](const sonic_engine* e) -> const float* { return e->align_P; }},
    {"align_matrix", CAP(e->align_M ? (size_t)e->align_S * e->align_Amax : 0), nullptr, nullptr, [](const sonic_engine* e) -> const float* { return e->align_M; }},
};
// Debug read-back of an internal activation buffer as fp32 (tests / diagnostics only).
extern "C" int sonic_debug_read(sonic_engine* e, const char* name, int index, float* out, int64_t n) {
    if (!e || !name || !out) return SONIC_ERR_INVALID;
    ENTER(e);
    if (!strncmp(name, "gemm_", 5)) { const int r = gemm_form_read(e, name, out, n); if (r >= 0) return r; }      // the GEMM form hook's C / Vt and the route witness
    if (!strcmp(name, "hook_grammar_state")) {      // the rows' states behind the last hook launch that took a grammar (host words: exact in fp32)
        if (n < 0 || n > 64) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        for (int64_t i = 0; i < n; ++i) out[i] = (float)e->hook_state_out[i];
        return SONIC_OK;
    }
    if (!strcmp(name, "hook_lm_state") || !strcmp(name, "hook_lm_tok")) {      // the rows' words as the last hook launch left them (exact in fp32: below 2^24)
        if (n < 0 || n > 64 || !e->hook_lm_words) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        int w[128]; HIPC(e, stream_sync(e)); HIPC(e, d2h(e, w, e->hook_lm_words, sizeof w));
        for (int64_t i = 0; i < n; ++i) out[i] = (float)w[(name[8] == 's' ? 0 : 64) + i];
        return SONIC_OK;
    }
    if (!strcmp(name, "hook_lm_add")) {          // the vectors [rows][V] the last \"lm.hook.step\" left
        if (n < 0 || !e->hook_lm_add || (size_t)n > (size_t)e->hook_lm_rows * e->hook_lm_V) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        HIPC(e, stream_sync(e)); if (n > 0) HIPC(e, d2h(e, out, e->hook_lm_add, (size_t)n * 4));
        return SONIC_OK;
    }
    if (!strcmp(name, "hook_truncation")) {         // the rows' records behind the last hook launch that took a truncation: [y of the last kept id | that id | n] (host words; ids and counts exact in fp32)
        if (n < 0 || n > 64 * 3) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        for (int64_t i = 0; i < n; ++i) { if (i % 3 == 0) memcpy(&out[i], &e->hook_trunc_rec[i], 4); else out[i] = (float)(int)e->hook_trunc_rec[i]; }
        return SONIC_OK;
    }
    if (!strcmp(name, "draft_accepted")) {          // a_r of the handle's last prefill (option draft_verify; exact in fp32); zeros behind a prefill without drafts
        if (n < 0 || n > 64) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        if (!e->opt_draft_verify) return fail(e, SONIC_ERR_INVALID, "draft_accepted: option draft_verify is off on this handle");
        int acc[64] = {0};
        if (e->draft_last_S > 0 && e->draft_acc) { HIPC(e, stream_sync(e)); HIPC(e, d2h(e, acc, e->draft_acc, 64 * 4)); }
        for (int64_t i = 0; i < n; ++i) out[i] = (float)acc[i];
        return SONIC_OK;
    }
    if (!strcmp(name, "score_tokens")) {            // the packed tokens of the handle's last parallel forced run, shared prompt or not (exact in fp32: at most tok_cap)
        if (n != 1) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        out[0] = (float)e->score_tokens;
        return SONIC_OK;
    }
    if (!strcmp(name, "fork_ms")) {                 // fork_kv_kernel's time in the handle's last forked prefill, from the events around it; 0 behind an unforked one
        if (n != 1) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        out[0] = 0.f;
        if (e->fork_timed) { HIPC(e, stream_sync(e)); HIPC(e, hipEventElapsedTime(&out[0], e->fork_ev[0], e->fork_ev[1])); }
        return SONIC_OK;
    }
    if (!strcmp(name, "fp8_step_builds")) {         // token steps this handle built in the fp8 form since option fp8_weights was set (exact in fp32 below 2^24)
        if (n != 1) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        out[0] = (float)e->fp8_step_builds;
        return SONIC_OK;
    }
    if (!strcmp(name, "fp8_scales") || !strcmp(name, "fp8_matrix")) {      // mode fp8, matrix `index` (fp8_mat): its rows' scales, or a prefix of its e4m3 copy as fp32 s q, row-major in the tiled copy's row order
        Fp8Mat mt{};
        if (!e->opt_fp8_weights) return fail(e, SONIC_ERR_INVALID, "%s: option fp8_weights is off on this handle", name);
        if (!fp8_mat(e, index, &mt)) return fail(e, SONIC_ERR_INVALID, "index %d out of range for buffer %s (0 .. %d)", index, name, 4 * e->d.dec_layers);
        const bool sc = name[4] == 's';
        if (n < 0 || (size_t)n > (sc ? (size_t)mt.N : (size_t)mt.N * mt.K)) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        if (n == 0) return SONIC_OK;
        if (sc) { HIPC(e, stream_sync(e)); HIPC(e, d2h(e, out, *mt.sc, (size_t)n * 4)); return SONIC_OK; }
        float* tmp = nullptr;
        HIPC(e, hipMalloc((void**)&tmp, (size_t)n * 4));
        launch_fp8_read(*mt.w8, *mt.sc, tmp, mt.K, (long)n, e->st);
        hipError_t r = stream_sync(e);
        if (r == hipSuccess) r = d2h(e, out, tmp, (size_t)n * 4);
        (void)hipFree(tmp);
        HIPC(e, r);
        return SONIC_OK;
    }
    for (const DbgRow& r : DEBUG_BUFS) {
        if (strcmp(name, r.name) || !(e->f32 ? (bool)r.src32 : (r.src16 || r.f32_on_16))) continue;
        const bool tap = &r == &DEBUG_BUFS[0];
        if (tap && !e->taps) return fail(e, SONIC_ERR_INVALID, "no taps recorded");
        if (r.n_idx && (index < 0 || index >= r.n_idx(e))) return fail(e, SONIC_ERR_INVALID, "index %d out of range for buffer %s (0 .. %d)", index, name, r.n_idx(e) - 1);
        const size_t cap = r.cap(e), off = r.n_idx ? (size_t)index * cap : 0;
        if (n < 0 || (size_t)n > cap) return fail(e, SONIC_ERR_INVALID, "read of %lld elements exceeds buffer %s", (long long)n, name);
        if (!e->f32 && r.f32_on_16) { HIPC(e, stream_sync(e)); if (n > 0) HIPC(e, d2h(e, out, r.f32_on_16(e), (size_t)n * 4)); return SONIC_OK; }
        if (!e->f32) return read_back_16(e, r.src16(e) + off, out, (size_t)n);
        HIPC(e, stream_sync(e)); HIPC(e, d2h(e, out, r.src32(e) + off, (size_t)n * 4));      // fp32 kind: its buffers are fp32 already
        return SONIC_OK;
    }
    return fail(e, SONIC_ERR_INVALID, "unknown buffer %s", name);
}

extern "C" int sonic_debug_ktrace(sonic_engine* e, int64_t* out, int64_t n) {
    if (!e || !out) return SONIC_ERR_INVALID;
    ENTER(e);
    if (!e->kt) return fail(e, SONIC_ERR_INVALID, "ktrace is off");
    const int64_t have = (int64_t)8 * KT_SLOT_BLOCKS * 8;
    HIPC(e, stream_sync(e));
    HIPC(e, d2h(e, out, e->kt, (size_t)(n < have ? n : have) * 8));
    return SONIC_OK;
}
