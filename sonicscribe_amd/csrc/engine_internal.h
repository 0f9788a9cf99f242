// What the translation units of the engine (engine.cpp, engine_generation.cpp, engine_weights.cpp, engine_stages.cpp, engine_decode.cpp, engine_score.cpp, engine_f32.cpp,
// engine_ingest.cpp, engine_service.cpp, engine_options.cpp, engine_hooks.cpp) share: the engine struct and its parts, the constants, the error / entry macros and the helpers that
// cross a unit boundary.  Not part of the C ABI (include/sonic_hip.h); a function used by one unit only is static there.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sonic_hip.h"
#include "sched_engine.h"      // what dispatch.cpp and pipeline.cpp call: declared once, seen by the definitions
#include "common.h"
#include "kernels.h"

#define T_PAD_ALIGN 64
#define CHK_RING 64            // check events / pinned n_active words of the decode loop
#define DEV_ERR_ACTIVE (-(1 << 23))   // a running-row count below this: the device error word was set (greedy_kernel), the step's outputs are invalid
#define SVC_WORDS 132           // per check of the continuous loop: finished[64], n_new[64], n_active, padding
#define SCORE_CHUNK_DEFAULT 256   // score rows per lm_head GEMM + row-kernel launch of the parallel forced run (option score_chunk_rows; DESIGN.md 6.8 says why)
#define CHK_MAX_AHEAD 32       // deepest lookahead in chunks (a host that is frozen for tens of ms at a time - CPU quota, a busy event loop)

struct DevTensor {
    std::vector<int64_t> shape;
    bf16_t* p = nullptr;
    size_t n = 0;
};

// int8 mode (asr.py:169-210): a quantised Linear keeps row-wise int8 weights + row absmax instead of its 16-bit matrix
struct QW { int8_t* cb = nullptr; float* scb = nullptr; int8_t* cbt = nullptr; int8_t* cbk = nullptr; bool cb_rowmajor_kept = true; };   // cbt: fragment-tiled copy, cbk: k-major copy (decode step)
struct EncLayerW { float *ln1w, *ln1b, *bqkv, *bo, *ln2w, *ln2b, *b1, *b2; bf16_t *wqkv, *wo, *w1, *w2; QW qqkv, qo, q1, q2; };
#define KT_SLOT_BLOCKS 512                                   // "ktrace" diagnostics: blocks recorded per kernel slot, 8 timestamps each
struct DecLayerW { float *ln1, *ln2; bf16_t *wqkv, *wo, *wgu, *wdown;          // row-major (prefill GEMM)
                   bf16_t *wqkv_t, *wo_t, *wgu_t, *wgu_t8, *wdown_t;                    // fragment-tiled copies (decode skinny GEMM)
                   QW qqkv, qo, qgu, qdown;
                   // mode fp8 (option fp8_weights): the e4m3 copies beside the bf16 tiles (gu8: of wgu_t8, or of wgu_t where that is the layer's copy) and the rows' scales [N]
                   unsigned char *qkv8 = nullptr, *o8 = nullptr, *gu8 = nullptr, *down8 = nullptr; float *qkv_sc = nullptr, *o_sc = nullptr, *gu_sc = nullptr, *down_sc = nullptr; };

// SONIC_MODE_F32 (test only, f32kind.hip): fp32 weights as loaded (torch Linear layout, nothing packed but the conv taps) and fp32 activation buffers
struct F32EncL { float *ln1w, *ln1b, *wq, *bq, *wk, *wv, *bv, *wo, *bo, *ln2w, *ln2b, *w1, *b1, *w2, *b2; };
struct F32DecL { float *ln1, *wq, *wk, *wv, *wo, *ln2, *wg, *wu, *wd; };
struct F32State {
    std::map<std::string, float*> raw;               // name -> device tensor (owned by the engine's alloc list)
    float *conv1w = nullptr, *conv1b = nullptr, *conv2w = nullptr, *conv2b = nullptr, *enc_nw = nullptr, *enc_nb = nullptr;
    float *pj1w = nullptr, *pj1b = nullptr, *pj2w = nullptr, *pj2b = nullptr, *embed = nullptr, *dec_nw = nullptr;
    std::vector<F32EncL> enc; std::vector<F32DecL> dec;
    // encoder: time-major padded features, conv1 output (padded), residual stream, norm output, q / k / v, attention output, MLP, projector
    float *featT = nullptr, *h1 = nullptr, *x = nullptr, *ln = nullptr, *q = nullptr, *k = nullptr, *v = nullptr, *att = nullptr, *ff = nullptr, *ph = nullptr, *pe = nullptr;
    // decoder: token rows of the prefill (or the R rows of a token step), KV cache [layer][seq][ctx][KD], logits [64][vocab]
    float *dx = nullptr, *dhn = nullptr, *dq = nullptr, *dk = nullptr, *dv = nullptr, *datt = nullptr, *dg = nullptr, *du = nullptr, *dact = nullptr;
    float *Kc = nullptr, *Vc = nullptr, *logits = nullptr, *hlast = nullptr;
};

// resampler bank of one rate pair (engine_resample.cpp): built in double on the host, rounded once to fp32, k-major on the device
struct RsBank { float* dev = nullptr; int of = 0, nf = 0, width = 0, K = 0, tile = 0, kc = 0; };
#define RS_BANK_MAX_COEF ((int64_t)1 << 22)

// Values the caller leaves for the requests of the next prefill (options request_bias and sampling; the protocol is stage_* in engine_generation.cpp, which also holds the one list of the stages: req_*).  dev: the rows'
// words on the device, written by the prefill from the pinned mirror `host`, copied by the splice.  pending: the R of the values a setter left in `host` for the
// next prefill (-1: none); take: that prefill is under way and uploads them.  ev / busy: the last upload's copies out of `host` are older than this event.
template <typename W> struct ReqStage {
    W* dev = nullptr; W* host = nullptr; hipEvent_t ev = nullptr; bool busy = false;
    std::atomic<int> pending{-1}; bool take = false;
    int claim() { take = false; return pending.exchange(-1); }      // run_to_first_token: this batch consumes what is pending whatever becomes of it
};
// A grammar (sonic_load_tensor "grammar:<id>"): a deterministic token automaton on the device, created on a weight owner and shared by all of its handles.
// dev: GRAM_HEAD words (N, E), node_off[N + 1], edge_tok[E], edge_next[E] (kernels.h GreedyArgs.gram_ref).  refs: the requests that refer to it - staged
// (option request_grammar, a dispatcher's queue) or on a row; the destroy refuses while it is above zero
struct sonic_grammar { sonic_engine* root = nullptr; int id = 0; int* dev = nullptr; int N = 0, E = 0; int64_t bytes = 0; std::atomic<int> refs{0}; };
// A language model (sonic_load_tensor "lm:<id>"): a backoff n-gram automaton on the device, created on a weight owner and shared by all of its handles.
// dev: LM_HEAD words, then the arrays as lm_step_kernel reads them (kernels.h LmArgs).  refs: the handles whose option lm names it; the destroy refuses while it is above zero
struct sonic_lm { sonic_engine* root = nullptr; int id = 0; int* dev = nullptr; int V = 0, N = 0, E = 0, order = 0, start = 0; int64_t bytes = 0; std::atomic<int> refs{0}; };
struct sonic_engine {
    sonic_dims d;
    int device = 0, mode = 0, Bm = 0, max_ctx = 0;
    int dt = DT_BF16;          // activation / 16-bit weight element type: bf16 (native) or fp16 (int8 mode, asr.py:61)
    bool i8 = false;           // LLM.int8 linears
    bool f32 = false;          // SONIC_MODE_F32: the fp32 kind of every stage (test only; F32State, f32kind.hip)
    F32State* f = nullptr;
    hipStream_t st = nullptr;
    std::mutex mu;
    std::string err;
    std::vector<void*> allocs;
    bool cap_svc = false;                           // a continuous loop's chunk graph is being captured (chunk_graph)
    int64_t weight_bytes = 0, alloc_bytes = 0;      // alloc_bytes: every live device allocation of this engine (sonic_memory_info)
    bool finalized = false;

    std::map<std::string, DevTensor> raw;
    // packed weights
    bf16_t *conv1w = nullptr, *conv2w = nullptr; float *conv1b = nullptr, *conv2b = nullptr;
    std::vector<EncLayerW> enc;
    float *enc_nw = nullptr, *enc_nb = nullptr;
    unsigned short* gelu_lut = nullptr;     // bf16 GELU table (gemm256 EPI_BIAS_GELU epilogue), native mode
    bf16_t *pj1w = nullptr, *pj2w = nullptr; float *pj1b = nullptr, *pj2b = nullptr; QW qpj1, qpj2;
    // int8 mode scratch: quantised activations of the GEMM in flight, row statistics, outlier columns per request, window -> request map
    int8_t* qa = nullptr; float* q_sca = nullptr; unsigned char* q_flags = nullptr; int *q_oc_cnt = nullptr, *q_oc_list = nullptr, *win_req = nullptr;
    int q_kmax = 0; bf16_t* qkv_rm = nullptr;
    bf16_t* defer_tmp = nullptr; size_t defer_cap = 0; int opt_i8_defer_thr = 8; int opt_i8_no_xq = 0; int opt_i8_no_lnq = 0; int opt_i8_dbg = 0; int opt_i8_no_qkv_fuse = 0;   // rows deferred to the outlier side product leave the GEMM here
    // int8 decode step: the three quantised row sets (input norm output, attention output, SwiGLU output)
    int8_t *hn_q = nullptr, *att_q = nullptr, *act_q = nullptr; float *sca_hn = nullptr, *sca_att = nullptr, *sca_act = nullptr;
    int *oc_hn = nullptr, *oc_att = nullptr, *oc_act = nullptr, *ol_hn = nullptr, *ol_att = nullptr, *ol_act = nullptr;
    float *ov_hn = nullptr, *ov_att = nullptr, *ov_act = nullptr;      // the outliers' values beside the lists
    int* big_att = nullptr;                                             // [64][4] per-block counts of attention outputs >= 6.0
    float *amax_att = nullptr, *amax_act = nullptr;                     // [64][4] partial row maxima written by producers that do not own whole rows
    std::map<std::string, bool> raw_f16;   // int8 mode: tensors already converted to fp16 at load
    bf16_t* embed = nullptr; bf16_t* embed_t = nullptr;
    std::vector<DecLayerW> dec;
    float* dec_nw = nullptr;

    // derived sizes
    int T = 0, Tp = 0, Ta = 0, hd_e = 0, qkvN = 0, QD = 0, KD = 0, tok_cap = 0, out_cap = 0;
    long slabN = 0;

    // front-end
    int16_t* pcm = nullptr; int* n_samples_d = nullptr; std::vector<int> n_samples_h; int W = 0;
    float* logspec = nullptr; int* segmax = nullptr; bf16_t* feats_fm = nullptr; float* feats_f32 = nullptr;
    LogmelConst lc{};
    // encoder
    bf16_t *h1 = nullptr, *x = nullptr, *ln = nullptr, *qk = nullptr, *vt = nullptr, *att = nullptr, *ff = nullptr, *ph = nullptr, *pe = nullptr;
    float* enc_cs = nullptr;
    // decoder
    bf16_t *dx = nullptr, *dhn = nullptr, *dqkv = nullptr, *dq = nullptr, *datt = nullptr, *dact = nullptr;
    bf16_t *Kc = nullptr, *Vc = nullptr, *Vts = nullptr;
    float* dec_cs = nullptr;
    float *slab = nullptr, *lslab = nullptr, *ssq = nullptr;
    float* slab2 = nullptr;                                         // down_proj's slabs when the next q|k|v (or the lm_head) consumes them itself (PRE form, <= 2 rows)
    bf16_t *sx = nullptr, *shn = nullptr, *sq = nullptr, *satt = nullptr, *sact = nullptr;
    bf16_t* sx2 = nullptr;                                          // ... and the second residual buffer of that form (the stream ping-pongs layer by layer)
    int *kv_len = nullptr, *tok_pos = nullptr, *n_new = nullptr, *finished = nullptr, *max_new_d = nullptr, *n_active = nullptr;
    int *out_ids = nullptr, *step_ctr = nullptr, *seq_iota = nullptr;
    float* out_lp = nullptr;                                        // [64][out_cap][lp_width] log-probability of every emitted token, beside out_ids (option token_logprobs; lp_alloc);
                                                                    // with option top_logprobs = K the token's record is 1 + 2K floats (lp_width)
    int *src = nullptr, *tok_seq = nullptr, *tok_pos_pf = nullptr, *q_off = nullptr, *q_len = nullptr, *last_row = nullptr;
    float* dump = nullptr; size_t dump_cap = 0; int dump_steps = 0;
    bf16_t* taps = nullptr; int taps_on = 0; int last_ntok = 0;   // debug: prefill hidden states after embedding + each layer
    int* n_active_h = nullptr;  // pinned
    int R = 0, max_steps = 0, greedy_calls = 0, steps_run = 0; bool run_logits = false;   // state of the staged batch between the stage entry points
    int* force_d = nullptr; int force_ld = 0, force_R = 0;   // teacher forcing for the next runs (sonic_set_forced_ids)
    std::vector<int> force_h;                                // ... and the host's copy of those ids: the parallel forced run plans from them
    std::vector<int> last_qlen, last_maxnew;
    std::map<std::pair<int, int>, hipGraphExec_t> graphs;        // (rows, token steps) -> captured chunk of the decode loop
    // the pipelined early-stop check: behind every chunk the device's count of running rows is copied to n_active_h[chunk % CHK_RING] and an
    // event is recorded; the host reads check k only when chunk k + lookahead is already queued (run_decode_steps)
    hipEvent_t chk_ev[CHK_RING]{};
    bool run_starved = false;                                      // the current batch saw the queue run dry (lookahead grew)
    int lookahead = 1;                                             // chunks queued beyond the one whose check the host waits for; adapts (1..CHK_MAX_AHEAD)
    int* plan_h = nullptr; size_t plan_cap = 0;                    // pinned staging of a batch's prompt plan (no stream synchronise between encoder and prefill)
    // Two staging buffers used alternately, each with an event recorded behind the last copy that reads it: sonic_prefill_enqueue returns with those
    // copies still queued behind the encoder, and the next run on this handle must not overwrite a buffer the stream has not read yet
    int* plan_buf[2] = {nullptr, nullptr}; hipEvent_t plan_ev[2] = {nullptr, nullptr}; bool plan_busy[2] = {false, false}; int plan_idx = 0;

    // Slots (sonic_slot_create): further in-flight batches on ONE weight copy.  A slot is an engine of its own in every respect - stream, activation
    // buffers, KV cache, PCM staging, decode graphs, lock, options - except that its weight / constant pointers are the owner's.
    sonic_engine* owner = nullptr;                                 // slot: whose weights these are (never a slot itself)
    std::vector<sonic_engine*> slots;                              // owner: its slots (destroyed with it at the latest)
    std::mutex rings_mu;                                           // owner: guards `rings` (the registry every slot stages from)

    // continuous decoding (sonic_service_*): this engine's rows are a pool - requests prefilled on another handle of the same weights are spliced
    // into free rows between chunks of an endless greedy loop, finished rows are fetched and freed one by one
    bool svc_on = false;
    int64_t svc_launched = 0, svc_checked = 0;                     // chunks queued / checks read since sonic_service_begin
    int64_t svc_dry = 0;                                           // launches that found the stream empty with rows running (diagnostics)
    int svc_calm = 0;                                              // chunks since the queue last ran dry (the lookahead shrinks again after 256 of them)
    int* svc_h = nullptr;                                          // pinned ring [CHK_RING][SVC_WORDS]: finished[64] | n_new[64] | n_active
    int svc_fin[64]{}, svc_nn[64]{}, svc_active = 0; int64_t svc_seq = 0;   // the newest check read: state after chunk number svc_seq
    hipEvent_t sync_ev = nullptr;                                  // blocking-sync event behind stream_sync()
    // the finished rows' mirror: the kernel behind every chunk (service_status_kernel) copies a row's ids (and log-probability records) into pinned host
    // memory in the chunk that finds it finished, so a fetch is a memcpy behind the check's event - no copy command, no stream, no wait
    int* svc_out_h = nullptr;                                      // pinned [64][out_cap], allocated by the first sonic_service_begin
    float* svc_lp_h = nullptr; int svc_lp_w = 0;                   // pinned [64][out_cap * lp_width] (option token_logprobs), for records svc_lp_w floats wide
    int* mirrored = nullptr;                                       // device [64]: the row's tokens are in the mirror (cleared by a splice; free rows: 1)
    int64_t spliced_seq[64]{};                                     // chunks queued before the row's last splice: its mirror is valid once svc_seq is larger and svc_fin[row]
    int opt_fetch_stream = 0;                                      // 1 (A/B): no mirror; rows are fetched by copy commands on a stream of their own, as before the mirror
    hipStream_t st_io = nullptr;                                   // ... that stream, created by the first sonic_service_begin with fetch_stream = 1 (the default path owns ONE stream per handle)
    hipEvent_t xfer_ev = nullptr, splice_ev = nullptr, wait_ev = nullptr; bool wait_pending = false;   // cross-handle ordering of a splice

    // sonic_run_staged_async / sonic_wait: a worker thread of the engine's own runs the batch, the caller's thread returns at once
    struct AsyncJob { std::vector<int32_t> req_win, prompt_ids, max_new; std::vector<int64_t> prompt_off; int R = 0; bool has_rw = false; int want_logits = 0; } a_job;
    std::thread a_thread; std::mutex a_mu; std::condition_variable a_cv;
    bool a_started = false, a_pending = false, a_running = false, a_done = false, a_stop = false; int a_status = 0;

    // experiment knobs (sonic_set_option): per engine, copied into the launchers' thread-local view by ENTER()
    LaunchOpts opts;
    int opt_no_graph = 0, opt_gemm_timing = 0, opt_no_fused_rope = 0, opt_no_gelu_lut = 0, opt_gemm_trace = 0, opt_no_rope_tiles = 0, opt_prefill_rowmajor = 0;
    double host_launch_ms = 0, host_wait_ms = 0; int host_launches = 0;   // host time of the last run's decode loop: inside hipGraphLaunch / waiting for a check
    int step_launches_per_layer = 0;   // of the token step built last (decode_step): sonic_timings.decode_launches_per_layer
    int opt_f32_synth_bf16 = 0;    // SONIC_MODE_F32: sonic_load_synthetic writes the bf16-rounded values (the weights a bf16 engine gets from the same seed) as fp32
    int opt_decode_gemv = 0;       // 1: token steps of <= 4 rows run the GEMV chain (gemv.hip: five launches per layer, no MFMA tiles); opt-in - another summation order than the
                                   // MFMA chain, so a request's low bits then depend on whether its step had <= 4 rows.  Measured slower than the MFMA chain (profiles/round6_gemv_ab.txt): an experiment, off
    // mode fp8.  opt_fp8_weights: the owner's decoder matrices and embedding were snapped onto their e4m3 grids in place (W'), the e4m3 copies exist
    // (DecLayerW, embed8 / embed_sc) - set once on a bf16 owner before its slots exist (they copy both values and share the copies), never cleared.  opt_fp8_chain
    // (switched on with it; the A/B): token steps of <= 4 rows stream the e4m3 copies (gemv_fp8.hip) where every shape is eligible - the bits of the bf16 GEMV chain
    // on W', i.e. decode_gemv's caveat: another summation order than the MFMA chain.  fp8_step_builds: token steps this handle built in that form since the option was set
    int opt_fp8_weights = 0, opt_fp8_chain = 0; int64_t fp8_step_builds = 0;
    unsigned char* embed8 = nullptr; float* embed_sc = nullptr;
    int opt_no_pre_norm = 0;       // 1: never the PRE form of the <= 2-row decode step (standalone add+RMSNorm launches as for more rows; A/B - same bits)
    int opt_decode_chunk = 2;      // token steps per captured graph = granularity of the early-stop check (sonic_set_option "decode_chunk")
    int opt_token_logprobs = 0;    // 1: every greedy launch also writes log_softmax(logits)[token] to out_lp (greedy_kernel<T, true>); set on the owner before
                                   // its slots exist (they copy it).  The decode loops keep their hipGraph form; graphs are cached per value
    int opt_top_logprobs = 0;      // K in 0 .. 8: every greedy launch also writes the step's K best ids and their log-probabilities (greedy_kernel<T, true, ., ., ., true>);
                                   // set on the owner, after token_logprobs, before its slots exist (they copy it); out_lp then holds 1 + 2K floats per token (top_enable)
    // generation guards (sonic_set_generation; greedy_kernel<T, LP, true>): HF's repetition_penalty / no_repeat_ngram_size / suppress_tokens inside the greedy
    // kernel.  gen_on: any of them is set; set on the owner before its slots exist (they copy it).  hist[64][max_ctx]: every row's input_ids (prompt, then the emitted ids),
    // written by the prefill and the greedy kernel, copied by the splice; allocated with gen_suppress_d[256] by the first gen_apply that switches a guard on
    bool gen_on = false; float gen_penalty = 1.0f; int gen_ngram = 0; std::vector<int> gen_suppress;
    int* hist = nullptr; int* gen_suppress_d = nullptr;
    // option request_bias (sonic_set_request_bias; greedy_kernel<T, LP, true, true>): every row's own table, bias.dev[BIAS_TAB_WORDS] (kernels.h); allocated, with hist, by the option
    int opt_request_bias = 0;
    int opt_bias_fill = 0;         // measurement aid (option request_bias_fill, tools/ab_request_bias.sh): a prefill that was given no tables writes this many neutral entries per request
    ReqStage<int> bias;
    // option sampling (sonic_set_request_sampling; greedy_kernel<T, true, ., ., true>): every row's temperature bits and seed words, samp.dev[SAMP_WORDS] (kernels.h); allocated by the option
    int opt_sampling = 0;
    int opt_samp_fill_milli = 0;   // measurement aid (option sampling_fill_milli, tools/ab_sampling.sh): a prefill that was given no values decodes request r at this temperature (in thousandths) with seed r
    ReqStage<unsigned> samp;
    // option truncation (sonic_load_tensor "request_truncation"; greedy_kernel<T, true, ., ., true, ., ., true>): every row's top_k, top_p bits and lnm bits,
    // trunc.dev[TRUNC_STAGE_WORDS] (kernels.h); allocated by the option, which needs option sampling.  opt_trunc_fill: measurement aid (option truncation_fill,
    // tools/ab_truncation.sh): a prefill that was given no values decodes every request with top_k = 50, top_p = 0.9
    int opt_truncation = 0, opt_trunc_fill = 0;
    ReqStage<unsigned> trunc;
    // the kernel hooks' truncation (sonic_load_tensor "truncation.hook", float32 [B][3]): armed until the next sonic_test_greedy_sample launch takes it; hook_trunc_rec:
    // that launch's records (sonic_debug_read "hook_truncation")
    std::vector<unsigned> hook_trunc; unsigned hook_trunc_rec[64 * 3]{};
    // option grammar (options request_grammar_begin / request_grammar; greedy_kernel<T, true, true, ., ., ., true>): gram.dev holds GRAM_STAGE_WORDS 64-bit words - the 64
    // rows' grammar references (device addresses; 0: a free row), then their 64 state words (int: -1 free, n >= 0 a node, -2 left); allocated, with hist, by the
    // option.  gram_staged / gram_row: the references (sonic_grammar::refs) the staged requests and the rows of this handle hold - taken by the setter, moved to the
    // rows by the prefill, copied by the splice, dropped when a row is fetched, overwritten by the next prefill or goes with the handle.
    // Owner only: `grammars`, the registry (guarded by gram_mu; freed with the owner at the latest), and gram_bytes, their device bytes (part of sonic_memory_info)
    int opt_grammar = 0;
    ReqStage<unsigned long long> gram;
    sonic_grammar* gram_staged[64]{}; sonic_grammar* gram_row[64]{};
    std::mutex gram_mu; std::vector<sonic_grammar*> grammars; std::atomic<int64_t> gram_bytes{0};
    // the kernel hooks' grammar (sonic_load_tensor "grammar.hook:<V>", options hook_grammar_state / hook_grammar_eos; engine_hooks.cpp): the packed automaton, the rows'
    // states in, the EOS ids, armed until the next hook launch that has histories and log-probabilities takes it; hook_state_out: that launch's states out (sonic_debug_read)
    std::vector<int> hook_gram; int hook_state_in[64]; std::vector<int> hook_eos; int hook_state_out[64]{};
    // option lm / lm_weight (lm_step_kernel + greedy_kernel<T, true, true, ., ., ., false, ., true>): shallow fusion with the n-gram model `lm` of the weight
    // owner (a reference, sonic_lm::refs) at weight lm_weight.  lm_words[128]: the rows' state words, then their pending tokens (-1: none); lm_add[max_batch][vocab] fp32:
    // the rows' vectors, rebuilt every step.  Both come, with hist, with the option's first use, are counted by sonic_memory_info and go with the handle.  An option of
    // the handle, not a value of a request: nothing is staged.  Owner only: `lms`, the registry (guarded by gram_mu, freed with the owner at the latest)
    int opt_lm = 0; float lm_weight = 0.f; sonic_lm* lm = nullptr; int* lm_words = nullptr; float* lm_add = nullptr;
    std::vector<sonic_lm*> lms;
    std::vector<float> hook_form[7];      // the GEMM form hook's host buffers A, W, bias, resid, rope, C, Vt (sonic_load_tensor "gemm.form:<buffer>"; engine_hooks.cpp)
    // the kernel hooks' language model (sonic_load_tensor "lm.hook:<V>", options hook_lm_state / hook_lm_tok / hook_lm_weight; engine_hooks.cpp): the device blob in lm_step_kernel's
    // layout, the rows' words in (host) and out (device, [state 64 | tok 64]) and the vector [64][V] the last "lm.hook.step" left: the greedy hooks that have histories and
    // log-probabilities take it while it is armed
    int* hook_lm = nullptr; size_t hook_lm_cap = 0; int hook_lm_V = 0, hook_lm_N = 0; int hook_lm_in[128]; float hook_lm_weight = 0.f; int* hook_lm_words = nullptr; float* hook_lm_add = nullptr; size_t hook_lm_add_cap = 0; int hook_lm_rows = 0;
    // the parallel forced run (options forced_parallel / forced_fanout / score_chunk_rows; run_forced_parallel, engine_score.cpp): with forced ids set,
    // a run is ONE prefill of prompt || forced ids, the lm_head over every forced position as a GEMM per chunk of score rows, and rows_kernel (rows.hip) per row.
    // score_logits: the chunk's logits [score_rows_cap][vocab] in the activation type (fp32 kind: fp32); score_plan_d / score_plan_h: the score rows' plan (ScorePlan),
    // on the device and in pinned memory (one buffer: the run ends with a stream synchronise).  All three come with the first parallel run, are counted by
    // sonic_memory_info and go with the handle
    int opt_forced_parallel = 0, opt_forced_fanout = 1, opt_score_chunk_rows = SCORE_CHUNK_DEFAULT;
    void* score_logits = nullptr; int score_rows_cap = 0; int* score_plan_d = nullptr; int* score_plan_h = nullptr;
    // option forced_share_prompt: the candidates of one audio share ONE prefill of their prompt.  pre_row [2][64]: the sequences' pre_row | pre_len on
    // the device (with the handle's first shared run); score_tokens: the packed tokens of the last parallel forced run (sonic_debug_read "score_tokens"); hook_share: the
    // kernel hook's pre_row | pre_len (sonic_load_tensor "share_prompt.hook"), armed until the next sonic_test_prefill_attention takes it
    int opt_forced_share_prompt = 0; int* pre_row = nullptr; int score_tokens = 0; std::vector<int> hook_share;
    // word timestamps on the parallel forced run (options forced_align / align_head; align.hip).  align_heads: the selected heads as l * 256 + h, sorted
    // (empty: every head of the last ceil(dec_layers / 2) layers).  The buffers come with the first align run, sized to that run (and exchanged for larger ones by a
    // later run that needs more), are counted by sonic_memory_info and go with the handle: align_P 2 x [heads of a layer][S][A_max] and align_M [S][A_max] fp32, the DTW's
    // int8 trace [S][A_max], align_t [64][out_cap] (t_n beside out_lp's records), the plan (AlignPlan) on the device and pinned.  align_live: the prefill under way is an
    // align run's (run_prefill launches align_probs / _reduce behind the selected layers' RoPE); align_last: the batch in hand is one - its log-probability records
    // carry t_n as one more float (fetch_locked)
    int opt_forced_align = 0; std::vector<int> align_heads;
    float *align_P = nullptr, *align_M = nullptr, *align_t = nullptr; signed char* align_trace = nullptr; int *align_plan_d = nullptr, *align_plan_h = nullptr;
    size_t align_P_cap = 0, align_M_cap = 0, align_plan_cap = 0, align_Zoff = 0;      // align_P holds the probabilities and, align_Zoff floats on, the filtered z of one layer's heads
    bool align_live = false, align_last = false;
    int align_S = 0, align_nseq = 0, align_Amax = 0, align_Lmax = 0, align_Htot = 0, align_last_heads = 0;      // of the run under way / the last one
    std::vector<std::vector<int>> align_layer_heads; std::vector<int> align_layer_off;                             // per decoder layer: its selected heads, and where they start in the plan
    // draft-verified decoding (option draft_verify; sonic_load_tensor "request_draft"; rows.hip): a request of the next prefill may bring a draft of its
    // transcript - the prefill runs over prompt || draft, the lm_head over every draft position as a GEMM per chunk of rows into score_logits (the parallel forced
    // run's chunk buffer), rows_kernel per row, draft_accept_kernel per request, then the unchanged head.  draft_stage: the staged words [R | off[R + 1] | ids]
    // (draft_pending = their R, -1: none; draft_take: the prefill under way consumes them).  The buffers come with the handle's first drafted prefill, are counted by
    // sonic_memory_info and go with the handle: draft_plan_d, the verify rows' plan (DraftPlan), with a pinned mirror beside each of the two plan staging buffers; ver_tok
    // [tok_cap], ver_rec [tok_cap][lp_width] (ver_rec_w: the width it was allocated at), draft_acc [64] = a_r of the last drafted prefill (draft_last_S: its verify rows; 0: none)
    int opt_draft_verify = 0;
    std::vector<int> draft_stage; std::atomic<int> draft_pending{-1}; bool draft_take = false;
    int* draft_plan_d = nullptr; int* draft_plan_h[2] = {nullptr, nullptr}; int* ver_tok = nullptr; float* ver_rec = nullptr; int ver_rec_w = 0; int* draft_acc = nullptr;
    int draft_last_S = 0;
    // row forks (sonic_load_tensor "request_forks"; fork.hip): request a of the next prefill becomes fork_stage[a] >= 1 rows that share its prefill -
    // the sources are rows 0 .. A-1, the further forks follow behind them request by request; fork_kv_kernel copies a source's K / V (and history) to its forks behind
    // the last decoder layer, the head then runs over all the rows.  fork_pending = the staged A (-1: none), claimed and dropped as a draft is; no option, no buffer.
    // fork_ev: the kernel's bracket in the last forked prefill (fork_timed; sonic_debug_read "fork_ms")
    std::vector<int> fork_stage; std::atomic<int> fork_pending{-1};
    hipEvent_t fork_ev[2] = {nullptr, nullptr}; bool fork_timed = false;
    uint64_t spliced = 0;          // rows of the last prefill that sonic_splice_rows handed to a continuous loop (bit r = request r); cleared by every prefill (gen_busy)
    long long* kt = nullptr; int kt_layer = -1;     // diagnostics ("ktrace" option): in-kernel timestamps of one decoder layer's kernels
    int* ring_peak = nullptr;                        // [Bm] per-request max |s| of a ring-staged batch (ingest.hip)
    std::atomic<int64_t> ring_bytes{0};             // owner: device bytes of those rings (part of sonic_memory_info of the owner)
    std::vector<struct sonic_ring*> rings;          // rings created on this engine and not yet destroyed (freed with the engine at the latest)
    // resampler (owner only; engine_resample.cpp): the banks every rate ring and every slot share, and sonic_resample's own lock, stream and buffers
    std::mutex rs_mu;                               // guards everything below; never taken together with `mu` by sonic_resample
    std::map<std::pair<int, int>, RsBank> rs_banks; // (of, nf) -> bank; bytes counted in ring_bytes
    hipStream_t rs_st = nullptr; void* rs_in = nullptr; float* rs_out = nullptr; size_t rs_in_cap = 0, rs_out_cap = 0;

    // timing
    hipEvent_t ev[5]{};
    std::vector<hipEvent_t> gemm_ev;
    int gemm_ev_used = 0;
    sonic_timings tim{};
};

// Rows -> reference-call groups for LLM.int8's outlier columns: group of row r = gmap ? gmap[r / gdiv] : r / gdiv, G groups
struct QGroup { const int* gmap; int gdiv; int G; };
// the encoder's fused q|k|v linear in int8 mode: where V^T goes when the 256x256 kernel can take the whole epilogue (RoPE on q / k on the way out
// of the staged tile, V transposed while staging)
struct QkvVt { bf16_t* Vt; int n_split, seg_T, vt_ld; long vt_seg_stride; };

struct HostPlan {
    std::vector<int> src, tok_seq, tok_pos, q_off, q_len, last_row, max_new;
    int n_tok = 0, max_p = 0, max_steps = 0;
    // option forced_share_prompt (empty otherwise): q_len then counts a sequence's PACKED rows (a sharer's: its suffix alone, at positions from its
    // group's prompt length on), kv_len its keys, and keys [0, pre_len) of a sequence are those of cache row pre_row
    std::vector<int> kv_len, pre_row, pre_len;
    // option draft_verify: the S verify rows of the batch's drafts (draft_plan_d's layout: DraftPlan); S = 0: an ordinary prefill
    std::vector<int> draft; int S = 0;
    // row forks: the rows of the run (0: the requests are the rows), then per row the request it shares its prefill with (rows 0 .. R-1: themselves)
    int rows = 0; std::vector<int> fork_src;
};

// The three plans of the scoring passes, as the kernels read them: a view over a base pointer - the pinned host image and the device buffer alike - with one
// member per array.  PLAN_REQ_WORDS: the stride of every per-request array in them; rows.hip and align.hip index rq[64 + r], so it is 64
#define PLAN_REQ_WORDS 64
static_assert(PLAN_REQ_WORDS == 64, "the kernels read the plans' per-request words at a stride of 64");
// draft plan (draft_plan_d / draft_plan_h, HostPlan::draft): per verify row its hidden row | draft id | record index | request | history length, S of each; then per
// request D | first verify row | P | first packed token (req: the four of them as draft_accept_kernel takes them, one pointer)
struct DraftPlan {
    int *hidden, *target, *rec, *hrow, *hlen, *req, *dlen, *first, *P, *q_off;
    DraftPlan(int* b, size_t S) : hidden(b), target(b + S), rec(b + 2 * S), hrow(b + 3 * S), hlen(b + 4 * S), req(b + 5 * S), dlen(req), first(req + PLAN_REQ_WORDS), P(req + 2 * PLAN_REQ_WORDS), q_off(req + 3 * PLAN_REQ_WORDS) {}
    static size_t words(size_t tok_cap) { return 5 * tok_cap + 4 * PLAN_REQ_WORDS; }
};
// score plan (score_plan_d / score_plan_h): per score row its hidden-state row | target | record index, S of each (row_words; all the device buffer holds); then, in
// the host image, the rows' closing state n_new | finished | tok_pos | n_active (state_words)
struct ScorePlan {
    int *hidden, *target, *rec, *n_new, *finished, *tok_pos, *n_active;
    ScorePlan(int* b, size_t S) : hidden(b), target(b + S), rec(b + 2 * S), n_new(b + 3 * S), finished(n_new + PLAN_REQ_WORDS), tok_pos(n_new + 2 * PLAN_REQ_WORDS), n_active(n_new + 3 * PLAN_REQ_WORDS) {}
    static size_t row_words(size_t rows) { return 3 * rows; }  static size_t state_words() { return 4 * PLAN_REQ_WORDS; }
    static size_t words(size_t tok_cap) { return row_words(tok_cap) + state_words(); }
};
// align plan (align_plan_d / align_plan_h): per score row its query row and its sequence, tok_cap of each; then per sequence row0 | L | a0 | A (seq, 4 words each); then
// the selected heads layer by layer (tail_words: seq and heads, which travel as one copy)
struct AlignPlan {
    int *qrow, *rseq, *seq, *heads;
    AlignPlan(int* b, size_t tok_cap) : qrow(b), rseq(b + tok_cap), seq(b + 2 * tok_cap), heads(seq + 4 * PLAN_REQ_WORDS) {}
    static size_t tail_words() { return 4 * PLAN_REQ_WORDS + ALIGN_MAX_HEADS; }
    static size_t words(size_t tok_cap) { return 2 * tok_cap + tail_words(); }
};

#define HIPC(e, call)                                                                                      \
    do {                                                                                                   \
        hipError_t _r = (call);                                                                            \
        if (_r != hipSuccess) {                                                                            \
            const bool oom = (_r == hipErrorOutOfMemory);                                                  \
            return fail(e, oom ? SONIC_ERR_OOM : SONIC_ERR_HIP, "%s%s failed: %s (%s:%d)",                 \
                        oom ? "HIP out of memory: " : "", #call, hipGetErrorString(_r), __FILE__, __LINE__); \
        }                                                                                                  \
    } while (0)

#define TRY(x) do { int _s = (x); if (_s != SONIC_OK) return _s; } while (0)
// every locked C-ABI entry: serialise on the engine, select its device, and hand its experiment knobs to the launchers
// (hipGetLastError first: the slot is per thread and sticky, so a failure some earlier call of this thread ignored would otherwise
// surface at this call's closing hipGetLastError check)
#define ENTER(e) std::lock_guard<std::mutex> lk((e)->mu); (void)hipGetLastError(); HIPC(e, hipSetDevice((e)->device)); g_opts = (e)->opts
// ENTER for the entry points that consume the tables of sonic_set_request_bias (sonic_prefill*, sonic_run_staged, sonic_transcribe_*): whatever way the call
// leaves - a staging error ahead of the prefill included - the pending tables are dropped, so they can never reach a later batch (the values of
// sonic_set_request_sampling likewise).  keep: sonic_run_staged_async accepted the run, whose prefill is now their consumer
void req_drop_pending(sonic_engine* e);             // every per-request stage (engine_generation.cpp): nothing is pending afterwards, the staged grammar references are handed back
struct ReqDrop { sonic_engine* e; bool keep = false; ~ReqDrop() { if (!keep) req_drop_pending(e); } };
#define ENTER_CONSUME(e) std::lock_guard<std::mutex> lk((e)->mu); ReqDrop req_drop_{e}; (void)hipGetLastError(); HIPC(e, hipSetDevice((e)->device)); g_opts = (e)->opts

// ------------------------------------------------------------------------------------------ helpers (engine.cpp)
int fail(sonic_engine* e, int code, const char* fmt, ...);
hipError_t stream_sync(sonic_engine* e);
hipError_t h2d(sonic_engine* e, void* dst, const void* src, size_t bytes);
hipError_t d2h_async(sonic_engine* e, void* dst, const void* src, size_t bytes);
hipError_t d2h(sonic_engine* e, void* dst, const void* src, size_t bytes);
void zero_fill(sonic_engine* e, void* q, size_t bytes);
// Every device buffer is an ordinary hipMalloc allocation that sonic_destroy hands back to the driver (`del asr_model.model` is expected to
// return the VRAM: backend/main.py:84-90).  Rounds 2-3 kept the per-step activation buffers (and, in round 2, the KV cache and the tiled
// weights) in uncached (MTYPE UC) memory, parked in a process-wide pool that was never freed, because memory recycled between uncached and
// ordinary allocations came back with stale cache lines on this stack (tests/test_gemm256_path failed in 3 of 5 full-suite runs; root cause
// never found, tools/uc_recycle_repro.hip excludes two mechanisms).  Round 4 measured what the uncached buffers were still worth: nothing
// (bench.py, one box, SONIC_NO_UC=1 vs default: 126.27 vs 126.17 segments/s with two slots, 103.3 vs 103.6 one batch at a time - inside the
// run-to-run spread), so the uncached path, its pool and sonic_release_pool are gone rather than kept alive for an unmeasurable gain.
template <typename Tt> static int dalloc(sonic_engine* e, Tt** p, size_t n, bool zero = true) {
    void* q = nullptr;
    const size_t bytes = ((n ? n : 1) * sizeof(Tt) + 3) / 4 * 4;
    HIPC(e, hipMalloc(&q, bytes));
    e->allocs.push_back(q); e->alloc_bytes += (int64_t)bytes;
    if (zero) zero_fill(e, q, bytes);
    *p = (Tt*)q;
    return SONIC_OK;
}
// ... and hands one of them back early (a buffer exchanged for a larger one): n is the element count dalloc was given.  Waits for the stream first
template <typename Tt> static int dfree(sonic_engine* e, Tt** p, size_t n) {
    HIPC(e, stream_sync(e));
    const auto it = std::find(e->allocs.begin(), e->allocs.end(), (void*)*p);
    if (it != e->allocs.end()) e->allocs.erase(it);
    HIPC(e, hipFree(*p));
    e->alloc_bytes -= (int64_t)(((n ? n : 1) * sizeof(Tt) + 3) / 4 * 4);
    *p = nullptr;
    return SONIC_OK;
}

// ------------------------------------------------------------------------------------------ pipeline stages (engine_stages.cpp)
void gemm(sonic_engine* e, int epi, const bf16_t* A, long lda, const bf16_t* W, const float* bias, bf16_t* C, long ldc,
          int M, int N, int K, const bf16_t* R = nullptr, long ldr = 0, int w_tiled = 0, int gu8 = 0);
bool qlinear(sonic_engine* e, int epi, const bf16_t* X, long ldx, const bf16_t* w16, const QW& q, const float* bias, bf16_t* C, long ldc,
             int M, int N, int K, const bf16_t* R, long ldr, const QGroup& grp, const float* rope_cs = nullptr, int rope_T = 0, int rope_ncols = 0,
             bool prequant = false, const QkvVt* vt = nullptr);
extern thread_local int g_last_qlinear_defer;   // whether the calling thread's last int8 qlinear handed rows to the outlier side product (sonic_debug_read "gemm_route", fifth value; tests)
bool enc_qkv_fuses_rope(sonic_engine* e, const GemmArgs& a);   // the q|k|v launch of a 16-bit encoder layer takes the RoPE into its epilogue (also the form hook's rule)
int run_mel(sonic_engine* e, int W, bool want_f32);
int run_encoder(sonic_engine* e, int W, float* enc_layers_out, float* enc_out_host, int n_groups);
int keep_rows(const sonic_dims& d, int n_valid_frames);
int frames_of(int n_samples);
int plan_requests(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new, HostPlan& hp, int fan = 1, const int32_t* pos0 = nullptr);
int upload_plan(sonic_engine* e, int R, const HostPlan& hp);       // the prefill's prologue, every kind: the request plan through the pinned staging buffer ...
int reset_row_state(sonic_engine* e, int R, int n_tok);            // ... and the rows' counters, history, bias tables and sampling values for the greedy loop
int run_prefill(sonic_engine* e, int R, const HostPlan& hp, bool head = true);
int run_to_first_token(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new, bool want_logits);
int run_all(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new, bool want_logits);
// what every whole-batch run (run_to_first_token / run_all, run_forced_parallel) begins and ends with
int run_refuse_unready(sonic_engine* e);            // the entry refusals: weights not finalized, no PCM staged, a continuous loop on this handle
int run_wait_spliced(sonic_engine* e);              // rows of the previous batch were spliced away: the stream waits for the copy kernels that read them
int run_pick_plan_buffer(sonic_engine* e);          // plan_h = the staging buffer used two runs ago, once its copies are done
int run_reserve_dump(sonic_engine* e, bool want_logits, int dump_steps, int cap_steps, int rows);   // the step-logits dump holds cap_steps x rows x vocab; a fetch reads dump_steps of them
int run_upload_win_req(sonic_engine* e, const int32_t* req_win, int n_groups);   // int8 mode: the window -> outlier group map of the encoder
void run_zero_host_figures(sonic_engine* e);        // the decode loop's host figures start at zero ...
int run_close(sonic_engine* e, double host_enqueue_first, int steps_done);   // ... and the run ends: synchronise, the sticky error, the timings

// ------------------------------------------------------------------------------------------ the token step and its loop (engine_decode.cpp)
void skinny(sonic_engine* e, const bf16_t* X, long ldx, const bf16_t* W, float* P, int M, int N, int K, int* ks_out, long long* kt = nullptr);
GreedyArgs greedy_args(sonic_engine* e, int R, bool dump);
int chunk_graph(sonic_engine* e, int R, int n, hipGraphExec_t* out, bool svc = false);
int run_decode_steps(sonic_engine* e, int n_steps, int* done_out);
// the bits of a captured chunk's cache key above the row count (chunk_graph; GK_BIAS, GK_SAMPLE and GK_GRAMMAR are req_graph_key's): the greedy kernel's family and
// its pointers are part of the capture.  GK_TOPK counts: option top_logprobs = K <= 8 takes bits 17 .. 20
enum { GK_SVC = 1 << 12, GK_LP = 1 << 13, GK_GUARD = 1 << 14, GK_BIAS = 1 << 15, GK_SAMPLE = 1 << 16, GK_TOPK = 1 << 17, GK_GRAMMAR = 1 << 21, GK_TRUNC = 1 << 22, GK_LM = 1 << 23 };

// ------------------------------------------------------------------------------------------ scoring given tokens from a prefill (engine_score.cpp)
int run_forced_parallel(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new, bool want_logits);
void run_draft_verify(sonic_engine* e, int R, const HostPlan& hp);      // option draft_verify, behind the prefill's last layer (run_prefill)
int score_logits_alloc(sonic_engine* e);            // the chunk's logits [score_chunk_rows][vocab] the parallel forced run and the verify pass share
// word timestamps: the launches' one descriptor - Q rows [tok][Hq * 128], K as the strides say, the plan and buffers of the handle - shared by
// run_prefill / run_forced_parallel and the hook (sonic_test_attention on an align handle)
AlignArgs align_probs_args(sonic_engine* e, const bf16_t* Q, const bf16_t* K, long k_ld, long k_head_stride, long k_seq_stride, const int* heads, int n_heads, int Hq, int Hkv, const int* rec);
int align_alloc(sonic_engine* e, int S, int A_max, int heads_per_layer);      // the buffers at (at least) this run's need

// ------------------------------------------------------------------------------------------ SONIC_MODE_F32 (engine_f32.cpp)
int f32_alloc(sonic_engine* e);
int f32_finalize(sonic_engine* e);
int f32_run_encoder(sonic_engine* e, int W, float* enc_layers_out, float* enc_out_host);
GreedyArgs f32_greedy_args(sonic_engine* e, int R, bool dump);
int f32_run_prefill(sonic_engine* e, int R, const HostPlan& hp, bool head = true);   // head = false: the decoder layers only (the parallel forced run scores other rows)
void f32_score_norm(sonic_engine* e, const int* row_map, int S);                         // the final norm of the S score rows -> dhn [S][d] ...
void f32_score_logits(sonic_engine* e, int row0, int n, float* logits);                  // ... and the tied lm_head over rows row0 .. row0 + n of them
void decode_step_f32(sonic_engine* e, int R, bool dump);

// ------------------------------------------------------------------------------------------ ingest (engine_ingest.cpp), service (engine_service.cpp)
int stage_pcm_locked(sonic_engine* e, const int16_t* pcm, const int64_t* offsets, int W);
void ring_free(sonic_ring* r);
// resampler (engine_resample.cpp): the bank of in_rate -> out_rate from the owner's cache (built and uploaded on first use); refusals
// (rate <= 0, more than RS_BANK_MAX_COEF coefficients) come back as SONIC_ERR_INVALID with `err` naming the numbers
int resample_bank_get(sonic_engine* root, int64_t in_rate, int64_t out_rate, RsBank* out, std::string& err);
void resample_release(sonic_engine* e);
void async_shutdown(sonic_engine* e);
int fetch_locked(sonic_engine* e, int32_t* out_ids, int out_ld, int32_t* out_len, float* step_logits, float* out_lp = nullptr);
static inline bool fp8_chain_on(const sonic_engine* e) { return e->opt_fp8_weights && e->opt_fp8_chain; }
void drop_graphs(sonic_engine* e);                  // the captured decode chunks of this handle (engine_options.cpp)
int read_back_16(sonic_engine* e, const bf16_t* d, float* h, size_t n);   // n elements of a 16-bit device buffer -> fp32 on the host, through a temporary (engine_hooks.cpp; sonic_debug_read)

// ------------------------------------------------------------------------------------------ launch builders and shared launch sequences (the prefill's: engine_stages.cpp; the token step's: engine_decode.cpp)
// One builder per launch descriptor: production and the hooks fill SkinnyArgs / DecodeAttnArgs / the prefill's FlashArgs and RopeAppendArgs through these and set
// what only they need (i8, x_amax, pre_*, err, kt; dq, amax_out, big_out, pf) on the result.
SkinnyArgs skinny_args(const bf16_t* X, long ldx, const bf16_t* W, float* P, int M, int N, int K, int ksplit, int dt);
DecodeAttnArgs decode_attn_args(bf16_t* Kc, bf16_t* Vc, const float* P, const bf16_t* Q, int ksplit, int mpad, const float* cs, bf16_t* O, const int* kv_len,
                                int Hq, int Hkv, int ctx_max, int dt);
// the int8 token step (decode_step_i8, the sonic_test_decode_i8_* hooks): one Linear8bitLt = skinny_i8 into exact int32 slabs (amax == null: X holds the quantised rows;
// else the fp16 rows, quantised while staged from their absmax partials [M][4]; returns ksplit as launched) + the consumer's DeqInfo from deq_info
int skinny_i8(sonic_engine* e, const void* X, const float* amax, const int8_t* Wt, float* P, int M, int N, int K);
DeqInfo deq_info(const sonic_engine* e, const QuantOut& q, const QW& w, int K, const bf16_t* x16, int N);
FlashArgs prefill_flash_args(const bf16_t* Q, const bf16_t* Kc, const bf16_t* Vt, bf16_t* O, const int* q_off, const int* q_len, const int* kv_len,
                             int Hq, int Hkv, int ctx_max, int dt, const int* pre_row = nullptr, const int* pre_len = nullptr);
RopeAppendArgs rope_append_args(const bf16_t* qkv, bf16_t* q_out, bf16_t* Kc, bf16_t* Vc, bf16_t* Vt, long vt_ld, const int* tok_seq, const int* tok_pos, const float* cs,
                                int Hq, int Hkv, int ctx_max, int n_tok, int dt, const int* q_off, const int* q_len, int n_seq, int max_p);
// the o_proj -> RMSNorm -> gate/up chain of a decoder layer (decode_step, sonic_test_decode_o_gu): its forms, and its buffers in the order of OGuChain's fields -
// attention rows, tiled o_proj weights, residual rows (in place), norm weight, tiled gate/up weights and their interleave, norm output, SwiGLU output,
// sum-of-squares partials (fused forms), slabs (the other two), diagnostics slots
enum { OGU_FUSED = 0, OGU_SPLIT_NORM = 1, OGU_HALF_FUSED = 2, OGU_UNFUSED = 3 };
struct OGuChain { const bf16_t *att, *Wo; bf16_t* x; const float* ln_w; const bf16_t* Wgu; int gu8; bf16_t *hn, *act; float *ss, *slab; long long *kt_o, *kt_gu; };
void launch_o_gu(sonic_engine* e, int form, const OGuChain& c, int M, int K, int D, int ff, float eps);

// ------------------------------------------------------------------------------------------ what a handle generates with (engine_generation.cpp)
// log-probabilities (options token_logprobs / top_logprobs)
static inline int lp_width(const sonic_engine* e) { return 1 + 2 * e->opt_top_logprobs; }   // floats per token in every log-probability array of this handle
static inline bool lp_on(const sonic_engine* e) { return e->opt_token_logprobs && e->out_lp; }   // log-probabilities are live on this handle: the option is on and its buffer is there
int lp_alloc(sonic_engine* e);                      // out_lp on first use
int top_enable(sonic_engine* e, int K);             // option top_logprobs behind the lock and the busy check: out_lp at its new width
int lp_check(sonic_engine* e, const char* who);     // SONIC_ERR_INVALID naming the option when token_logprobs is off on this handle
// generation guards (sonic_set_generation)
int gen_apply(sonic_engine* e, float penalty, int ngram, const int32_t* suppress, int n_suppress);   // sonic_set_generation behind the lock and the busy check
int gen_busy(sonic_engine* e, const char* who);     // that busy check: SONIC_ERR_INVALID while the handle has work in hand
static inline bool hist_on(const sonic_engine* e) { return e->gen_on || e->opt_request_bias || e->opt_grammar || e->opt_lm; }   // the rows' input_ids are kept: a guard, the request bias, the grammar's or the language model's kernels read them
// shallow fusion (options lm / lm_weight)
static inline bool lm_live(const sonic_engine* e) { return e->opt_lm && e->lm && e->lm_words && e->lm_add && !e->opt_forced_parallel; }   // this handle decodes under its language model (a scoring handle ignores it)
int lm_create(sonic_engine* e, int id, const int* words, int64_t n);     // sonic_load_tensor "lm:<id>": the packed automaton, validated, onto e's weight owner; n = 0 destroys it
int lm_check(const char* who, const int* words, int64_t n, int vocab);   // that validation: SONIC_ERR_INVALID on the calling thread naming the broken rule
void lm_to_device_words(const int* words, std::vector<int>& out);       // the wire blob -> the device layout (LM_HEAD words in front)
int lm_select(sonic_engine* e, int id, sonic_engine* owner = nullptr);   // option lm behind the lock and the busy check (owner: the weight owner of a slot under construction): the reference, hist, the rows' words and the vector buffer on first use
int lm_set_weight(sonic_engine* e, int bits);       // option lm_weight: the bits of a finite fp32 >= 0
void lm_prefill_rows(sonic_engine* e, int R);       // a prefill's rows start at (start, no pending token)
void lm_step(sonic_engine* e, int R);               // lm_step_kernel right ahead of a greedy launch (nothing when the handle has no live model)
int lm_hook_arm(sonic_engine* e, int V, const int* words, int64_t n);    // sonic_load_tensor "lm.hook:<V>": the hooks' automaton, validated against V; every row at the start node, no pending token, weight 0
int gemm_form_stage(sonic_engine* e, const char* which, const void* data, int dtype, const int64_t* shape, int ndim);   // sonic_load_tensor "gemm.form:<buffer>" (engine_hooks.cpp)
int gemm_form_run(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim);                          // sonic_load_tensor "gemm.form.run": one GEMM in a production launch form
int gemm_form_read(sonic_engine* e, const char* name, float* out, int64_t n);                                             // sonic_debug_read "gemm_form_c" / "gemm_form_vt" / "gemm_route"; -1: another name
int lm_hook_step(sonic_engine* e, const int* finished, int64_t B);       // sonic_load_tensor "lm.hook.step": lm_step_kernel alone over B rows of the armed hook model (engine_hooks.cpp)
// the three per-request stages' switches (engine_options.cpp) and what the hooks and sonic_load_tensor share with them
int bias_enable(sonic_engine* e, int on);           // option request_bias behind the lock and the busy check: hist, the tables and their staging buffer on first use
int samp_enable(sonic_engine* e, int on);           // option sampling behind the lock and the busy check: the rows' words and their staging buffer on first use
int trunc_enable(sonic_engine* e, int on);          // option truncation behind the lock and the busy check: refused by name unless sampling is on; the rows' words and their staging buffer on first use
// one row's (top_k, top_p, min_p) as "request_truncation" states it -> the three words the kernel reads; SONIC_ERR_INVALID naming `who`, the row and the parameter for a
// NaN or a value out of range (message on e, or the calling thread's for e = NULL); nothing is clamped
int trunc_pack(sonic_engine* e, const char* who, const float* v, int row, unsigned* w);
int trunc_stage_rows(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim);   // sonic_load_tensor "request_truncation": the values of the next prefill's rows
int trunc_hook_arm(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim);     // sonic_load_tensor "truncation.hook": the next sonic_test_greedy_sample launch's rows
int share_hook_arm(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim);     // sonic_load_tensor "share_prompt.hook" (engine_hooks.cpp): the next sonic_test_prefill_attention launch's pre_row | pre_len
int gram_enable(sonic_engine* e, int on);           // option grammar behind the lock and the busy check: hist, the rows' references and state words and their staging buffer on first use
// one request's table as sonic_set_request_bias takes it -> its BIAS_ROW_WORDS device words, grouped and ordered as the kernel reads them; *count = its entries.
// SONIC_ERR_INVALID (message on e, naming `who`) for more than BIAS_MAX_ENTRIES entries, a length outside 1 .. BIAS_MAX_LEN, an id outside [0, V), a NaN or +inf bias
int bias_pack(sonic_engine* e, const char* who, const int32_t* seq_ids, const int32_t* seq_off, const float* bias, int n, int V, int* row, int* count);
int samp_check(sonic_engine* e, const char* who, const float* temperature, int n);   // SONIC_ERR_INVALID (message on e, or the calling thread's for e = NULL) unless every value is 0 or in [1e-3, 100]
void samp_pack(unsigned* w, float t, uint64_t seed);   // one row's three words as the kernel reads them: the temperature's bits, the seed's low and high word
int gram_create(sonic_engine* e, int id, const int* words, int64_t n);   // sonic_load_tensor "grammar:<id>": the packed automaton [N | E | node_off | edge_tok | edge_next] onto e's weight owner; n = 0 destroys it
int gram_hook_arm(sonic_engine* e, int V, const int* words, int64_t n);  // sonic_load_tensor "grammar.hook:<V>": the hooks' automaton, validated against V; every row free, no EOS ids
int gram_stage_begin(sonic_engine* e, int R);       // option request_grammar_begin: R requests staged for the next prefill, all free (the caller holds the lock)
int gram_stage_row(sonic_engine* e, int value);     // option request_grammar = request << 16 | grammar id: that staged request refers to that grammar
// the splice's one descriptor (splice_kv_kernel / splice_state_kernel, engine_service.cpp, which fills the rest of it); declared here for req_splice_args
struct SpliceArgs {
    const bf16_t *Ks, *Vs; bf16_t *Kd, *Vd; int layers, Bm, Hkv, ctx, hd;
    int src[64], dst[64];
    const int *kv_len_s, *tok_pos_s, *n_new_s, *fin_s, *max_new_s, *out_s; int out_ld;
    const int* hist_s; int* hist_d;                      // generation guards on the destination: the row's history (prompt + first token) travels with it, [.][ctx]
    const int* bias_s; int* bias_d;                      // option request_bias on both: the row's table travels with it (count first, then only the used entries)
    const unsigned* samp_s; unsigned* samp_d;            // option sampling on both: the row's temperature and seed travel with it (its step index is n_new)
    const unsigned* trunc_s; unsigned* trunc_d;          // option truncation on both: the row's three words travel with it
    const int* lm_s; int* lm_d;                          // option lm on both: the row's state word and pending token travel with it ([state 64 | tok 64])
    unsigned long long* gram_s; unsigned long long* gram_d;            // option grammar on both: the row's grammar reference and its state word (behind the 64 references) MOVE with it: the source row is free afterwards
    const float* lp_s; float* lp_d; int lp_w;            // option token_logprobs on the destination: the first token's log-probability record (lp_w floats: 1, or 1 + 2K with
                                                         // option top_logprobs) travels with its id
    int *kv_len_d, *tok_pos_d, *n_new_d, *fin_d, *max_new_d, *out_d, *n_active_d;
    int* mirrored_d;                                     // the destination's mirror flags: a spliced row's tokens are not in the pinned mirror yet
    const bf16_t *sx_s, *shn_s; bf16_t *sx_d, *shn_d; int D;
    const int8_t* hq_s; int8_t* hq_d; const float *sca_s, *ov_s; float *sca_d, *ov_d; const int *oc_s, *ol_s; int *oc_d, *ol_d;   // int8 mode: layer 0's quantised input row
};
// The per-request stages (bias, samp, gram) at every point of a request's life, one function per point: the stages are listed in these functions and nowhere else.
// The caller holds the lock (both locks: the splice)
int req_claim(sonic_engine* e, int R, bool forked = false);   // a prefill begins: it consumes what the setters left; SONIC_ERR_INVALID when a setter was given another count than the batch's R (forked: R counts rows, and a draft is refused)
const char* req_claim_none(sonic_engine* e);        // ... a run that applies no processors: consumed all the same; names what was staged (NULL: nothing was)
int req_upload(sonic_engine* e, int R);             // the prefill's part: the claimed values, or the neutral ones, into the rows' words, on the stream
void req_greedy_args(const sonic_engine* e, GreedyArgs& g);   // the rows' words into the greedy launch (g.out_lp and g.hist are set)
int req_graph_key(const sonic_engine* e);           // the stages' bits of a captured chunk's cache key (the greedy kernel's family is part of the capture)
int req_splice_check(sonic_engine* d, sonic_engine* p);      // SONIC_ERR_INVALID (message on d) unless source and destination agree in every stage's option
void req_splice_args(sonic_engine* d, sonic_engine* p, SpliceArgs& a, const int32_t* src_rows, const int32_t* dst_rows, int n);   // the rows' words travel; a row's grammar reference moves with it
void req_rows_free(sonic_engine* e);                // a continuous loop begins: every row of the pool is free
int* req_release_state(const sonic_engine* e);      // what the release kernels reset in a fetched row beside its counters (NULL: nothing) ...
void req_row_release(sonic_engine* e, int row);     // ... and what the row held on the host goes with it
void req_batch_fetched(sonic_engine* e, const int* fin, int R);   // a batch is fetched: once its R rows have all ended they let go of what they held
// draft-verified decoding (option draft_verify)
int draft_enable(sonic_engine* e, int on);          // the option behind the lock and the busy check: refused on the int8 and fp32 kinds and on a scoring handle
int draft_stage_words(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim);   // sonic_load_tensor "request_draft": the drafts of the next prefill's requests
// a prefill begins (behind req_claim): the claimed drafts checked against the batch (SONIC_ERR_INVALID naming the cause) and, when one of them is not empty, the
// requests' longer sequences prompt || draft (ids, off), the budgets plan_requests checks them with (left) and the draft lengths (dlen).  dlen stays empty otherwise
int draft_extend(sonic_engine* e, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new,
                 std::vector<int32_t>& ids, std::vector<int64_t>& off, std::vector<int32_t>& left, std::vector<int>& dlen);
int draft_alloc(sonic_engine* e);                   // the buffers, at the handle's first drafted prefill (and ver_rec again when top_logprobs has changed since)
// row forks (sonic_load_tensor "request_forks")
int fork_stage_counts(sonic_engine* e, const void* data, int dtype, const int64_t* shape, int ndim);   // the fork counts of the next prefill's requests
// a prefill begins (ahead of req_claim, which then counts rows): the staged counts are consumed - checked against the batch's R requests (SONIC_ERR_INVALID naming
// request_forks) and returned as the row -> request map (empty: no counts, or all of them 1 - the prefill of today)
int fork_claim(sonic_engine* e, int R, std::vector<int>& fork_src);
ForkArgs fork_args(sonic_engine* e, int R, const std::vector<int>& fork_src);      // the copy's one descriptor (run_prefill)
int gen_inherit(sonic_engine* e, const sonic_engine* root);   // sonic_slot_create: the owner's generation options (token_logprobs .. forced_align) onto the new slot, with their buffers
void gen_release(sonic_engine* e);                  // sonic_destroy: the stages' pinned mirrors and events, the grammar references this handle holds, an owner's grammars
