/*
 * sonic_hip.h -- C ABI of libsonic_hip.so, the MI355X-native engine behind SonicScribe's
 * ASRModel.transcribe() (reference: backend/asr.py:335-488).
 *
 * The reference has no FFI of its own (pure Python); this is the boundary its
 * `ASRModel` methods bind through ctypes (sonicscribe_amd/engine.py).  Plain
 * pointers and sizes only; every function returns a sonic_status; outputs are caller-allocated;
 * no callbacks; no global state besides the handle.  Calls on one engine are serialised
 * internally (the reference is entered from up to 3 executor threads plus the event-loop
 * thread, backend/main.py:429-430,616-624, backend/transcription_manager.py:58).
 *
 * Which reference interface each entry point replaces:
 *   sonic_create / sonic_load_* / sonic_finalize_weights
 *                              ASRModel.__init__ + _load_model_standard   asr.py:25-87,120-146
 *                              (models_manager.asr_model_init             models_manager.py:16-32)
 *   sonic_transcribe_batch     the device part of ASRModel.transcribe     asr.py:393-422
 *                              (processor features + model.generate(do_sample=False))
 *   sonic_stage_pcm / sonic_run_staged / sonic_fetch_tokens
 *                              the same, split so PCM can be HBM-resident before a timed region
 *   sonic_logmel               WhisperFeatureExtractor.__call__ as invoked from asr.py:393
 *                              (HF:feature_extraction_whisper.py:193-346)
 *   sonic_encode               GlmAsrModel.get_audio_features             HF:modeling_glmasr.py:380-408
 *   sonic_prefill / sonic_decode_step
 *                              the two halves of model.generate: the prompt forward (logits_to_keep = 1,
 *                              HF:generation/utils.py:2612-2616) and iterations of the greedy loop (:2876-2943)
 *   sonic_device_info          torch.version.cuda / torch.cuda.get_device_name() / get_device_properties(0).total_memory
 *                              in ASRModel.get_model_info                   asr.py:501-506
 *   sonic_memory_info          torch.cuda.memory_allocated() / memory_reserved() in the debug dict  asr.py:453-457
 *   sonic_destroy              `del asr_model.model` + torch.cuda.empty_cache(): every device byte goes back   backend/main.py:84-90
 *   sonic_last_error           the exception text re-raised at            asr.py:469-481
 *   sonic_vad_create / sonic_vad_load_tensor / sonic_vad_destroy / sonic_vad_last_error
 *                              VADProcessor.__init__ (load_silero_vad)    backend/vad.py:7-22
 *                              (models_manager.vad_model_init             models_manager.py:34-49)
 *   sonic_vad_probs            the model(chunk, 16000) loop inside get_speech_timestamps as called from
 *                              VADProcessor.detect_voice_activity / is_voice_active   backend/vad.py:41-126
 *   sonic_vad_probs_rings      the same loop over audio that already lies in device rings: the whole-file VAD call of
 *                              /transcribe/file (backend/main.py:308-314, the file tensor uploaded for it) and the per-tick
 *                              window of vad_processor_manager.py:95-104 (int16 / 32768 of the accumulated chunks)
 *   sonic_resample             torchaudio.transforms.Resample(sampling_rate, target_sr)(wav)             backend/asr.py:255-261
 *   sonic_ring_create_rate     the host resampling in front of everything that reads a session's or a file's audio:
 *                              Resample(sampling_rate, 16000) at backend/vad.py:63-67 and :108-112,
 *                              audio.set_frame_rate(16000) at backend/utils.py:18
 *   sonic_ring_flush           the end of such a stream (the trailing samples of Resample's output)      backend/asr.py:255-261
 *   sonic_ring_read            the per-session debug WAV dump                                            backend/debug.py:14-72
 *   sonic_fetch_logprobs / sonic_fetch_rows_lp / sonic_dispatch_next_lp / sonic_pipeline_submit_lp
 *                              the "confidence" field of the wire messages, which the reference can only fill with the constants
 *                              "tentative" and "high": every emitted token's log-probability, on every scheduler
 *                                                                                                        backend/connection_manager.py:159,274
 *   sonic_test_greedy_lp       (test hook of the kernel behind them)                                     backend/connection_manager.py:159,274
 *   sonic_set_generation       the LogitsProcessorList that generate() builds from the checkpoint's generation_config.json
 *                              (repetition_penalty, no_repeat_ngram_size, suppress_tokens)               backend/asr.py:411-422
 *   sonic_get_generation / sonic_test_greedy_guard   (what is in force; test hook of the kernel behind it)
 *   sonic_set_request_bias     `hotwords` of a request as a bias on the scores: HF's sequence_bias / bad_words_ids
 *                              (SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor; generation/logits_process.py),
 *                              one table per request                                                      backend/asr.py:303-333
 *   sonic_test_greedy_bias     (test hook of the kernel behind it; through the dispatcher: sonic_dispatch_request's seq_ids .. n_seq)
 *   sonic_set_request_sampling temperature sampling with a seed per request (HF's TemperatureLogitsWarper + multinomial as one Gumbel-max draw): what
 *                              openai-whisper's decode_with_fallback retries a poor segment with
 *   sonic_test_greedy_sample   (test hook of the kernel behind it; through the dispatcher: sonic_dispatch_request's sampled, temperature, seed)
 */
#ifndef SONIC_HIP_H
#define SONIC_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: these declarations are its whole dynamic symbol table (tests/test_host_logic.py checks
 * `nm -D` against this header).  SONIC_ABI_VERSION moves whenever a signature or a struct layout below changes. */
#define SONIC_API __attribute__((visibility("default")))
#define SONIC_ABI_VERSION 13
SONIC_API int sonic_abi_version(void);

typedef struct sonic_engine sonic_engine;

typedef enum {
    SONIC_OK = 0,
    SONIC_ERR_INVALID = 1,   /* bad argument / shape / state            -> ValueError / RuntimeError */
    SONIC_ERR_HIP = 2,       /* HIP runtime failure                     -> RuntimeError */
    SONIC_ERR_OOM = 3,       /* message contains "out of memory" (asr.py:471 hint branch) */
    SONIC_ERR_MISMATCH = 4,  /* audio placeholders != audio feature rows (HF:modeling_glmasr.py:426-429) */
    SONIC_ERR_UNSUPPORTED = 5
} sonic_status;

/* SONIC_MODE_INT8 = asr.py mode="int8" (:148-210): fp16 activations, every nn.Linear except lm_head / embed_tokens replaced by
 * LLM.int8() (row-wise int8 weights, per-token int8 activations, outlier columns |x| >= 6.0 in fp16).  bitsandbytes is absent offline,
 * so this mode is checked against the restatement in oracle/sonic_oracle.c only (parity unpinned). */
enum { SONIC_MODE_NATIVE = 0 /* bf16, asr.py mode="native" */, SONIC_MODE_INT8 = 1 /* asr.py mode="int8" */,
       /* test only: fp16 weights and activations through the SAME kernel templates (their KF16 / f16_t instantiations - since round 5 also
        * the fused decode kernels skinny_o / skinny_gu the bf16 headline runs), no quantisation.  Not an asr.py mode: it exists so that layouts,
        * epilogues, RoPE, masking, KV append and the greedy controller can be checked at fp16's 8x finer rounding against the reference's fp32
        * arithmetic (tests/test_gpu_fp16_mode.py) */
       SONIC_MODE_F16 = 2,
       /* test only: the fp32 KIND of every stage (csrc/f32kind.hip) - fp32 weights, activations and accumulation behind the same request plan, PCM
        * staging, log-mel kernel, prompt assembly, KV bookkeeping and greedy controller (greedy_kernel<float>).  It exists to show north_star's
        * "within 1e-3 on logits" literally on the GPU (tests/test_gpu_fp32_mode.py against tests/golden/\*_fp32.npz); the product kinds keep the
        * reference's bf16 / fp16 op-boundary roundings and cannot.  No slots, no continuous decoding, no graphs; speed is irrelevant. */
       SONIC_MODE_F32 = 3 };
enum { SONIC_DTYPE_F32 = 0, SONIC_DTYPE_BF16 = 1, SONIC_DTYPE_I32 = 2 /* grammars only: sonic_load_tensor "grammar:<id>" */ };

/* Model dimensions (defaults: HF:configuration_glmasr.py:44-54,86-103). */
typedef struct {
    int32_t n_mels, n_frames, enc_T;
    int32_t enc_d, enc_ff, enc_layers, enc_heads, enc_rotary_dim;
    float enc_theta, enc_ln_eps;
    int32_t merge;
    int32_t dec_d, dec_ff, dec_layers, dec_heads, dec_kv_heads, dec_head_dim;
    float dec_theta, dec_rms_eps;
    int32_t vocab, audio_token_id, n_eos;
    int32_t eos[8];
} sonic_dims;

/* Per-stage device time of the last sonic_run_staged / sonic_transcribe_batch (HIP events on the engine stream). */
typedef struct {
    float mel_ms, encoder_ms, prefill_ms, decode_ms, total_ms;
    float gemm_ms;          /* summed duration of the encoder's dominant GEMM kernel launches (fc1, bias+GELU epilogue) */
    int32_t gemm_launches;  /* ... and how many launches that was */
    double gemm_flops;      /* algorithmic FLOPs of those launches */
    int32_t decode_steps;
    float enc_gemm_ms;      /* summed duration of ALL encoder-layer GEMM launches (QKV, o, fc1, fc2) of the last run */
    double enc_gemm_flops;  /* ... and their algorithmic FLOPs (SURVEY.md 8d "encoder GEMM MFMA utilisation") */
    /* host side of the same run (wall clock of the calling / worker thread): enqueueing everything up to the first token, time inside the
     * decode loop's hipGraphLaunch calls, time blocked on the pipelined early-stop checks, and how many chunk launches that was */
    float host_prefill_enqueue_ms, host_decode_launch_ms, host_decode_wait_ms;
    int32_t host_decode_launches;
    int32_t decode_lookahead;   /* chunks the decode loop kept queued beyond the early-stop check it was waiting for (adapts: 1 on a host that keeps up) */
    int32_t decode_launches_per_layer;   /* kernel launches per decoder layer of the token step the last run used (5: <= 2 rows, round 6; 6: fused bf16 / fp16 chain; 7: 33 - 64
                                          * rows inside continuous loops; 8: int8 and the unfused chain) */
} sonic_timings;

/* ---- lifetime ---- */
SONIC_API int sonic_device_count(void);
/* max_batch: windows per call (<= 64); max_ctx: decoder context capacity per sequence (multiple of 64). */
SONIC_API int sonic_create(const sonic_dims* dims, int device_id, int mode, int max_batch, int max_ctx, sonic_engine** out);
SONIC_API void sonic_destroy(sonic_engine* e);
SONIC_API const char* sonic_last_error(sonic_engine* e); /* e may be NULL: error of the last failed sonic_create on this thread */
/* name (NUL-terminated, truncated to name_cap), total / currently free device memory, hipRuntimeGetVersion(); any output may be NULL */
SONIC_API int sonic_device_info(int device_id, char* name, int name_cap, int64_t* total_bytes, int64_t* free_bytes, int32_t* hip_runtime_version);
/* How many hardware queues the HIP runtime of THIS process gives its streams on the device (measured once per device: eight probe streams with a
 * 300 us spin kernel each; streams that share a queue run in order), what GPU_MAX_HW_QUEUES says now (0 = unset) and how many an engine with slots,
 * device rings and VAD wants (8).  Every handle owns ONE stream - finished rows of a continuous loop leave through a pinned mirror, not a stream of their
 * own - so a bulk pipeline of D decoding and P prefill handles needs D + P queues: the default 3 + 1 fits the runtime's own default of four; each device
 * ring, the resampler and a VAD add a stream of theirs.  The runtime reads the variable at its first call only: in the reference's process torch initialises it (backend/asr.py:53
 * `torch.cuda.is_available()`), so the host sets GPU_MAX_HW_QUEUES=8 in its environment - the library never writes the
 * environment, and the first sonic_create warns on stderr when the measured count is below the wanted one (SONIC_QUIET=1 silences it). */
SONIC_API int sonic_runtime_info(int device_id, int32_t* hw_queues, int32_t* hw_queues_env, int32_t* hw_queues_wanted);
/* allocated: bytes of this handle's live device allocations (a slot: its own buffers; the weights are its owner's); reserved = allocated
 * (no caching allocator under the engine: sonic_destroy returns everything to the driver) */
SONIC_API int sonic_memory_info(sonic_engine* e, int64_t* allocated_bytes, int64_t* reserved_bytes);

/* Another batch in flight on the SAME weight copy.  The reference keeps up to three decodes in flight on its one model object in file
 * mode (backend/main.py:429-445, asyncio.Semaphore(3) + run_in_executor at :616-624) and serialises them on the device; here a slot is a
 * full engine handle of its own -- stream, PCM staging, activation buffers, KV cache, decode graphs, lock, options -- whose weight and
 * constant pointers are the owner's (sonic_weight_bytes(owner) does not move, sonic_weight_bytes(slot) == 0).  Batches on different slots
 * run concurrently on the GPU: one batch's MFMA-bound encoder / prefill fills the bubbles of another's latency-bound decode loop
 * (DESIGN.md 4).  Every entry point below takes a slot handle; rings created through any handle can be staged by every slot of the same
 * owner.  sonic_destroy(slot) releases a slot early; sonic_destroy(owner) releases its slots first (their handles are dead after that).
 * sonic_slot_count: the owner plus its live slots. */
SONIC_API int sonic_slot_create(sonic_engine* owner_or_slot, sonic_engine** slot_out);
SONIC_API int sonic_slot_count(sonic_engine* e);
/* row / context capacity, mode, device and the identity of the weight copy (equal for an engine and all of its slots) of a handle; any out pointer may be NULL */
SONIC_API int sonic_engine_info(sonic_engine* e, int32_t* max_batch, int32_t* max_ctx, int32_t* mode, int32_t* device_id, const void** weights_id);

/* ---- the bulk pipeline as native threads (round 5) ----
 * What sonicscribe_amd/pipeline.py's host loop does (round 4: Python threads over the calls above, polling) inside the library: one thread per
 * prefill handle (stage PCM, queue log-mel + encoder + prompt forward + first token, hand the batch over), one per decoding handle (splice
 * handed-over batches into free row blocks of its continuously decoding handle, queue decode chunks, fetch the rows of a block the moment all of
 * them are finished).  Every wait is a condition variable or a blocking HIP event: no polling, no interpreter in the loop - the headline no longer
 * depends on how quickly a busy host schedules Python threads.  The reference's counterpart: three executor threads around one model object
 * (backend/main.py:429-445, 616-624).
 *   sonic_pipeline_create(decoders, n_dec, prefills, n_pre, block, rows_per_decoder, &p)   handles of ONE weight copy (an engine and its slots);
 *                       the decoders are put into continuous mode (sonic_service_begin); a decoder holds rows_per_decoder / block batches at a time
 *   sonic_pipeline_submit(p, pcm, offsets, W, req_win, R, prompt_ids, prompt_off, max_new, out_ids, out_ld, out_len, &ticket)
 *                       one batch of R <= block requests (arguments as sonic_transcribe_batch).  pcm == NULL: the batch is what the prefill
 *                       handles already have staged (sonic_stage_pcm on each of them; the benchmark's HBM-resident input).  The prompt arrays
 *                       are copied; pcm, out_ids and out_len must stay valid until the ticket is waited for.  Returns at once.
 *   sonic_pipeline_wait(p, ticket)   blocks until that batch's rows are in out_ids / out_len and returns its status; ticket 0: every batch
 *                       submitted so far, first failure or SONIC_OK.  A bad request fails alone; a failed decoding handle fails everything in flight.
 *   sonic_pipeline_destroy(p)       completes what was submitted, joins the threads, sonic_service_end on the decoders (the handles stay yours) */
typedef struct sonic_pipeline sonic_pipeline;
SONIC_API int sonic_pipeline_create(sonic_engine* const* decoders, int n_dec, sonic_engine* const* prefills, int n_pre, int block, int rows_per_decoder,
                                    sonic_pipeline** out);
SONIC_API int sonic_pipeline_submit(sonic_pipeline* p, const int16_t* pcm, const int64_t* offsets, int W, const int32_t* req_win, int R,
                                    const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new,
                                    int32_t* out_ids, int out_ld, int32_t* out_len, int64_t* ticket_out);
SONIC_API int sonic_pipeline_wait(sonic_pipeline* p, int64_t ticket);
SONIC_API int sonic_pipeline_stats(sonic_pipeline* p, int64_t* batches_done, int64_t* chunks_queued, int32_t* batches_in_flight_max);
SONIC_API const char* sonic_pipeline_last_error(sonic_pipeline* p);
SONIC_API int sonic_pipeline_destroy(sonic_pipeline* p);

/* ---- weights (names: GlmAsrForConditionalGeneration.state_dict() keys, see sonicscribe_amd/spec.py) ----
 * On a finalized engine the call also carries the named int32 words that need no entry point of their own: "grammar:<id>" /
 * "grammar.hook:<V>" (DESIGN.md 6.10), "request_draft" (6.11, beside sonic_set_forced_ids), "request_forks" and "lm:<id>" / "lm.hook:<V>" /
 * "lm.hook.step":
 *
 * Shallow fusion (options lm / lm_weight): a backoff n-gram language model over the model's own tokens, added to every step's scores inside the decode
 * loops.  One hypothesis, no search; an option of a handle, not a value of a request.
 *   sonic_load_tensor(e, "lm:<id>", words, SONIC_DTYPE_I32, {n}, 1), id in 1 .. 65535, creates the model on e's weight owner (shape {0}: destroys it - refused by
 *   name while a handle's option lm refers to it); it takes the owner's registry lock, not the engine lock, and its bytes are counted by sonic_memory_info.
 *   words (floats as their bits): V | N | E | order | start | uni[V] f32 | node_off[N + 1] | bo_next[N] | bo_w[N] f32 | edge_tok[E] | edge_next[E] | edge_w[E] f32.
 *   Node 0 is the empty context; a node's edges ascend strictly by token id; bo_next[0] = -1 and 0 <= bo_next[n] < n (nodes are numbered by context length), a
 *   chain has at most order - 1 links; uni[w], the root's log-probability (natural log) of every id, and all weights are finite; root edges serve the transition
 *   only and carry uni's bits; order <= 8, N <= 4 194 304, E <= 16 777 216, V = the model's vocabulary; a node may have no edge.  Every violation is
 *   SONIC_ERR_INVALID naming the rule (the calling thread's sonic_last_error(NULL)); nothing is truncated.
 *   scores of a row at node n, all in fp32 with separately rounded operations, L = lm_weight: c_0 = n, c_{j+1} = bo_next[c_j] down to c_k = 0; A_0 = +0,
 *   A_{j+1} = A_j + bo_w[c_j]; add[w] = L * (A_k + uni[w]) for every w; then for j = k - 1 down to 0, in that order, add[edge_tok[e]] = L * (A_j + edge_w[e]) for
 *   every edge e of c_j: the longest context that lists an id wins.  transition on the emitted token t: t is searched among the node's edges - found, the state is
 *   edge_next; else the search repeats at bo_next, and ends at the root; a token outside [0, V) ends at the root.
 *   option lm = id (0: off; after token_logprobs; on the owner before its slots are created - they copy it), option lm_weight = the bits of the fp32 L, finite and >= 0.
 *   lm switches the rows' history on as grammar does and allocates two state words per row and the vector buffer, max_batch x V fp32.  lm_step_kernel (one block per
 *   row) then runs right ahead of every greedy launch - prefill, decode steps of every kind, captured or not - consuming the row's pending token and writing its
 *   vector; the greedy kernel's LM instantiations form rT(logit) + add[w] ahead of the request bias (then penalty, bans, temperature).  The step logits stay raw; the
 *   log-probabilities, the alternatives and the truncation see the fused scores.  sonic_splice_rows moves the two words and refuses handles whose lm or lm_weight
 *   differ.  Refused by name: lm beside grammar or draft_verify (and the reverse), row forks and sonic_pipeline_create on such a handle; a scoring handle
 *   (forced_parallel) ignores it.  The int8 and fp32 kinds support it (same greedy families).
 *   hooks: "lm.hook:<V>" arms an automaton validated against V (shape {0}: disarms); options hook_lm_state = row << 24 | state, hook_lm_tok = row << 24 | (token + 1)
 *   (0: none pending) and hook_lm_weight = the bits set the rows' words; "lm.hook.step" (one `finished` word per row) launches lm_step_kernel alone;
 *   sonic_debug_read "hook_lm_state" / "hook_lm_tok" / "hook_lm_add" read the states, pending tokens and vectors [rows][V].  The next guard / bias / sample hook
 *   launch of that V with log-probabilities takes the vector through its family's LM instantiation and leaves the emitted ids in the pending tokens.
 *
 * Row forks (sonic_load_tensor "request_forks"): one prefilled request becomes several rows - N samples of one audio (Whisper's best_of) pay for
 * log-mel, encoder and prefill once.
 *   sonic_load_tensor(e, "request_forks", counts, SONIC_DTYPE_I32, {A}, 1): request a of the NEXT prefill on this handle (the entry points sonic_set_request_bias
 *   names) becomes counts[a] >= 1 rows; that call consumes the counts on success and on failure alike (sonic_run_staged_async keeps them for its run, as a draft).
 *   No option, no buffer: sonic_memory_info does not move.  Without staged counts, or with every count 1, a prefill launches exactly what it launched before.
 *   row order, with R' = sum counts: rows 0 .. A-1 are the requests themselves (fork 0), through the decoder layers exactly as without forks; the forks j >= 1
 *   follow request by request, row(a, j) = A + sum_{b < a} (counts[b] - 1) + (j - 1).  The entry point's R, prompts, budgets and req_win stay per request (A of
 *   them); sonic_set_request_bias, sonic_set_request_sampling and "request_grammar_begin" / "request_grammar" state their values per ROW, R' of them in row order;
 *   out_ids / out_len / step_logits, sonic_fetch_*, sonic_decode_step and sonic_splice_rows (src_rows) see R' rows.
 *   what runs: behind the last decoder layer fork_kv_kernel copies, per forked request, layer and kv head, the kv_len * head_dim elements of K and of V from the
 *   request's cache row to each fork's row - every 16-byte piece read once and written counts[a] - 1 times - and the row's history where the handle keeps one.  The
 *   head (final norm through the row map, lm_head, greedy kernel) then runs over R' rows: every fork's first token is drawn from its request's logits under its
 *   own row's seed, temperature, bias table and grammar.  From there on the rows are ordinary rows of the decode loops.
 *   refusals (SONIC_ERR_INVALID, the message naming request_forks): a count below 1; more rows than max_batch; the int8 and fp32 kinds; a scoring handle
 *   ("forced_parallel"); and at the prefill: an A that is not the batch's R; forced ids set (sonic_set_forced_ids); a draft in the same prefill; a per-row stage
 *   that was given another count than R'.
 *   sonic_debug_read "kcache" / "vcache" (index = decoder layer, Bm * Hkv * max_ctx * head_dim elements) read the cache; "fork_ms" (n = 1) is the kernel's time in
 *   the handle's last forked prefill.
 *
 * Truncation (option "truncation", sonic_load_tensor "request_truncation" / "truncation.hook"): top_k / top_p / min_p on the temperature-scaled scores
 * of a sampling row - HF's TopK -> TopP -> MinP warpers - with the cut found inside the greedy kernel.  sonic_set_option(e, "truncation", 1): on the owner before its
 * slots (they copy it); SONIC_ERR_INVALID naming "sampling" unless that option is on, and while the handle has work in hand; 768 bytes (64 rows x 3 words).
 *   sonic_load_tensor(e, "request_truncation", values, SONIC_DTYPE_F32, {R, 3}, 2): row r of the NEXT prefill on this handle (the entry points
 *   sonic_set_request_bias names) draws under top_k = values[3r] (an integer, 0 = off), top_p = values[3r + 1] (in (0, 1], 1 = off), min_p = values[3r + 2] (in [0, 1],
 *   0 = off); NaN and values out of range are refused by name, nothing is clamped; rows with temperature 0 ignore them.  Consumed or dropped with the sampling values;
 *   stated per row under forks; a prefill without them has every filter off; sonic_splice_rows copies a row's words and refuses handles whose options differ.
 *   dispatcher: sonic_dispatch_request's cut, top_k, top_p, min_p.
 *   "truncation.hook" (same layout, B rows) arms the next sonic_test_greedy_sample launch; sonic_debug_read "hook_truncation" (3B floats) returns its records: the y of
 *   the last kept id in (y descending, id ascending), that id, the kept count n; (0, -1, V) for a row that was not cut. */
SONIC_API int sonic_load_tensor(sonic_engine* e, const char* name, const void* data, int dtype, const int64_t* shape, int ndim);
SONIC_API int sonic_load_synthetic(sonic_engine* e, uint64_t seed);          /* portable generator, sonicscribe_amd/synth.py */
SONIC_API int sonic_finalize_weights(sonic_engine* e);                        /* packs fused QKV / gate-up, conv im2col order */
SONIC_API int64_t sonic_weight_bytes(sonic_engine* e);

/* ---- stage entry points (parity tests) ---- */
/* pcm: B segments concatenated; offsets[B+1] in samples (segment i = pcm[offsets[i] .. offsets[i+1])), each <= 30 s.
 * feats_out: [B][n_mels][n_frames] fp32 (HF layout), mask_out: [B][n_frames] int32; either may be NULL. */
SONIC_API int sonic_logmel(sonic_engine* e, const int16_t* pcm, const int64_t* offsets, int B, float* feats_out, int32_t* mask_out);
/* feats: [B][n_mels][n_frames] fp32 (cast to bf16 as asr.py:280-301 does); n_valid_frames[B].
 * embeds_out: [B][enc_T/merge][dec_d] fp32 (first n_audio_out[b] rows valid).
 * taps (optional, may be NULL): enc_layers_out [B][enc_layers][enc_T][enc_d], enc_out [B][enc_T][enc_d]. */
SONIC_API int sonic_encode(sonic_engine* e, const float* feats, const int32_t* n_valid_frames, int B,
                 float* embeds_out, int32_t* n_audio_out, float* enc_layers_out, float* enc_out);

/* ---- the hot call ---- */
/* W windows of PCM (as sonic_logmel); R requests, request r owns windows req_win[r] .. req_win[r+1]-1 (R == W and
 * req_win == NULL for the single-window case).  prompt_ids concatenated, prompt_off[R+1]; max_new[R].
 * out_ids: [R][out_ld] int32, out_len[R]; step_logits (optional): [max(max_new)][R][vocab] fp32 = the bf16 logits
 * each step's argmax saw (row r of step s valid while s < out_len[r]). */
SONIC_API int sonic_transcribe_batch(sonic_engine* e, const int16_t* pcm, const int64_t* offsets, int W,
                           const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                           const int32_t* max_new, int32_t* out_ids, int out_ld, int32_t* out_len, float* step_logits);

/* split form: stage (H2D) -> run (device only, timed) -> fetch (D2H) */
SONIC_API int sonic_stage_pcm(sonic_engine* e, const int16_t* pcm, const int64_t* offsets, int W);
SONIC_API int sonic_run_staged(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                     const int32_t* max_new, int want_step_logits);
SONIC_API int sonic_fetch_tokens(sonic_engine* e, int32_t* out_ids, int out_ld, int32_t* out_len, float* step_logits);
/* Per-token log-probabilities (option "token_logprobs", off by default; set it on the owner before its slots are created, they copy it).  For
 * token n of request r, with l the vocabulary-long vector of logits that step's argmax compared (the values step_logits returns):
 *   logprob[r][n] = l[tok] - max(l) - log(sum_i exp(l_i - max(l))),   tok = the token written to out_ids (the argmax, or the forced id)
 * = HF compute_transition_scores(sequences, scores, normalize_logits=True) of a greedy generate().  The greedy kernel sums while it searches the
 * maximum: no second pass, the decode loops keep their hipGraph form, and a request's values are the same bits on every scheduler.
 * sonic_fetch_logprobs: the rows and counts of sonic_fetch_tokens (row r's out_len[r] values at out_lp + r * out_ld; nothing beyond them is
 * written), valid whenever that call is.  Every fetch / submit form (sonic_fetch_logprobs, sonic_fetch_rows_lp, sonic_dispatch_next_lp,
 * sonic_pipeline_submit_lp) returns SONIC_ERR_INVALID, the message naming token_logprobs, while the option is off.
 *
 * The best alternatives of every step (option "top_logprobs" = K in 0 .. 8, default 0; OpenAI's top_logprobs).  sonic_set_option(e, "top_logprobs", K) on the
 * owner before its slots are created (they copy it) and after option token_logprobs (SONIC_ERR_INVALID naming token_logprobs otherwise); refused outside
 * 0 .. 8 and while the handle has work in hand; the log-probability buffer grows with it (counted by sonic_memory_info) - it is exchanged for a new one, so
 * fetch a finished batch's log-probabilities BEFORE changing K: afterwards they are gone.  With s the vector of fully
 * processed scores the log-probability sum runs over (bias, repetition penalty, bans, in that order; unperturbed and at temperature 1, also when the row
 * samples), order the ids by s descending, then id ascending: alternative k < K is the k-th id of that order among the ids with s > -inf, with
 * log_softmax(s)[id] formed from the same maximum and sum as the emitted token's value - an emitted token that is among the alternatives carries the same
 * bits, and on a greedy, unforced row alternative 0 IS the emitted token.  Places beyond the finite scores hold id -1 and -inf.  Teacher forcing and
 * sampling change the emitted token, never the alternatives.  No launch and no pass over the logits is added; tokens and their log-probabilities keep
 * their bits.
 * Record layout: while K > 0, EVERY log-probability array of the handle holds W = 1 + 2K floats per token instead of one:
 *   [0]            the emitted token's log-probability (what the array held before)
 *   [1 .. K]       the K alternatives' log-probabilities, descending
 *   [K + 1 .. 2K]  the K alternatives' ids as fp32 values (ids stay below 2^24: exact; -1 = none)
 * and the caller sizes its array per form:
 *   sonic_fetch_logprobs     out_ld counts floats: row r's out_len[r] records start at out_lp + r * out_ld, so out_ld >= W * the most tokens of a row
 *   sonic_fetch_rows_lp      out_ld counts tokens, as for out_ids: row i's records start at out_lp + i * out_ld * W (n * out_ld * W floats in all)
 *   sonic_dispatch_next_lp   out_lp holds out_cap * W floats: token i's record at out_lp + i * W
 *   sonic_test_greedy_lp / _guard / _bias / _sample   lp_out holds B * W floats: row b's record at lp_out + b * W
 *   sonic_pipeline_submit_lp stays one float per token: sonic_pipeline_create refuses a handle with K > 0, the message naming top_logprobs
 * sonic_splice_rows copies a row's first record (it comes from the prefill) and refuses handles whose K differ; sonic_dispatch_create likewise. */
SONIC_API int sonic_fetch_logprobs(sonic_engine* e, float* out_lp, int out_ld);
/* HF generate()'s logits processors for greedy decoding (generation/logits_process.py), applied inside the greedy kernel to the fp32 scores the argmax
 * compares, in HF's order.  input_ids = the request's prompt ids (audio placeholders included) followed by every id emitted so far, forced ids included:
 *   repetition_penalty p   every id that occurs in input_ids: s = s < 0 ? s * p : s / p, once (fp32 multiply, correctly rounded fp32 divide); 1.0 = none
 *   no_repeat_ngram_size n every id that followed an earlier occurrence of the last n - 1 ids becomes -inf (n = 1: every id seen); 0 = none
 *   suppress_tokens        the listed ids are -inf at every step; at most 256 ids, n_suppress = 0 = none
 * A row whose scores are all -inf emits token 0.  step_logits stay the raw logits (HF output_logits); with option token_logprobs the log-probabilities are
 * those of the processed scores (HF compute_transition_scores over `scores`; a banned forced id gives -inf).  The neutral values switch everything off:
 * the engine then launches exactly what it launched before.  Set it on the owner before its slots are created (they copy it); sonic_splice_rows refuses
 * a source whose values differ from the destination's.  SONIC_ERR_INVALID: p not finite or <= 0, n outside 0 .. 64, more than 256 ids, an id outside the
 * vocabulary, or the handle has work in hand (a prefilled batch whose decode loop has not ended, an asynchronous run, a continuous loop).
 * sonic_set_option keys "gen_repetition_penalty_milli", "gen_no_repeat_ngram_size", "gen_suppress_token" (one id, -1 = none) set one value each for
 * drivers that only pass integers. */
SONIC_API int sonic_set_generation(sonic_engine* e, float repetition_penalty, int no_repeat_ngram_size, const int32_t* suppress, int n_suppress);
/* Per-request sequence bias: HF's SequenceBiasLogitsProcessor, with NoBadWordsLogitsProcessor folded in as entries of bias -inf (generation/logits_process.py),
 * on a table that belongs to the request - the reference's per-connection / per-upload hotwords (backend/asr.py:303-333) as shallow biasing of the scores.
 * A table is a list of entries, each a token sequence of 1 .. 8 ids and an fp32 bias; equal sequences are merged as HF's list-to-dict conversion merges them (the
 * last bias wins, at the first position).  Per token a fp32 sum starts at +0.0, takes the length-1 entry of that token, then - in list order - every longer
 * entry that ends on the token, has L <= len(input_ids) and whose first L - 1 ids equal the last L - 1 ids of input_ids (the prompt ids, audio placeholders
 * included, then every emitted id); score = score + sum, once, in fp32, ahead of the processors of sonic_set_generation.  A bad word is an entry of bias -inf
 * (with finite biases the fold gives HF's bits: (s + b) -> penalty -> -inf and s + (b + -inf) -> penalty are both -inf for p > 0).  step_logits stay raw;
 * with option token_logprobs the log-probabilities are over the biased scores.  A row whose scores are all -inf emits token 0.
 *   option "request_bias" (sonic_set_option): on the owner before its slots are created (they copy it); allocates the rows' history and tables (counted by
 *       sonic_memory_info); refused while the handle has work in hand, as sonic_set_generation is.  sonic_splice_rows refuses handles whose options differ.
 *   sonic_set_request_bias: the tables of the R requests of the NEXT sonic_prefill / sonic_prefill_enqueue / sonic_run_staged[_async] / sonic_transcribe_* on this
 *       handle, which consumes them on success and on failure alike - a sonic_transcribe_* that fails while staging drops them too (a later batch starts without tables).  Request r owns entries req_off[r] .. req_off[r + 1]; entry i is
 *       seq_ids[seq_off[i] .. seq_off[i + 1]) with bias[i].  SONIC_ERR_INVALID, nothing truncated: the option is off (the message names it), more than 256
 *       entries in a request, a sequence outside 1 .. 8 ids, an id outside the vocabulary, a NaN or +inf bias; at the prefill, an R that is not the batch's.
 *   dispatcher: sonic_dispatch_request's seq_ids, seq_off, bias, n_seq. */
SONIC_API int sonic_set_request_bias(sonic_engine* e, const int32_t* seq_ids, const int32_t* seq_off, const float* bias, const int32_t* req_off, int R);
/* Temperature sampling.  A request with temperature t > 0 and a 64-bit seed emits, as its n-th token (n = 0 for the prefill's), the first maximum over
 * the vocabulary of y_i = fdiv_rn(s_i, t) + g_i in fp32: s the fully processed score (request bias, repetition penalty, bans: HF's order, then its
 * TemperatureLogitsWarper), g_i = -ln(-ln(u_i)), u_i = ((w_i >> 9) + 0.5) * 2^-23, w_i = word i & 3 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and
 * counter (i >> 2, n, 0, 0).  By the Gumbel-max identity this is an exact draw from softmax(s / t); it depends on (scores, t, seed, n) alone - never on batch, row,
 * slot or scheduler - so a sampled transcript is as reproducible as a greedy one.  The kernel's g is within 3.2e-6 of the exact value.  t = 0 is
 * greedy decoding, bit for bit.  The log-probabilities (option token_logprobs) stay log_softmax(s)[token] at temperature 1: openai-whisper's convention, the one the
 * thresholds of its fallback are calibrated on.  step_logits stay raw; teacher forcing wins over sampling; a row whose scores are all -inf emits token 0.
 *   option "sampling" (sonic_set_option): on the owner before its slots are created (they copy it) and after option token_logprobs (SONIC_ERR_INVALID naming
 *       token_logprobs otherwise); allocates three words per row (counted by sonic_memory_info); refused while the handle has work in hand.  sonic_splice_rows
 *       copies a row's words and refuses handles whose options differ.
 *   sonic_set_request_sampling: the values of the R requests of the NEXT prefill on this handle (the entry points sonic_set_request_bias names), which consumes them
 *       on success and on failure alike; a batch without values is greedy.  SONIC_ERR_INVALID, nothing clamped: the option is off (the message names it), a
 *       temperature that is neither 0 nor in [1e-3, 100] (NaN included); at the prefill, an R that is not the batch's.
 *   dispatcher: sonic_dispatch_request's sampled, temperature, seed. */
SONIC_API int sonic_set_request_sampling(sonic_engine* e, const float* temperature, const uint64_t* seed, int R);
/* Grammar-constrained decoding: a request's transcript restricted to the paths of a deterministic token automaton - HF's prefix_allowed_tokens_fn
 * (PrefixConstrainedLogitsProcessor), Vosk's `grammar`, the strict mode of a phrase list - with the mask and the state transition inside the greedy kernel.  The
 * feature adds no entry point: a grammar is loaded as a tensor, everything else is an option.
 * A grammar is an automaton in CSR form: node_off[N + 1], edge_tok[E], edge_next[E]; node 0 is the start node; the edges of node n are node_off[n] .. node_off[n + 1],
 * sorted by token id, strictly ascending.  EOS is an ordinary edge, added where a transcript may end: there is no accept flag.
 *   Per row one state word: -1 the row is free (no grammar: the kernel behaves as without the option), n >= 0 it is at node n, -2 it has left its grammar.
 *   A step of a running row at node n: every id that is not an edge token of n scores -inf, behind the request bias and the repetition penalty, folded into the
 *   bans of the n-gram guard and the suppress list (HF's chain SequenceBias -> RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> PrefixConstrained ->
 *   SuppressTokens: bans commute, so the fold gives HF's tokens); then temperature and noise for a sampled row; compare, log-probabilities and alternatives run over
 *   the masked scores.  The emitted token - argmax, sample or forced id - moves the state to its edge's `next` if n has an edge for it, else to -2 (a forced id
 *   outside the grammar; token 0, which a row emits when the guards have banned every allowed id).  A row at -2 allows only the handle's EOS ids: it ends on
 *   its next step.  step_logits stay raw; a finished row changes nothing.
 *   create: sonic_load_tensor with the name "grammar:<id>" (id 1 .. 65535, the caller's choice), dtype SONIC_DTYPE_I32, ndim 1 and the words
 *       [N | E | node_off | edge_tok | edge_next], on a finalized engine; it lands on the weight owner, is shared by all of its handles and by any number of requests,
 *       is counted by the owner's sonic_memory_info and does not wait for a decoding batch.  SONIC_ERR_INVALID, nothing truncated, the calling thread's last error
 *       (engine NULL) naming the cause: node_off[0] != 0, node_off not monotone, node_off[N] != E, a node without an edge, a token id outside [0, vocab) or equal to the
 *       audio placeholder, a `next` outside [0, N), edges of a node not sorted and unique, N outside 1 .. 65536, E outside 1 .. 1048576, a length that is not
 *       2 + N + 1 + 2E, an id that is taken, weights that are not finalized.
 *   destroy: the same call with shape {0}.  SONIC_ERR_INVALID ("in use") while a staged or running request refers to the grammar - a reference is taken when a
 *       request is staged or submitted; it moves with the row at a splice (the source row is free afterwards) and is dropped when the row is fetched from a
 *       continuous loop, when a batch whose every row has ended is fetched, when the handle's next prefill overwrites the row, or with its handle.  sonic_destroy of the owner frees what is left.
 *   option "grammar" (sonic_set_option): on the owner before its slots are created (they copy it) and after option token_logprobs (SONIC_ERR_INVALID naming
 *       token_logprobs otherwise); allocates the rows' history, if nothing else has, their references and state words (counted by sonic_memory_info); refused while
 *       the handle has work in hand.  sonic_splice_rows copies a row's reference and state and refuses handles whose options differ.
 *   options "request_grammar_begin" = R, then "request_grammar" = request << 16 | id per constrained request: the grammars of the R requests of the NEXT prefill on
 *       this handle (the entry points sonic_set_request_bias names); that prefill consumes them on success and on failure alike and starts every constrained row at
 *       node 0.  SONIC_ERR_INVALID: option grammar is off (the message names it), an id that is no live grammar of the handle's weight owner; at the prefill, an R
 *       that is not the batch's.  A scoring handle (option forced_parallel) refuses staged grammars, and consumes them, as it does bias tables.
 *   dispatcher: sonic_dispatch_request's grammar_id; the request holds a reference from its submit until it completes. */
/* the values in force on this handle; at most `cap` ids are copied to suppress, *n_suppress is their full count (any pointer may be NULL) */
SONIC_API int sonic_get_generation(sonic_engine* e, float* repetition_penalty, int32_t* no_repeat_ngram_size, int32_t* suppress, int cap, int32_t* n_suppress);
/* sonic_run_staged without blocking the caller: the arguments are copied, a worker thread owned by the handle runs the batch, the call
 * returns at once (the reference's counterpart is loop.run_in_executor(None, asr_model.transcribe, ...), backend/main.py:616-624).  One
 * outstanding run per handle; until sonic_wait has returned the handle takes no other call (ring appends excepted).
 * sonic_wait(e, 1, NULL) blocks until the run is complete and returns ITS status; sonic_wait(e, 0, &busy) polls. */
SONIC_API int sonic_run_staged_async(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                                     const int32_t* max_new, int want_step_logits);
SONIC_API int sonic_wait(sonic_engine* e, int block, int32_t* busy_out);
/* stage entry points: sonic_run_staged = sonic_prefill + sonic_decode_step(max(max_new) - 1).  sonic_prefill runs log-mel, encoder,
 * projector, decoder prefill and emits the first token of every request; sonic_decode_step runs up to n_steps further greedy steps
 * (*steps_done_out of them: fewer once the largest budget is reached or every row stopped) and reports the rows still running.
 * sonic_fetch_tokens may be called after either. */
SONIC_API int sonic_prefill(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off,
                  const int32_t* max_new, int want_step_logits);
SONIC_API int sonic_decode_step(sonic_engine* e, int n_steps, int32_t* n_active_out, int32_t* steps_done_out);
/* sonic_prefill without the closing wait: the work is queued on the handle's stream when the call returns (the splice of its rows into a
 * continuously decoding handle orders itself behind it on the device; any other reader calls sonic_synchronize first) */
SONIC_API int sonic_prefill_enqueue(sonic_engine* e, const int32_t* req_win, int R, const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new);
/* Continuous decoding: one handle decodes forever over its max_batch rows; requests join and leave ROW BY ROW instead of batch by batch.  The
 * reference awaits one transcribe() at a time per connection and blocks its event loop inside it (backend/connection_manager.py:127-245,
 * backend/transcription_manager.py:58); a batch engine makes a request wait for the running batch and pads every batch to its slowest row.
 *   sonic_service_begin(d)      d's rows become a pool (all free), its chunk graph is captured; d takes no batch calls until sonic_service_end
 *   sonic_prefill(p, ...)       on ANOTHER handle of the same weights (a slot): log-mel, encoder, prompt forward, first token of R requests
 *   sonic_splice_rows(d, p, n, src_rows, dst_rows, &seq)   rows src_rows[] of p (KV cache, control words, next-step input) -> free rows
 *                               dst_rows[] of d, queued on d's stream between two chunks; p may start its next prefill at once (it waits for the
 *                               copies on the device).  seq = chunks d had queued before: checks with a larger number describe the new occupants
 *   sonic_service_step(d, k, rows, finished[64], n_new[64], &seq, &n_active)   queue k more chunks (k * decode_chunk token steps for rows
 *                               0 .. rows-1 rounded up to 16; rows = 0: all - the caller names the highest occupied row + 1, so a lightly loaded
 *                               pool steps faster) and return the newest completed check: finished[r] = 1 once row r hit EOS / its budget (or is
 *                               free), n_new[r] its tokens
 *   sonic_fetch_row(d, row, n, ids)   the n tokens of a finished row; the row is free again
 *   sonic_fetch_rows(d, n, rows, counts, ids, ld)   the same for n finished rows in one call (row i's tokens at ids + i * ld)
 * A request's tokens are the same bits as in a solo run (rows are independent in every decode kernel; tests/test_gpu_continuous.py). */
SONIC_API int sonic_service_begin(sonic_engine* d);
SONIC_API int sonic_service_end(sonic_engine* d);
SONIC_API int sonic_splice_rows(sonic_engine* d, sonic_engine* p, int n, const int32_t* src_rows, const int32_t* dst_rows, int64_t* seq_out);
SONIC_API int sonic_service_step(sonic_engine* d, int n_chunks, int rows, int32_t* finished_out, int32_t* n_new_out, int64_t* seq_out, int32_t* n_active_out);
SONIC_API int sonic_fetch_row(sonic_engine* d, int row, int n, int32_t* out_ids);
SONIC_API int sonic_fetch_rows(sonic_engine* d, int n, const int32_t* rows, const int32_t* counts, int32_t* out_ids, int out_ld);
/* sonic_fetch_rows with both arrays in one call (the fetch releases the rows): row i's log-probabilities at out_lp + i * out_ld, as its ids.
 * sonic_splice_rows refuses a source without option token_logprobs when the destination has it (the first token's value comes from the prefill). */
SONIC_API int sonic_fetch_rows_lp(sonic_engine* d, int n, const int32_t* rows, const int32_t* counts, int32_t* out_ids, int out_ld, float* out_lp);

/* Request-level scheduling for live traffic as native threads (csrc/dispatch.cpp): what the reference does with one `await
 * transcribe()` per partial / final of every WebSocket session (backend/connection_manager.py:127-245, backend/transcription_manager.py:19-65) and
 * three executor threads in file mode (backend/main.py:429-445, 616-624), all serialised on one model object.  decoders: handles that decode
 * continuously over their max_batch rows (sonic_service_begin is called on them); prefills: handles that run log-mel + encoder + prompt forward +
 * first token of whatever is queued - as many requests as the emptiest decoder has free rows - and hand the rows over; all handles share one
 * weight copy.  A request is W windows (host PCM, or slices of device rings: see sonic_stage_mixed), a prompt and a budget; it joins a running loop
 * between two chunks and leaves the moment it hits EOS / its budget.  Tokens equal the solo run's bit for bit (decode rows are independent). */
typedef struct sonic_dispatch sonic_dispatch;
struct sonic_ring;
SONIC_API int sonic_dispatch_create(sonic_engine* const* decoders, int n_dec, sonic_engine* const* prefills, int n_pre, int adaptive_tiles, sonic_dispatch** out);
/* One request, whole: its audio, its prompt and budget, and the values it brings of its own.  All-zero is "none" for every value: a zeroed record with size, the
 * audio, the prompt and the budget filled in is a plain greedy request.  The submit copies everything before it returns.  A value is refused (SONIC_ERR_INVALID, the
 * calling thread's sonic_last_error(NULL) starting with the value's name) unless every handle of the dispatcher has the value's option on, and when it is invalid. */
typedef struct sonic_dispatch_request {
    int64_t size;                                /* sizeof(sonic_dispatch_request) as the caller compiled it: refused unless it is the library's */
    /* the audio, W >= 1 windows.  Window w: host samples host_pcm[host_off[w] .. host_off[w + 1]) (int16, already peak-normalised over the request, as sonic_stage_pcm
     * takes them; 0 == host_off[0] <= ... <= host_off[W]) when rings or rings[w] is NULL, else samples [ring_start[w], ring_start[w] + ring_n[w]) of rings[w] (raw
     * wire PCM, normalised on the device over the request's windows) */
    const int16_t* host_pcm; const int64_t* host_off;
    struct sonic_ring* const* rings; const int64_t* ring_start; const int32_t* ring_n;
    int32_t W;
    const int32_t* prompt_ids; int32_t prompt_len;
    int32_t max_new;
    /* "request_bias:" its sequence-bias table, n_seq entries in sonic_set_request_bias's form for one request; n_seq = 0: none */
    const int32_t* seq_ids; const int32_t* seq_off; const float* bias; int32_t n_seq;
    /* "sampling:" sampled != 0: it draws under (temperature, seed) as a request of sonic_set_request_sampling; 0: greedy, the two are not read */
    int32_t sampled; float temperature; uint64_t seed;
    /* "truncation:" cut != 0: its draws are cut by (top_k, top_p, min_p), a row of "request_truncation" (top_k an integer value); only beside sampled */
    int32_t cut; float top_k, top_p, min_p;
    /* "grammar:" 0: none, else the id of a live grammar ("grammar:<id>") of the dispatcher's weight owner */
    int32_t grammar_id;
    /* "draft:" its draft (option draft_verify), n_draft ids that fit the vocabulary and the budget (n_draft <= max_new - 1) and are neither the audio placeholder
     * nor an EOS id; n_draft = 0: none.  A drafted request carries no table, temperature > 0 or grammar */
    const int32_t* draft_ids; int32_t n_draft;
} sonic_dispatch_request;
SONIC_API int sonic_dispatch_submit(sonic_dispatch* d, const sonic_dispatch_request* r, int64_t* ticket_out);
SONIC_API int sonic_dispatch_cancel(sonic_dispatch* d, int64_t ticket);                 /* queued requests only */
/* next completed request in completion order; blocks up to timeout_ms (< 0: until one completes or the dispatcher is closed and drained); *ticket_out = 0: none */
SONIC_API int sonic_dispatch_next(sonic_dispatch* d, int timeout_ms, int64_t* ticket_out, int32_t* status_out, int32_t* out_ids, int out_cap, int32_t* n_out,
                                  char* err, int err_cap);
/* sonic_dispatch_next plus the log-probabilities of the completed request (out_lp[i] belongs to out_ids[i]; at most out_cap are copied).  Every handle of
 * the dispatcher needs option token_logprobs: SONIC_ERR_INVALID otherwise, err naming the option. */
SONIC_API int sonic_dispatch_next_lp(sonic_dispatch* d, int timeout_ms, int64_t* ticket_out, int32_t* status_out, int32_t* out_ids, int out_cap, int32_t* n_out,
                                     char* err, int err_cap, float* out_lp);
SONIC_API int sonic_dispatch_stats(sonic_dispatch* d, int64_t* prefill_batches, int64_t* decode_chunks, int32_t* load_windows, int32_t* free_rows);
SONIC_API int sonic_dispatch_close(sonic_dispatch* d);     /* queued requests fail, running ones complete (still collectable); handles leave continuous mode */
SONIC_API int sonic_dispatch_destroy(sonic_dispatch* d);

/* Device-resident ingest.  A ring holds the raw wire PCM of one streaming session in HBM: what the reference keeps as
 * 2048-byte chunks in a host dict (backend/audio_manager.py:21-33, fed from backend/main.py:813-842) and concatenates on the host for
 * every partial / final decode (audio_manager.py:99-123).  A decode names sample ranges of rings instead of handing over host buffers;
 * the reference's conversions between the wire and the feature extractor -- int16 -> float32 / 32768
 * (backend/transcription_manager.py:45-54), peak normalisation over the request and the PCM_16 round trip (backend/asr.py:247-276) --
 * run on the device, bit-identical with the host path.  Appends use the ring's own stream and lock: they do not wait for a batch that
 * is decoding.  A ring belongs to the engine it was created on; sonic_destroy frees the rings that are still alive (their handles
 * are dead after that). */
typedef struct sonic_ring sonic_ring;
SONIC_API int sonic_ring_create(sonic_engine* e, int64_t capacity_samples, sonic_ring** out);
SONIC_API void sonic_ring_destroy(sonic_ring* r);
/* append n samples (any chunk size <= capacity); *first_index = absolute sample index of pcm[0].  Returns at once: the samples are
 * copied to a pinned mirror and their H2D copy is queued; decodes that name them order behind it */
SONIC_API int sonic_ring_append(sonic_ring* r, const int16_t* pcm, int64_t n, int64_t* first_index);
SONIC_API int64_t sonic_ring_head(sonic_ring* r);     /* samples appended so far */
/* Rings at any input rate (ABI 11).  A ring made by sonic_ring_create_rate takes, in sonic_ring_append, samples at in_rate; a polyphase
 * windowed-sinc kernel (csrc/resample.hip: torchaudio's sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) writes them into the ring
 * as 16 kHz int16, q = clip(rint(y * 32768)).  capacity_samples, the ring's content, its indices, sonic_ring_head, *first_index and every
 * reader stay in 16 kHz samples; *first_index is the head before the call and the head after it tells how many outputs the chunk made
 * (possibly none).  With of = in_rate / g, nf = 16000 / g, width = ceil(6 * of / (min(of, nf) * 0.99)): after N input samples in total the ring
 * holds the outputs j < nf * (floor((N - width - of) / of) + 1) (0 for N < width + of) - the frames whose taps all exist - and keeps the input
 * samples the next frames still need on the device.  An output's bits do not depend on how the stream was cut into appends.  A chunk whose
 * outputs exceed the capacity is refused.  in_rate == 16000 gives exactly the ring of sonic_ring_create.  Refused (SONIC_ERR_INVALID, the
 * message names the numbers): in_rate <= 0, and rates whose coefficient bank nf * (2 * width + of) exceeds 2^22 entries (16001 Hz).  The bank
 * is built once per rate pair, in double, rounded to fp32, and shared by every ring and slot of the engine.
 * sonic_ring_flush ends the stream: it emits the remaining outputs up to ceil(nf * N / of) with zeros beyond the last sample; the next
 * append starts a new stream without history.  It does nothing on a 16 kHz ring.
 * sonic_ring_read copies the ring samples [first, first + n) to the host, behind every append so far; the range rule is that of
 * sonic_stage_mixed.  Appends, flushes and reads report failures through sonic_last_error(NULL) of the calling thread. */
SONIC_API int sonic_ring_create_rate(sonic_engine* e, int64_t capacity_samples, int32_t in_rate, sonic_ring** out);
SONIC_API int sonic_ring_flush(sonic_ring* r);
SONIC_API int sonic_ring_read(sonic_ring* r, int64_t first, int64_t n, int16_t* out_i16);
/* One-shot resampler over a whole host buffer of n samples (exactly one of pcm_i16 - taken as s / 32768 - and pcm_f32 is given), zeros
 * beyond both ends: *n_out = ceil(nf * n / of) fp32 outputs, the same bits the rate ring rounds.  out_f32 == NULL asks for *n_out only.
 * Takes its own lock and stream, never the engine's batch lock: it does not queue behind a decode.  Errors: sonic_last_error(NULL). */
SONIC_API int sonic_resample(sonic_engine* e, const int16_t* pcm_i16, const float* pcm_f32, int64_t n, int32_t in_rate, int32_t out_rate,
                             float* out_f32, int64_t out_cap, int64_t* n_out);
/* sonic_pipeline_submit with the windows of sonic_stage_mixed: window w is a range of ring rings[w] (raw wire PCM, a1 + a2 on the device,
 * peak over the windows of its request) or, where rings[w] is NULL, host PCM as in sonic_pipeline_submit.  The ring arrays are copied; the
 * ranges are checked, and the rings locked, when a prefill thread stages the batch (a range that has left its ring by then fails the batch
 * with sonic_stage_mixed's message).  File mode submits its segments this way on a bulk model (backend/main.py:429-445). */
SONIC_API int sonic_pipeline_submit_mixed(sonic_pipeline* p, const int16_t* host_pcm, const int64_t* host_off, sonic_ring* const* rings,
                                          const int64_t* ring_start, const int32_t* ring_n, int W, const int32_t* req_win, int R,
                                          const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new,
                                          int32_t* out_ids, int out_ld, int32_t* out_len, int64_t* ticket_out);
/* sonic_pipeline_submit_mixed (rings may be NULL: host windows only) plus out_lp [R][out_ld]: token i of request r gets its log-probability at
 * out_lp[r * out_ld + i] (the same out_ld as out_ids); it stays valid until the ticket has been waited for.  Needs option token_logprobs on every
 * handle of the pipeline: SONIC_ERR_INVALID otherwise, sonic_pipeline_last_error naming the option. */
SONIC_API int sonic_pipeline_submit_lp(sonic_pipeline* p, const int16_t* host_pcm, const int64_t* host_off, sonic_ring* const* rings,
                                       const int64_t* ring_start, const int32_t* ring_n, int W, const int32_t* req_win, int R,
                                       const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new,
                                       int32_t* out_ids, int out_ld, int32_t* out_len, float* out_lp, int64_t* ticket_out);
/* sonic_transcribe_batch with every window either host samples (rings == NULL or rings[w] == NULL: int16 PCM already peak-normalised,
 * host_off[W+1]; ring windows have empty host ranges) or samples [ring_start[w], ring_start[w] + ring_n[w]) of rings[w], which must
 * still be inside the ring's last `capacity` samples.  The windows of one request (req_win) share one peak.  Without req_win R == W. */
SONIC_API int sonic_transcribe_mixed(sonic_engine* e, const int16_t* host_pcm, const int64_t* host_off, sonic_ring* const* rings,
                           const int64_t* ring_start, const int32_t* ring_n, int W, const int32_t* req_win, int R,
                           const int32_t* prompt_ids, const int64_t* prompt_off, const int32_t* max_new,
                           int32_t* out_ids, int out_ld, int32_t* out_len, float* step_logits);
/* the staging half alone (then sonic_run_staged / sonic_fetch_tokens) */
SONIC_API int sonic_stage_mixed(sonic_engine* e, const int16_t* host_pcm, const int64_t* host_off, sonic_ring* const* rings,
                      const int64_t* ring_start, const int32_t* ring_n, int W, const int32_t* req_win, int R);

/* Teacher forcing (parity tests; mirrors the oracle's force_ids): while set, token n of request r is ids[r * ld + n] instead of
 * the argmax -- logits are still computed and returned, EOS / budget rules apply to the forced token (HF:generation/utils.py:2925-2936
 * with next_tokens replaced).  ids == NULL clears.  Forced runs use the eager decode loop.
 *
 * The parallel forced run (scoring given transcripts; options "forced_parallel", "forced_fanout", "score_chunk_rows").  Under teacher forcing no
 * input depends on an output, so while option "forced_parallel" is 1 AND forced ids are set, a run through sonic_transcribe_batch, sonic_transcribe_mixed,
 * sonic_run_staged or sonic_run_staged_async is computed as ONE prefill pass instead of the eager loop: sequence r is its prompt followed by
 * ids[r][0 .. L_r - 1), where L_r = 1 + the index of the first EOS id among ids[r][0 .. max_new[r]), or max_new[r] if there is none (the rule above); the tied lm_head
 * runs over all forced positions as one GEMM per chunk of "score_chunk_rows" rows (16 .. 4096, default 256), and a row kernel takes log_softmax(logits)[ids[r][n]] of
 * every position.  Only ids[r][0 .. L_r) is read: pad rows with any valid id.  With the option 0, or without forced ids, the engine launches exactly what it did.
 *   results, through the existing calls: out_ids[r][0 .. L_r) are the forced ids and out_len[r] = L_r; sonic_fetch_logprobs returns the records in its layout
 *   (1 + 2K floats per token with option top_logprobs = K: the forced token's log-probability, the K best ids of that position by (score descending, id ascending)
 *   with their log-probabilities, formed from the same maximum and sum) and needs option token_logprobs, as ever; step_logits [n][r][V] are returned if asked, rows
 *   n >= L_r of a request are not written; sonic_get_timings fills mel / encoder / prefill as for a run whose decode loop took no step.  The handle then holds
 *   a finished batch: sonic_decode_step reports 0 active rows, and the next run may follow at once.
 *   NO logits processor is applied, whatever the handle carries: the parallel run scores the RAW model distribution at temperature 1 - HF's
 *   compute_transition_scores over `logits`, not over `scores`.  With generation guards active this is the one difference from the step-by-step forced run.
 *   Tables of sonic_set_request_bias or values of sonic_set_request_sampling staged for such a run are refused (SONIC_ERR_INVALID) and consumed.
 *   "forced_fanout" = N (1 .. max_batch, default 1; read as a parallel run starts): the call's R sequences are R / N audio requests with N candidate sequences
 *   each - sequence r takes its audio rows from audio request r / N, req_win has R / N + 1 entries (NULL: W == R / N), and log-mel, encoder and projector run once
 *   per audio request.  R not divisible by N: SONIC_ERR_INVALID.  Each sequence prefills its own prompt; only the encoder is shared.
 *   "forced_share_prompt" = 1 (default 0; read as a parallel run starts; adds no entry point and no struct): the N sequences of a group also share ONE
 *   prefill of their prompt.  The first sequence of a group is packed as ever, prompt || ids[0 .. L - 1), in its cache row; every other one packs only ids[0 .. L - 1)
 *   (L - 1 rows at positions P .. P + L - 2 of its own cache row; none for L = 1), and its attention reads keys [0, P) from the first one's row.  Token 0 of every
 *   sequence of a group is scored from the first one's hidden row P - 1, token n >= 1 from the sequence's own row.  The run counts A * P + sum(L_r - 1) tokens against
 *   one prefill where it counted sum(P + L_r - 1); results, the EOS rule and R <= max_batch are what they were, rows end with kv_len = P + L - 1.  Not bit-equal to the
 *   unshared form (the attention's key tiles differ).  Refusals (SONIC_ERR_INVALID naming forced_share_prompt): set without "forced_parallel" (which can then not be
 *   switched off), on an int8 handle, on the fp32 kind, beside "forced_align" (either way round), while the handle has work in hand; at the run, the sequences of a
 *   group bringing different prompt ids (the message names the first two that differ).  Slots copy it.  sonic_debug_read "score_tokens" (1 value): the packed tokens
 *   of the handle's last parallel forced run, in either form.
 *   test hook: sonic_load_tensor "share_prompt.hook" (int32 [2][B]: pre_row | pre_len) arms the next sonic_test_prefill_attention on the handle: sequence b's keys
 *   [0, pre_len[b]) are then those of cache row pre_row[b] (0 <= pre_row < B, 0 <= pre_len <= kv_len - q_len), through the builder the run uses.
 *   refusals (SONIC_ERR_INVALID, the message naming the cause): prompts and forced ids together beyond one prefill (the message says how many tokens were asked
 *   and how many fit); the audio placeholder id among the forced ids; and the existing checks (placeholder count, vocabulary, prompt + max_new <= max_ctx).
 *   "forced_parallel" is refused while the handle has work in hand (the rule of sonic_set_generation).  Slots copy it from their owner; it may also be set on a
 *   slot alone.  A handle with the option on is a scoring handle: sonic_prefill, sonic_prefill_enqueue, sonic_service_begin, sonic_splice_rows (as source or
 *   destination), sonic_dispatch_create and sonic_pipeline_create refuse it by name.  Its buffers (the chunk's logits: score_chunk_rows x vocab elements; three
 *   words per score row) come with its first parallel run, are counted by sonic_memory_info and go with the handle.
 *   test hook: on such a handle sonic_test_greedy_lp sends its rows to the row kernel instead - the slabs are summed over ksplit in the greedy kernel's order and
 *   rounded to the element type, those values are the logits row the kernel reads and logits_out returns them; force_ids is required, tok_out holds the forced ids,
 *   lp_out B records of 1 + 2K floats; B may exceed 64 (up to 4096), mpad stays the slab row stride.
 *
 * Word timestamps on the parallel forced run (options "forced_align", "align_head").  While option "forced_align" is 1 a parallel forced run also
 * says WHEN every scored token was spoken: at the selected decoder heads the attention of the score rows onto the audio placeholder keys (softmax over the audio run
 * alone), normalised over the tokens (std = 0: 0), median-filtered (width 7, reflect) and averaged over the heads, then dynamic time warping - openai-whisper's
 * find_alignment, the decoder's self-attention onto the audio run in the place of Whisper's cross-attention.  t_n is the index into sequence r's audio run at which
 * token n starts; one audio token is 1280 samples = 80 ms, and a request of several windows carries its windows' kept rows one after the other.
 *   results: every log-probability record of such a run is W = 1 + 2K + 1 floats - the record above, bit for bit, and t_n as the last float (an index: exact).
 *   sonic_fetch_logprobs' out_ld counts floats and must hold n_new[r] * W of them ("out_ld too small" otherwise).  A run without forced ids on the same handle (a
 *   greedy run) returns records of 1 + 2K floats as ever.  The records need option token_logprobs.
 *   "forced_align" = 1 is accepted only on a handle with "forced_parallel" = 1 (which can then not be switched off), refused on the fp32 kind and while the handle has
 *   work in hand; slots copy it and the heads.  With it 0 the engine launches exactly what it did.
 *   "align_head" = l * 256 + h adds head h of decoder layer l to the selection (at most 256; out of range or a full list: SONIC_ERR_INVALID; a head already in
 *   the list is no error), -1 returns to the default: every head of the last ceil(dec_layers / 2) layers - Whisper's rule for a model without alignment heads.
 *   Heads are added layer by layer, ascending within a layer, without atomics: the same bits on every run, whatever else the run holds.
 *   refusals at the run (SONIC_ERR_INVALID by name): a sequence whose audio placeholders are not ONE contiguous run, or that has none; more than 4000 targets.
 *   buffers (probabilities of one layer's heads, the matrix, the DTW's trace, t_n, the plan) come with the first align run sized to it, grow with a later run that
 *   needs more, are counted by sonic_memory_info and go with the handle.
 *   sonic_debug_read: "align_probs" [heads of the last selected layer][S][A_max] and "align_matrix" [S][A_max] of the last run, fp32 on every kind (S = the run's
 *   score rows, sequence after sequence; A_max = its longest audio run).
 *   test hook: on such a handle sonic_test_attention(q [B][Tq][Hq * 128], k [B][Tk][Hkv * 128], v = NULL, out, B, Tq, Tk, Hq, Hkv, hd = 128, causal = 0) runs the
 *   three kernels on caller data - all Hq heads, the audio run being all Tk keys - and out is [B][Tq][Tk + 1]: the matrix's row, then t_n.
 *
 * Draft-verified decoding (option "draft_verify", sonic_load_tensor "request_draft", sonic_debug_read "draft_accepted"): HF
 * generate()'s assisted / prompt-lookup decoding with the draft brought by the caller - a previous partial of the same audio, a first-pass model, an edited transcript.
 * The engine accepts the longest prefix of the draft that the model itself would have emitted, takes the model's own token at the first disagreement and carries on in
 * the ordinary greedy loop, without leaving the device.  Every emitted token is an argmax of the model's processed scores; a wrong draft costs its prefill rows.  The
 * feature adds no entry point and no struct: it travels as an option, a named int32 "tensor" and a sonic_debug_read name.
 *   "draft_verify" = 1: set on the owner before its slots are created (they copy it).  Refused (SONIC_ERR_INVALID by name) while the handle has work in hand (the
 *   rule of sonic_set_generation); on the int8 kind, whose prefill quantises per request group, so that a draft would change the group; on the fp32 test kind; on a
 *   scoring handle ("forced_parallel", which in turn is refused while this option is on).  With the option off, or on with no draft staged, the engine launches
 *   exactly what it launched before.  The buffers (the chunk's logits of the parallel forced run, score_chunk_rows x vocab elements; five words per draft position
 *   and 4 x 64 per batch; a choice and a log-probability record per position; 64 accepted counts) come with the handle's first drafted prefill, are counted by
 *   sonic_memory_info and go with the handle.
 *   sonic_load_tensor(e, "request_draft", words, SONIC_DTYPE_I32, {n}, 1), words = [R | off[0 .. R] | ids]: the drafts of the R requests of the NEXT prefill on this
 *   handle (the entry points sonic_set_request_bias names), which consumes them on success and on failure alike.  Request r's draft is ids[off[r] .. off[r + 1]);
 *   D_r = off[r + 1] - off[r] may be 0.  SONIC_ERR_INVALID, nothing truncated, the message naming the cause: the option is off; an id outside the vocabulary; an id that
 *   is the audio placeholder or one of the handle's EOS ids; and at the prefill: an R that is not the batch's; D_r > max_new[r] - 1; prompts and drafts together
 *   beyond one prefill (the message says how many tokens were asked for and how many fit); forced ids set on the handle; a drafted request that also carries a bias
 *   table, a temperature > 0 or a grammar (undrafted requests of the same batch may carry them).
 *   A drafted request r with prompt P_r and draft d[0 .. D): the prefill runs over prompt || d, the K/V rows written as a prefill writes them.  Draft position n is
 *   decided from the hidden row at position P - 1 + n: final norm, the tied lm_head as the prefill-family GEMM into the chunk buffer of the parallel forced run
 *   ("score_chunk_rows" rows per launch), one block of rows_kernel per row.  s_n = the row's logits after the handle's processors (sonic_set_generation, HF's
 *   order) with history prompt || d[0 .. n); t_n = the first maximum of s_n (ties: the lower id; all -inf: 0); a_r = the least n with t_n != d[n], or D.  The request
 *   then stands exactly where a prefill of prompt || d[0 .. a) would have left it, with its first a tokens and their log-probability records already written:
 *   out_ids[r][0 .. a) = d[0 .. a); record n = log_softmax(s_n)[d[n]] and, with "top_logprobs" = K, the K alternatives of s_n, in the handle's layout of 1 + 2K
 *   floats; n_new = a, kv_len = P + a, the next position P + a, the step counter a, and the head's row map pointing at hidden row P - 1 + a.  The UNCHANGED head then
 *   produces token a (final norm over that row, the skinny lm_head, the greedy kernel: it appends to the history and applies the EOS and budget rules), and the decode
 *   loop follows - graphs, chunks, continuous scheduler as they are.  K/V rows behind position P + a are stale and never read: decode attention sees kv_len keys, and
 *   the next step overwrites position P + a.
 *   consequences: a request with D = 0 goes through the very kernels of a batch without drafts and keeps its bits, also beside drafted requests.  Token a comes
 *   from the skinny lm_head, the decision at position a from the GEMM: around a near-tie the head may emit d[a] after all - still the model's argmax, under the
 *   step path's rounding.  Accepted tokens carry the prefill path's rounding, not the step loop's (DESIGN.md 6.8 measured max |dlogit| 0.031 between the two), so
 *   near a tie a drafted run may leave the undrafted run's transcript where the two roundings order two ids differently.
 *   want_step_logits: steps 0 .. D_r of a drafted row receive the raw logits of the verify pass (as the parallel forced run dumps its rows); steps from a on are
 *   overwritten by the head and the loop as always.
 *   sonic_debug_read(e, "draft_accepted", 0, out, R): a_r of the handle's last prefill as fp32 values (zeros behind a prefill without drafts); tests and diagnostics.
 *   sonic_splice_rows refuses handles whose "draft_verify" differ, and copies a row's first n_new ids and records - for every row without an accepted draft that is one.
 *   dispatcher: sonic_dispatch_request's draft_ids, n_draft.  With the option on, the prefill batcher counts prompt + draft tokens against one prefill's capacity.
 *   sonic_pipeline_create refuses a handle with the option on, by name.
 *   test hook: on such a handle sonic_test_greedy_guard WITH force_ids sends its rows to rows_kernel (its choosing instantiations) - the slabs become the logits row as on a scoring handle;
 *   row b is one draft position with history hist[b][0 .. hist_len[b]) and draft id force_ids[b]; tok_out[b] = t, lp_out B records of 1 + 2K floats; neutral guard
 *   values launch the unguarded instantiation; B may exceed 64 (up to 4096). */
SONIC_API int sonic_set_forced_ids(sonic_engine* e, const int32_t* ids, int R, int ld);
SONIC_API int sonic_get_timings(sonic_engine* e, sonic_timings* out);
SONIC_API int sonic_synchronize(sonic_engine* e);

/* ---- single-kernel test hooks (host fp32 in/out, converted to bf16 on device; used by tests/ only) ---- */
SONIC_API int sonic_test_gemm(sonic_engine* e, const float* A, const float* W, const float* bias, const float* resid, float* C,
                    int M, int N, int K, int epi);
/* The GEMM form hook: one MFMA GEMM in a launch form production uses, on the handle's own type (bf16, fp16, or int8 through the Linear8bitLt path).  It adds no entry
 * point: like the language-model hooks it travels as named "tensors" of sonic_load_tensor and names of sonic_debug_read (a 16-bit or int8 handle; any state of its weights).
 *   stage    sonic_load_tensor "gemm.form:A" / ":W" / ":bias" / ":resid" / ":rope" / ":C" / ":Vt", SONIC_DTYPE_F32, ndim 1 (shape {0}: drops it): fp32 values of the element type
 *   run      sonic_load_tensor "gemm.form.run", SONIC_DTYPE_I32, ndim 1: the words of one sonic_gemm_form record (all-zero = the dense form of sonic_test_gemm, `size` set
 *            as in sonic_dispatch_request).  Refused by name (SONIC_ERR_INVALID) when the record contradicts itself or a staged buffer has another size than it asks for.
 *            The run consumes A, W, bias, resid and rope; C and Vt stay, holding what the launch left
 *   read     sonic_debug_read "gemm_form_c" / "gemm_form_vt" (a prefix of the buffer); "gemm_route" (n = 4 or 5): the route of the calling thread's last launch_gemm, host
 *            only - rows on the 256x256 tile, rows on the 128x128 kernel, that kernel's launch shape 0 / 1 / 2, the CU count the decision used; both row counts
 *            non-zero: the ragged-tail split; a fifth value: whether the thread's last int8 linear armed the deferral of long outlier lists.  The GEMM tests
 *            assert the kernel they mean to test from it.
 *   A      flat, (batch - 1) * strideA + (M - 1) * lda + K elements (conv forms: the padded [W][rows + 2][ch] buffer; lda < K = overlapping rows)
 *   W      [N][K] row-major; w_tiled: tiled on the device by launch_tile_weights (int8: launch_tile_weights_i8 of the quantised codes), gu8 (EPI_SWIGLU, w_tiled):
 *          by launch_tile_weights_gu8 from the 16-row-interleaved gate/up matrix
 *   C      in-out, c_row_offset * ldc + (batch - 1) * strideC + (M + 8) * ldc elements: uploaded, the GEMM writes at row c_row_offset of every batch, all read back
 *   resid  [M][ldr] for EPI_BIAS_RESID; resid_in_place: R = C (the residual is what the caller put into C), no resid staged
 *   EPI_QKV_VT (4): columns < n_split -> C (ldc), the rest transposed per segment of seg_T rows into Vt [ceil(M / seg_T)][N - n_split][vt_ld], in-out like C;
 *          rope [seg_T][32] cos | sin with rope_ncols: fused into the epilogue exactly when the encoder would (256x256 tile, not under no_fused_rope / gemm_force128).
 *          int8: the Linear8bitLt q|k|v of the encoder, asked for C [M + 8][N] (ldc = N) as run_encoder asks - when the engine fuses, columns < n_split come back
 *          rotated, the V columns untouched and V^T in Vt; else all N columns plain and Vt untouched (the caller runs the two passes)
 *   int8   X in groups of group_rows rows (0: one group), batch <= 1 */
typedef struct sonic_gemm_form {
    int32_t size;                                /* sizeof(sonic_gemm_form) as the caller compiled it */
    int32_t M, N, K, epi;
    int32_t lda, ldc, ldr;                       /* 0: dense (K, the output width, the output width) */
    int32_t batch, strideA, strideC, c_row_offset;
    int32_t w_tiled, gu8;
    int32_t resid_in_place;
    int32_t n_split, seg_T, vt_ld, rope_ncols;
    int32_t group_rows;
    int32_t gelu_arith;                          /* EPI_BIAS_GELU, 16-bit: launch without the GELU table, as the conv stem does */
} sonic_gemm_form;
SONIC_API int sonic_test_skinny(sonic_engine* e, const float* X, const float* W, float* C, int M, int N, int K);
SONIC_API int sonic_test_skinny_gu(sonic_engine* e, const float* X, const float* Wgu_interleaved, float* act, int M, int N, int K);
/* the argmax + greedy controller on caller-provided lm_head partial slabs [ksplit][mpad][V] fp32: token picked per row
 * (first maximum of the bf16-rounded slab sum) and optionally the bf16 logits [B][V] it compared */
/* one Linear8bitLt call (backend/asr.py:182-198: bnb.nn.Linear8bitLt(has_fp16_weights=False, threshold=6.0)) through the engine's int8
 * kernels: W [N][K] quantised row-wise on the device, X [M][K] in groups of group_rows rows (one group = one reference call), int8 MFMA
 * GEMM + dequantising epilogue epi.  fp32 buffers holding fp16 values.  Needs an engine created with SONIC_MODE_INT8. */
SONIC_API int sonic_test_linear_int8(sonic_engine* e, const float* X, const float* W, const float* bias, const float* resid, float* out,
                           int M, int N, int K, int group_rows, int epi);
SONIC_API int sonic_test_greedy(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, int32_t* tok_out, float* logits_out);
/* sonic_test_greedy through the log-probability instantiation of the kernel (greedy_kernel<T, true>): tok_out / logits_out as above, lp_out[B] = the
 * log-probability of the token each row emits; force_ids (optional, [B]): that token instead of the argmax, as under sonic_set_forced_ids */
SONIC_API int sonic_test_greedy_lp(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* force_ids, int32_t* tok_out,
                                   float* logits_out, float* lp_out);
/* the same launch through the guard instantiation (greedy_kernel<T, LP, true>): row b decides with the history hist[b * hist_ld .. + hist_len[b]) and the three
 * parameters of sonic_set_generation; logits_out stays the raw logits, lp_out (optional) is over the processed scores, force_ids (optional) as above */
SONIC_API int sonic_test_greedy_guard(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* hist, int hist_ld, const int32_t* hist_len,
                                      float repetition_penalty, int no_repeat_ngram_size, const int32_t* suppress, int n_suppress, const int32_t* force_ids,
                                      int32_t* tok_out, float* logits_out, float* lp_out);
/* the same launch through the bias instantiation (greedy_kernel<T, LP, true, true>): sonic_test_greedy_guard's arguments plus the B rows' tables in
 * sonic_set_request_bias's packed form (req_off[B + 1]) */
SONIC_API int sonic_test_greedy_bias(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* hist, int hist_ld, const int32_t* hist_len,
                                     float repetition_penalty, int no_repeat_ngram_size, const int32_t* suppress, int n_suppress, const int32_t* force_ids,
                                     const int32_t* seq_ids, const int32_t* seq_off, const float* bias, const int32_t* req_off,
                                     int32_t* tok_out, float* logits_out, float* lp_out);
/* the same launch through the sampling instantiations (greedy_kernel<T, true, GUARD, BIAS, true>) in the handle's own type: hist_len = NULL: the plain family (the
 * guard arguments are ignored); hist_len without req_off: the guard family; both: the bias family.  Row b draws with temperature[b] and seed[b] as its step[b]-th
 * token (0 .. 65535).  lp_out is required (log_softmax over the processed scores at temperature 1); noise_out[B][V] (may be NULL) receives the Gumbel value the
 * kernel added at every id of a row with temperature > 0 and stays 0 for the others. */
SONIC_API int sonic_test_greedy_sample(sonic_engine* e, const float* slabs, int ksplit, int mpad, int V, int B, const int32_t* hist, int hist_ld, const int32_t* hist_len,
                                       float repetition_penalty, int no_repeat_ngram_size, const int32_t* suppress, int n_suppress, const int32_t* force_ids,
                                       const int32_t* seq_ids, const int32_t* seq_off, const float* bias, const int32_t* req_off,
                                       const float* temperature, const uint64_t* seed, const int32_t* step,
                                       int32_t* tok_out, float* logits_out, float* lp_out, float* noise_out);
/* the grammar instantiations (greedy_kernel<T, true, true, BIAS, SAMPLE, TOPK, true>) ride on the three hooks above: an automaton armed on the handle - sonic_load_tensor
 * "grammar.hook:<V>" (the packed words of a grammar, validated against V), then options hook_grammar_state = row << 20 | (state + 2) and hook_grammar_eos = id - is taken
 * by the next of these launches that has histories and lp_out, in the handle's own type; sonic_debug_read "hook_grammar_state" returns the rows' states afterwards. */
SONIC_API int sonic_test_attention(sonic_engine* e, const float* q, const float* k, const float* v, float* out,
                         int B, int Tq, int Tk, int Hq, int Hkv, int hd, int causal);
SONIC_API int sonic_test_decode_attention(sonic_engine* e, const float* q, const float* k, const float* v, float* out,
                                int B, int Tk, int Hq, int Hkv);
/* the decode attention as the decode step launches it, over caller-filled caches [B][Hkv][ctx_max][128] (the caller decides what lies behind kv_len) and
 * per-row kv_len[B] in 1..ctx_max (new token included).  Fused mode (slabs != NULL, q == NULL): q|k|v partial slabs [ksplit][mpad][(Hq + 2 Hkv) * 128] fp32
 * (ksplit 1..8, mpad >= B) and the RoPE table rope_cs [ctx_max][128] fp32 (cos | sin); the kernel sums the slabs, applies RoPE at kv_len - 1 and appends the
 * K / V row.  Given-q mode (q != NULL, slabs == NULL): q [B][Hq * 128], nothing appended.  out [B][Hq * 128]; kcache_out / vcache_out (optional) receive the
 * caches as the launch left them.  Hq / Hkv <= 4.  The int8 dequantising prologue is reached through sonic_test_decode_i8_attn. */
SONIC_API int sonic_test_decode_attention_cache(sonic_engine* e, const float* q, const float* slabs, int ksplit, int mpad, const float* rope_cs,
                                      const float* kcache, const float* vcache, const int32_t* kv_len, float* out, float* kcache_out, float* vcache_out,
                                      int B, int Hq, int Hkv, int ctx_max);
/* the prefill's causal attention (head dim 128) with its own strides: packed q [n_tok][Hq * 128] with q_off / q_len / kv_len [B] (1 <= q_len <= kv_len <=
 * ctx_max: query t of a sequence sits at position kv_len - q_len + t), K [B][Hkv][ctx_max][128], V^T [B][Hkv][128][ctx_max], ctx_max a multiple of 64.
 * out [n_tok][Hq * 128] is read first: rows outside every [q_off, q_off + q_len) come back as they went in. */
SONIC_API int sonic_test_prefill_attention(sonic_engine* e, const float* q, const float* kcache, const float* vt, const int32_t* q_off, const int32_t* q_len,
                                 const int32_t* kv_len, float* out, int n_tok, int B, int Hq, int Hkv, int ctx_max);
/* the decode step's and the prefill's glue kernels, one launch each, on caller-made data (fp32 buffers holding element-type values; 16-bit engines only; every
 * shape and index is checked before the launch).  x / y / resid / qk and the three caches are in-out: uploaded, then read back.  csrc/engine_hooks.cpp has the layouts.
 *   sonic_test_add_rmsnorm   x[r] += sum of slabs [ksplit][mpad][d], y[r] = RMSNorm(x[r]) * w for r < rows <= rows_alloc; d % 8 == 0, d <= 2048, ksplit 1..8, mpad >= rows.
 *                            q_out != NULL (fp16 engine): also the row quantised for a Linear8bitLt - q [rows][d], sca / oc_cnt [rows], oc_list / oc_val [rows][d]
 *   sonic_test_quant_rows    the same five outputs for X [M][ld] (first K columns; fp16 engine; K % 8 == 0, K <= 8192, ld % 8 == 0)
 *   sonic_test_swiglu_slab   gate / up slabs [ksplit][mpad][2 ff], columns interleaved in groups of 16 (gu8 = 0) or 8 (gu8 = 1) -> act [rows][ff]
 *   sonic_test_decode_o_gu   o_proj + residual -> RMSNorm -> gate/up + SwiGLU; form 0 fused (default step), 1 split norm (rmsnorm_ss), 2 unfused (slabs + add_rmsnorm);
 *                            shapes as skinny_o_eligible / skinny_gu_eligible accept them; hn_out [M][D] for forms 1, 2; ss_out (optional, forms 0, 1) [2][D / 64][32][4]
 *   sonic_test_rope_append   prefill RoPE + K / V / V^T append, tiled = 1 per 16-position tile, 0 per token; sequence b = tokens q_off[b] .. + q_len[b] at positions 0 ..
 *   sonic_test_rope_enc      encoder partial RoPE in place on qk [M][ld], table row m mod T */
SONIC_API int sonic_test_add_rmsnorm(sonic_engine* e, float* x, const float* slabs, int ksplit, int mpad, const float* w, float eps, float* y, int rows, int rows_alloc, int d,
                                     int8_t* q_out, float* sca_out, int32_t* oc_cnt_out, int32_t* oc_list_out, float* oc_val_out);
SONIC_API int sonic_test_quant_rows(sonic_engine* e, const float* X, int M, int K, int ld, int8_t* q_out, float* sca_out, int32_t* oc_cnt_out, int32_t* oc_list_out, float* oc_val_out);
SONIC_API int sonic_test_swiglu_slab(sonic_engine* e, const float* slabs, int ksplit, int mpad, int ff, int rows, int gu8, float* act);
SONIC_API int sonic_test_decode_o_gu(sonic_engine* e, const float* att, const float* Wo, float* resid, const float* ln_w, float eps, const float* Wgu, int form,
                                     int M, int K, int D, int ff, int rows_alloc, float* hn_out, float* act_out, float* ss_out);
SONIC_API int sonic_test_rope_append(sonic_engine* e, const float* qkv, const float* cs, const int32_t* tok_seq, const int32_t* tok_pos, const int32_t* q_off, const int32_t* q_len,
                                     int n_tok, int B, int Hq, int Hkv, int ctx_max, int vt_ld, int tiled, float* q_out, float* Kc, float* Vc, float* Vt);
SONIC_API int sonic_test_rope_enc(sonic_engine* e, float* qk, int M, int ld, int T, int heads2, int hd, int rd, const float* cs);
/* the int8 token step's dequantising consumers, each behind one decode-flavour Linear8bitLt run as the step runs it (int8 engines only; X [M][K] and W [N][K] are fp32
 * holding fp16 values, 1 <= M <= 64; W is quantised, tiled and - layout 1 - also transposed into the k-major copy on the device; N, K as the int8 skinny GEMM takes them).
 * info_out (optional) [2] = ksplit as launched, the GEMM's tiling 0 .. 4; slab_sum_out (optional) int32 [M][N] = the int32 slabs summed.  csrc/engine_hooks.cpp has the layouts.
 *   sonic_test_decode_i8_norm    o_proj / down_proj + add_rmsnorm with a DeqInfo and a QuantOut: x, y [rows_alloc][N] in-out, N <= 2048; form 0 quantises the rows first and
 *                                lists their outliers, form 1 (the step's default) hands the GEMM the rows' absmax partials amax [M][4] and the consumer those and the counts
 *                                big [M][4] of their elements >= 6.0 (K <= 32 x the consumer's block size); the five quantiser outputs of y as sonic_test_add_rmsnorm's
 *   sonic_test_decode_i8_swiglu  gate/up (W [2 ff][K], rows interleaved in groups of 16) + swiglu_quant: act [rows_alloc][ff] in-out, ff <= 8192, and its five quantiser outputs
 *   sonic_test_decode_i8_attn    q|k|v (X [B][D]) + the fused decode attention with the DeqInfo; caches, rope_cs, kv_len as sonic_test_decode_attention_cache; Hkv <= 4;
 *                                amax / big [B][4] in-out: the per-kv-head partials of the output rows' absmax without the elements >= 6.0, and their counts */
SONIC_API int sonic_test_decode_i8_norm(sonic_engine* e, const float* X, const float* W, float* x, const float* norm_w, float eps, float* y, const float* amax, const int32_t* big,
                                        int M, int N, int K, int rows_alloc, int form, int layout,
                                        int8_t* q_out, float* sca_out, int32_t* oc_cnt_out, int32_t* oc_list_out, float* oc_val_out, int32_t* info_out, int32_t* slab_sum_out);
SONIC_API int sonic_test_decode_i8_swiglu(sonic_engine* e, const float* X, const float* W, float* act, int M, int ff, int K, int rows_alloc, int layout,
                                          int8_t* q_out, float* sca_out, int32_t* oc_cnt_out, int32_t* oc_list_out, float* oc_val_out, int32_t* info_out, int32_t* slab_sum_out);
SONIC_API int sonic_test_decode_i8_attn(sonic_engine* e, const float* X, const float* Wqkv, const float* rope_cs, const float* kcache, const float* vcache, const int32_t* kv_len,
                                        float* amax, int32_t* big, float* out, float* kcache_out, float* vcache_out, int B, int D, int Hq, int Hkv, int ctx_max, int layout,
                                        int32_t* info_out, int32_t* slab_sum_out);
SONIC_API int sonic_test_layernorm(sonic_engine* e, const float* x, const float* w, const float* b, float* y, int rows, int d, float eps, int rms);
/* times `iters` launches of the encoder's dominant GEMM shape on the engine stream with HIP events */
SONIC_API int sonic_bench_gemm(sonic_engine* e, int M, int N, int K, int epi, int iters, float* ms_per_launch);
/* times the decode-step skinny GEMM (variant: 0 LDS-DMA nt, 1 LDS-DMA default policy, 2 registers nt, 3 registers plain, 9 pure-read floor) */
SONIC_API int sonic_bench_skinny(sonic_engine* e, int M, int N, int K, int variant, int iters, float* us_per_launch);
/* debug read-back of an internal bf16 activation buffer as fp32 ("prefill_tap" with index = 0 (embeddings) .. dec_layers,
 * "pe", "dx", "dqkv", "dq", "datt", "dact", "enc_x"; "align_probs", "align_matrix": fp32 buffers of the last align run, see sonic_set_forced_ids; "draft_accepted": the accepted counts of the last prefill, see there; "kcache" / "vcache" with index = decoder layer: the KV cache [max_batch][kv heads][max_ctx][head_dim]; "fork_ms", see sonic_load_tensor;
 * mode fp8 (option "fp8_weights"): "fp8_step_builds" (n = 1: token steps built in the fp8 form since the option was set), "fp8_scales" / "fp8_matrix" with index = layer * 4 +
 * {0 q|k|v, 1 o_proj, 2 gate/up, 3 down_proj} or 4 * dec_layers for the lm_head: the rows' scales, and a prefix of the e4m3 copy as fp32 scale * code, row-major in the
 * row order of the tiled copy); tests / diagnostics only */
SONIC_API int sonic_debug_read(sonic_engine* e, const char* name, int index, float* out, int64_t n);
/* diagnostics: in-kernel timestamps (100 MHz device wall clock) of the decode kernels of one decoder layer, recorded while the option
 * "ktrace" = layer index is set: out[slot][block < 512][8 points], slots 0 qkv, 1 attention, 2 o_proj, 3 gate/up, 4 down */
SONIC_API int sonic_debug_ktrace(sonic_engine* e, int64_t* out, int64_t n);
/* per-engine experiment knobs: "skinny_variant", "gemm_force128", "gemm256_stagger", "prefill_taps", "no_fused_gu",
 * "no_graph" (eager decode loop), "decode_chunk" (token steps per hipGraph launch = granularity of the early-stop check and of row splices, default 2),
 * "decode_lookahead" (start value of the adaptive queue depth of the decode loop, in chunks), "gemm_timing" (HIP events around every encoder-layer GEMM launch -> sonic_timings.enc_gemm_*),
 * "no_fused_rope" (encoder RoPE as its own pass), "no_gelu_lut" (fc1 GELU by arithmetic instead of the LDS table); the full list with what each one measured is in
 * DESIGN.md 1.  Round 6: "no_pre_norm" (<= 2 rows: standalone add + RMSNorm launches instead of the five-launch chain; same bits), "decode_gemv" / "decode_prefetch" /
 * "decode_attn_occ2" (experiments that lost: profiles/round6_*), "f32_synth_bf16" (SONIC_MODE_F32: sonic_load_synthetic writes the bf16-rounded values),
 * "inject_dev_err" (tests: sets / clears the device error word); "token_logprobs" (not an experiment: per-token log-probabilities, see sonic_fetch_logprobs);
 * "top_logprobs" (not an experiment either: the K best alternatives of every step in the same records, see sonic_fetch_logprobs);
 * "forced_parallel", "forced_fanout", "forced_share_prompt", "score_chunk_rows" (not experiments: forced runs as one prefill pass - scoring given transcripts - see sonic_set_forced_ids);
 * "forced_align", "align_head" (not experiments: word timestamps on that pass, see sonic_set_forced_ids);
 * "draft_verify" (not an experiment: a request's draft is verified in its prefill pass, see sonic_set_forced_ids);
 * "fp8_weights" (not an experiment: mode fp8, DESIGN.md 6.16 - value 1, once, on a finalized bf16 weight owner before its slots exist: every decoder matrix and the
 * embedding are snapped in place onto a per-row power-of-two-scaled OCP e4m3 grid, the e4m3 copies (one byte per weight, four per row) are added to
 * sonic_weight_bytes / sonic_memory_info, and token steps of <= 4 rows stream them; refused by name on int8 / fp16 / fp32 handles, on a slot, on an owner with slots,
 * while the handle has work in hand, and for 0 after 1), "fp8_chain" (0 / 1, only with fp8_weights on, which sets it to 1: 0 runs the snapped model on the default
 * chains - full batch invariance, no byte saving; with 1 a request's low bits depend on whether its step ran at <= 4 rows, as with "decode_gemv") */
SONIC_API int sonic_set_option(sonic_engine* e, const char* key, int value);

/* ---- Silero VAD network (silero-vad 5.x / 6.x, 16 kHz branch; csrc/vad.hip, layer table in sonicscribe_amd/vad_net.py) ----
 * A handle of its own, not part of sonic_engine: the reference builds the VAD apart from the ASR model (models_manager.py:34-49), and a
 * VAD call never queues behind a decoding batch.  Own stream and lock: thread-safe, calls from several threads serialise on the handle.
 *   sonic_vad_create(device_id, max_windows, &v)   max_windows: windows the first buffers hold; a larger call grows them (never refused)
 *   sonic_vad_last_error(v)      v may be NULL: the error of the last failed sonic_vad_create on this thread
 *   sonic_vad_load_tensor(v, name, data, shape, ndim)   fp32, names of load_silero_vad()'s state dict without the `_model.` prefix; name
 *                                and shape are checked.  Until all 15 tensors are loaded sonic_vad_probs returns SONIC_ERR_INVALID naming
 *                                the first missing one
 *   sonic_vad_probs(v, pcm_i16, pcm_f32, off, B, probs)   exactly one of pcm_i16 / pcm_f32; sequence b = samples off[b] .. off[b+1]-1
 *                                (16 kHz).  int16 means x / 32768; float is divided by max|x| when that exceeds 1 (backend/vad.py:24-38).
 *                                A sequence is cut into ceil(n / 512) windows (the last zero-padded), each scored with the model state
 *                                carried from the previous window (reset per sequence); probs[sum of ceil(n_b / 512)] in sequence order.
 *                                All fp32; a sequence's probabilities do not depend on the rest of the call (bit for bit). */
typedef struct sonic_vad sonic_vad;
SONIC_API int sonic_vad_create(int device_id, int max_windows, sonic_vad** out);
SONIC_API void sonic_vad_destroy(sonic_vad* v);
SONIC_API const char* sonic_vad_last_error(sonic_vad* v);
SONIC_API int sonic_vad_load_tensor(sonic_vad* v, const char* name, const float* data, const int64_t* shape, int ndim);
SONIC_API int sonic_vad_probs(sonic_vad* v, const int16_t* pcm_i16, const float* pcm_f32, const int64_t* off, int B, float* probs);
/* sonic_vad_probs over audio that is already resident in device rings (sonic_ring_*), read in place: replaces the upload of the whole
 * file tensor for backend/main.py:308-314 (vad_processor.detect_voice_activity(full_audio_tensor)) and the second upload of every tick's
 * window bytes (vad_processor_manager.py:95-104).  Sequence b is the concatenation of pieces seq_piece[b] .. seq_piece[b+1]-1 (seq_piece[0]
 * = 0), piece p the samples [piece_start[p], piece_start[p] + piece_n[p]) (absolute indices, as sonic_ring_append returns them) of ring
 * piece_ring[p]; a file is one piece, a gate window whose chunk ids skip is several.  A sequence is windowed exactly as a host sequence
 * of sonic_vad_probs (int16 form: x / 32768): ceil(n / 512) windows, the last zero-padded, state and context reset per sequence - the
 * first window has no context whatever precedes it in the ring - and gives the same bits.  Windows may straddle the ring's wrap and
 * piece boundaries.  The rules of sonic_stage_mixed hold: rings are looked up in the registry of e's weight owner (a destroyed ring or one
 * of another engine is refused, never dereferenced), a ring on another device than v is refused, a piece outside [head - capacity, head)
 * is refused, ring locks are taken in one global order and held until the kernel that reads the rings has completed, and the VAD's
 * stream orders behind each ring's last append.  Does not take e's lock: it never queues behind a decoding batch. */
SONIC_API int sonic_vad_probs_rings(sonic_vad* v, sonic_engine* e, sonic_ring* const* piece_ring, const int64_t* piece_start,
                                    const int32_t* piece_n, const int64_t* seq_piece, int B, float* probs);

#ifdef __cplusplus
}
#endif
#endif /* SONIC_HIP_H */
