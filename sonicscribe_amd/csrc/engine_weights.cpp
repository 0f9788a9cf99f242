// sonic_hip engine: the tensor inventory, weight upload (sonic_load_tensor / sonic_load_synthetic), LLM.int8 quantisation and the packing of
// sonic_finalize_weights.
#include "engine_internal.h"

static uint64_t mix64h(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31);
}
static uint64_t fnv1a64h(const char* s) { uint64_t h = 0xCBF29CE484222325ULL; for (; *s; ++s) { h ^= (uint8_t)*s; h *= 0x100000001B3ULL; } return h; }

// conv weight [C][Ci][3] -> [C][3][Ci]
__global__ void conv_permute_kernel(const bf16_t* in, bf16_t* out, int C, int Ci) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)C * Ci * 3) return;
    const int k = e % 3, ci = (e / 3) % Ci, c = e / (3L * Ci);
    out[((long)c * 3 + k) * Ci + ci] = in[e];
}

// ------------------------------------------------------------------------------------------ tensor inventory (spec.py order)
struct InvEntry { std::string name; std::vector<int64_t> shape; int kind; };  // kind 0 mat, 1 embed, 2 bias, 3 norm
static std::vector<InvEntry> inventory(const sonic_dims& d) {
    std::vector<InvEntry> v;
    const int64_t C = d.enc_d, F = d.enc_ff, M = d.n_mels;
    auto add = [&](const std::string& n, std::vector<int64_t> s, int k) { v.push_back({n, s, k}); };
    const std::string at = "model.audio_tower.";
    add(at + "conv1.weight", {C, M, 3}, 0); add(at + "conv1.bias", {C}, 2);
    add(at + "conv2.weight", {C, C, 3}, 0); add(at + "conv2.bias", {C}, 2);
    for (int i = 0; i < d.enc_layers; ++i) {
        const std::string p = at + "layers." + std::to_string(i) + ".";
        add(p + "input_layernorm.weight", {C}, 3); add(p + "input_layernorm.bias", {C}, 2);
        add(p + "self_attn.q_proj.weight", {C, C}, 0); add(p + "self_attn.q_proj.bias", {C}, 2);
        add(p + "self_attn.k_proj.weight", {C, C}, 0);
        add(p + "self_attn.v_proj.weight", {C, C}, 0); add(p + "self_attn.v_proj.bias", {C}, 2);
        add(p + "self_attn.o_proj.weight", {C, C}, 0); add(p + "self_attn.o_proj.bias", {C}, 2);
        add(p + "post_attention_layernorm.weight", {C}, 3); add(p + "post_attention_layernorm.bias", {C}, 2);
        add(p + "mlp.fc1.weight", {F, C}, 0); add(p + "mlp.fc1.bias", {F}, 2);
        add(p + "mlp.fc2.weight", {C, F}, 0); add(p + "mlp.fc2.bias", {C}, 2);
    }
    add(at + "norm.weight", {C}, 3); add(at + "norm.bias", {C}, 2);
    const int64_t PI = C * d.merge, PM = 2L * d.dec_d, D = d.dec_d;
    const std::string pj = "model.multi_modal_projector.";
    add(pj + "linear_1.weight", {PM, PI}, 0); add(pj + "linear_1.bias", {PM}, 2);
    add(pj + "linear_2.weight", {D, PM}, 0); add(pj + "linear_2.bias", {D}, 2);
    const std::string lm = "model.language_model.";
    add(lm + "embed_tokens.weight", {d.vocab, D}, 1);
    const int64_t QD = (int64_t)d.dec_heads * d.dec_head_dim, KD = (int64_t)d.dec_kv_heads * d.dec_head_dim, FF = d.dec_ff;
    for (int i = 0; i < d.dec_layers; ++i) {
        const std::string p = lm + "layers." + std::to_string(i) + ".";
        add(p + "input_layernorm.weight", {D}, 3);
        add(p + "self_attn.q_proj.weight", {QD, D}, 0); add(p + "self_attn.k_proj.weight", {KD, D}, 0);
        add(p + "self_attn.v_proj.weight", {KD, D}, 0); add(p + "self_attn.o_proj.weight", {D, QD}, 0);
        add(p + "post_attention_layernorm.weight", {D}, 3);
        add(p + "mlp.gate_proj.weight", {FF, D}, 0); add(p + "mlp.up_proj.weight", {FF, D}, 0); add(p + "mlp.down_proj.weight", {D, FF}, 0);
    }
    add(lm + "norm.weight", {D}, 3);
    return v;
}
static size_t numel(const std::vector<int64_t>& s) { size_t n = 1; for (auto x : s) n *= (size_t)x; return n; }

// ------------------------------------------------------------------------------------------ weights
static int raw_alloc(sonic_engine* e, const std::string& name, const std::vector<int64_t>& shape, DevTensor** out) {
    DevTensor& t = e->raw[name];
    if (!t.p) {
        t.shape = shape; t.n = numel(shape);
        void* q = nullptr;
        HIPC(e, hipMalloc(&q, t.n * sizeof(bf16_t)));
        t.p = (bf16_t*)q; e->alloc_bytes += (int64_t)(t.n * sizeof(bf16_t));
    } else if (t.shape != shape) return fail(e, SONIC_ERR_INVALID, "tensor %s loaded twice with different shapes", name.c_str());
    *out = &t;
    return SONIC_OK;
}

extern "C" int sonic_load_tensor(sonic_engine* e, const char* name, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!e || !name || !data || !shape) return SONIC_ERR_INVALID;
    // grammars are int32 "tensors" of a finalized engine: "grammar:<id>" creates (shape {0}: destroys) one on the weight owner, without the
    // engine lock; "grammar.hook:<V>" arms the kernel hooks' automaton
    if (!strncmp(name, "grammar:", 8) || !strncmp(name, "grammar.hook:", 13)) {
        if (dtype != SONIC_DTYPE_I32 || ndim != 1 || shape[0] < 0) return fail(nullptr, SONIC_ERR_INVALID, "%s: a grammar is one row of int32 words (SONIC_DTYPE_I32, ndim 1)", name);
        if (name[7] == ':') return gram_create(e, atoi(name + 8), (const int*)data, shape[0]);
        return gram_hook_arm(e, atoi(name + 13), (const int*)data, shape[0]);
    }
    // language models, likewise: "lm:<id>" creates (shape {0}: destroys) one on the weight owner; "lm.hook:<V>" arms the kernel hooks' automaton and
    // "lm.hook.step" (one finished flag per row) launches lm_step_kernel alone on it
    if (!strncmp(name, "lm:", 3) || !strncmp(name, "lm.hook:", 8) || !strcmp(name, "lm.hook.step")) {
        if (dtype != SONIC_DTYPE_I32 || ndim != 1 || shape[0] < 0) return fail(nullptr, SONIC_ERR_INVALID, "%s: a language model is one row of int32 words (SONIC_DTYPE_I32, ndim 1)", name);
        if (name[2] == ':') return lm_create(e, atoi(name + 3), (const int*)data, shape[0]);
        if (name[7] == ':') return lm_hook_arm(e, atoi(name + 8), (const int*)data, shape[0]);
        return lm_hook_step(e, (const int*)data, shape[0]);
    }
    if (!strncmp(name, "gemm.form:", 10)) return gemm_form_stage(e, name + 10, data, dtype, shape, ndim);      // the GEMM form hook's buffers and its launch (include/sonic_hip.h)
    if (!strcmp(name, "gemm.form.run")) return gemm_form_run(e, data, dtype, shape, ndim);
    if (!strcmp(name, "request_draft")) return draft_stage_words(e, data, dtype, shape, ndim);      // the drafts of the next prefill's requests (option draft_verify)
    if (!strcmp(name, "request_forks")) return fork_stage_counts(e, data, dtype, shape, ndim);      // the fork counts of the next prefill's requests
    if (!strcmp(name, "request_truncation")) return trunc_stage_rows(e, data, dtype, shape, ndim);      // top_k / top_p / min_p of the next prefill's rows (option truncation)
    if (!strcmp(name, "truncation.hook")) return trunc_hook_arm(e, data, dtype, shape, ndim);      // ... and of the next sonic_test_greedy_sample launch
    if (!strcmp(name, "share_prompt.hook")) return share_hook_arm(e, data, dtype, shape, ndim);      // pre_row | pre_len of the next sonic_test_prefill_attention launch (option forced_share_prompt's kernel)
    ENTER(e);
    if (e->finalized) return fail(e, SONIC_ERR_INVALID, "weights already finalized");
    std::vector<int64_t> shp(shape, shape + ndim);
    bool known = false;
    for (auto& it : inventory(e->d)) if (it.name == name) { known = true; if (it.shape != shp) return fail(e, SONIC_ERR_INVALID, "tensor %s: unexpected shape", name); }
    if (!known) return fail(e, SONIC_ERR_INVALID, "unknown tensor name %s", name);
    if (e->f32) {      // fp32 kind: the tensor stays fp32 (a bf16 source is widened exactly)
        const size_t n = numel(shp);
        float*& dst = e->f->raw[name];
        if (!dst) TRY(dalloc(e, &dst, n, false));
        if (dtype == SONIC_DTYPE_F32) HIPC(e, h2d(e, dst, data, n * 4));
        else if (dtype == SONIC_DTYPE_BF16) {
            bf16_t* tmp = nullptr;
            HIPC(e, hipMalloc((void**)&tmp, n * 2));
            hipError_t r = h2d(e, tmp, data, n * 2);
            if (r == hipSuccess) { launch_bf16_to_f32(tmp, dst, (long)n, e->st, DT_BF16); r = stream_sync(e); }
            (void)hipFree(tmp);
            HIPC(e, r);
        } else return fail(e, SONIC_ERR_INVALID, "dtype must be f32 or bf16");
        e->weight_bytes += (int64_t)n * 4;
        return SONIC_OK;
    }
    DevTensor* t;
    TRY(raw_alloc(e, name, shp, &t));
    if (dtype == SONIC_DTYPE_BF16) {
        HIPC(e, h2d(e, t->p, data, t->n * 2));
    } else if (dtype == SONIC_DTYPE_F32) {
        float* tmp = nullptr;
        HIPC(e, hipMalloc((void**)&tmp, t->n * 4));
        hipError_t r = h2d(e, tmp, data, t->n * 4);
        // int8 mode loads the checkpoint with torch_dtype=float16 (asr.py:156): an fp32 source goes straight to fp16
        if (r == hipSuccess) { launch_f32_to_bf16(tmp, t->p, (long)t->n, e->st, e->dt); r = stream_sync(e); if (e->dt == DT_F16) e->raw_f16[name] = true; }
        (void)hipFree(tmp);
        HIPC(e, r);
    } else return fail(e, SONIC_ERR_INVALID, "dtype must be f32 or bf16");
    return SONIC_OK;
}

extern "C" int sonic_load_synthetic(sonic_engine* e, uint64_t seed) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    if (e->finalized) return fail(e, SONIC_ERR_INVALID, "weights already finalized");
    for (auto& it : inventory(e->d)) {
        DevTensor* t = nullptr;
        float* t32 = nullptr;
        if (e->f32) { float*& dst = e->f->raw[it.name]; if (!dst) TRY(dalloc(e, &dst, numel(it.shape), false)); t32 = dst; e->weight_bytes += (int64_t)numel(it.shape) * 4; }
        else TRY(raw_alloc(e, it.name, it.shape, &t));
        float scale = 0.1f, offset = 0.f;
        if (it.kind == 0) { double fi = 1; for (size_t i = 1; i < it.shape.size(); ++i) fi *= (double)it.shape[i]; scale = (float)sqrt(3.0 / fi); }
        else if (it.kind == 1) scale = (float)sqrt(3.0 / (double)it.shape[1]);
        else if (it.kind == 3) offset = 1.0f;
        const uint64_t key = mix64h(seed * 0x9E3779B97F4A7C15ULL + fnv1a64h(it.name.c_str()));
        if (e->f32) launch_synth_fill(key, (long)numel(it.shape), scale, offset, nullptr, t32, e->st, e->opt_f32_synth_bf16);     // the generator's exact fp32 values (synth.py bf16=False); option f32_synth_bf16: the bf16-rounded ones (the weights of a bf16 engine with the same seed)
        else launch_synth_fill(key, (long)t->n, scale, offset, t->p, nullptr, e->st);
    }
    HIPC(e, stream_sync(e));
    return SONIC_OK;
}

static int need(sonic_engine* e, const std::string& name, DevTensor** t) {
    auto it = e->raw.find(name);
    if (it == e->raw.end() || !it->second.p) return fail(e, SONIC_ERR_INVALID, "missing weight tensor %s", name.c_str());
    *t = &it->second;
    return SONIC_OK;
}
static int to_f32(sonic_engine* e, const std::string& name, float** out) {
    DevTensor* t; TRY(need(e, name, &t));
    TRY(dalloc(e, out, t->n, false));
    launch_bf16_to_f32(t->p, *out, (long)t->n, e->st, e->dt);
    e->weight_bytes += (int64_t)t->n * 4;
    return SONIC_OK;
}
// int8 mode: row-wise int8 of a packed [N][K] fp16 matrix (Int8Params.cuda()); the 16-bit matrix is released afterwards
static int quantize(sonic_engine* e, bf16_t** w16, int N, int K, QW* q, bool tiled, bool kmajor = false) {
    TRY(dalloc(e, &q->cb, (size_t)N * K, false)); TRY(dalloc(e, &q->scb, (size_t)N, false));
    launch_quant_weights(*w16, q->cb, q->scb, N, K, e->st);
    e->weight_bytes += (int64_t)N * K + (int64_t)N * 4 - (int64_t)N * K * 2;
    if (tiled) {
        TRY(dalloc(e, &q->cbt, (size_t)N * K, false));
        launch_tile_weights_i8(q->cb, q->cbt, N, K, e->st);
        e->weight_bytes += (int64_t)N * K;
        // k-major copy for the decode consumers' outlier gathers (8 consecutive bytes per outlier column and 8 outputs; from the tiled copy the same 8 bytes lie in 8
        // different 16-byte pieces: 16 x the cache lines).  Rounds 3 - 5 kept it for all four decoder projections (1.29 GB at full size); round 6 keeps it only where it
        // pays - o_proj and down_proj, whose consumer (add + RMSNorm: one block per row walking the row's whole outlier list over 2048 outputs) got 25 % slower without it -
        // and lets the prefill epilogues, the side product, the attention prologue and SwiGLU gather from the tiled copy: 3 683 -> 2 865 MiB at the same step time.
        // SONIC_KEEP_CBK=1: all four (A/B); SONIC_NO_CBK=1: none (2 395 MiB, the 64-row step +4.9 %).
        if ((kmajor && !getenv("SONIC_NO_CBK")) || getenv("SONIC_KEEP_CBK")) {
            TRY(dalloc(e, &q->cbk, (size_t)N * K, false));
            launch_transpose_i8(q->cb, q->cbk, N, K, e->st);
            e->weight_bytes += (int64_t)N * K;
        }
    }
    HIPC(e, stream_sync(e));
    for (auto it = e->allocs.begin(); it != e->allocs.end(); ++it) if (*it == (void*)*w16) { e->allocs.erase(it); break; }
    (void)hipFree(*w16); *w16 = nullptr; e->alloc_bytes -= (int64_t)N * K * 2;
    if (q->cbt && !getenv("SONIC_KEEP_ROWMAJOR")) {
        // the row-major int8 matrix was the prefill GEMM's operand and its outlier-column source: the tiled and the k-major copy serve both now
        for (auto it = e->allocs.begin(); it != e->allocs.end(); ++it) if (*it == (void*)q->cb) { e->allocs.erase(it); break; }
        (void)hipFree(q->cb); q->cb = nullptr; q->cb_rowmajor_kept = false;
        e->alloc_bytes -= (int64_t)(((size_t)N * K + 3) / 4 * 4); e->weight_bytes -= (int64_t)N * K;
    }
    return SONIC_OK;
}
// concatenate row blocks of [rows_i][K] tensors
static int concat_rows(sonic_engine* e, const std::vector<std::string>& names, bf16_t** out) {
    size_t tot = 0; std::vector<DevTensor*> ts;
    for (auto& n : names) { DevTensor* t; TRY(need(e, n, &t)); ts.push_back(t); tot += t->n; }
    TRY(dalloc(e, out, tot, false));
    size_t o = 0;
    for (auto* t : ts) { HIPC(e, hipMemcpyAsync(*out + o, t->p, t->n * 2, hipMemcpyDeviceToDevice, e->st)); o += t->n; }
    e->weight_bytes += (int64_t)tot * 2;
    return SONIC_OK;
}
static int keep_raw(sonic_engine* e, const std::string& name, bf16_t** out) {
    DevTensor* t; TRY(need(e, name, &t));
    *out = t->p; e->allocs.push_back(t->p); t->p = nullptr;   // ownership moves to the engine's alloc list
    e->weight_bytes += (int64_t)t->n * 2;
    return SONIC_OK;
}

extern "C" int sonic_finalize_weights(sonic_engine* e) {
    if (!e) return SONIC_ERR_INVALID;
    ENTER(e);
    if (e->finalized) return SONIC_OK;
    if (e->f32) return f32_finalize(e);
    const sonic_dims& d = e->d;
    const std::string at = "model.audio_tower.", pj = "model.multi_modal_projector.", lm = "model.language_model.";
    e->weight_bytes = 0;
    if (e->dt == DT_F16)   // a bf16 checkpoint (or the synthetic generator's bf16 values) loaded as fp16, in place (asr.py:156 torch_dtype=float16)
        for (auto& kv : e->raw) if (kv.second.p && !e->raw_f16.count(kv.first)) launch_bf16_to_f16(kv.second.p, kv.second.p, (long)kv.second.n, e->st);
    {   // conv stem in im2col order [C][3][Ci]
        DevTensor *w1, *w2; TRY(need(e, at + "conv1.weight", &w1)); TRY(need(e, at + "conv2.weight", &w2));
        TRY(dalloc(e, &e->conv1w, w1->n, false)); TRY(dalloc(e, &e->conv2w, w2->n, false));
        hipLaunchKernelGGL(conv_permute_kernel, dim3((w1->n + 255) / 256), dim3(256), 0, e->st, w1->p, e->conv1w, d.enc_d, d.n_mels);
        hipLaunchKernelGGL(conv_permute_kernel, dim3((w2->n + 255) / 256), dim3(256), 0, e->st, w2->p, e->conv2w, d.enc_d, d.enc_d);
        e->weight_bytes += (int64_t)(w1->n + w2->n) * 2;
        TRY(to_f32(e, at + "conv1.bias", &e->conv1b)); TRY(to_f32(e, at + "conv2.bias", &e->conv2b));
    }
    e->enc.resize(d.enc_layers);
    for (int i = 0; i < d.enc_layers; ++i) {
        const std::string p = at + "layers." + std::to_string(i) + ".";
        EncLayerW& L = e->enc[i];
        TRY(to_f32(e, p + "input_layernorm.weight", &L.ln1w)); TRY(to_f32(e, p + "input_layernorm.bias", &L.ln1b));
        TRY(concat_rows(e, {p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"}, &L.wqkv));
        TRY(dalloc(e, &L.bqkv, (size_t)3 * d.enc_d, true));   // k_proj has no bias (modeling_glmasr.py:184)
        DevTensor *bq, *bv; TRY(need(e, p + "self_attn.q_proj.bias", &bq)); TRY(need(e, p + "self_attn.v_proj.bias", &bv));
        launch_bf16_to_f32(bq->p, L.bqkv, d.enc_d, e->st, e->dt);
        launch_bf16_to_f32(bv->p, L.bqkv + 2 * d.enc_d, d.enc_d, e->st, e->dt);
        TRY(keep_raw(e, p + "self_attn.o_proj.weight", &L.wo)); TRY(to_f32(e, p + "self_attn.o_proj.bias", &L.bo));
        TRY(to_f32(e, p + "post_attention_layernorm.weight", &L.ln2w)); TRY(to_f32(e, p + "post_attention_layernorm.bias", &L.ln2b));
        TRY(keep_raw(e, p + "mlp.fc1.weight", &L.w1)); TRY(to_f32(e, p + "mlp.fc1.bias", &L.b1));
        TRY(keep_raw(e, p + "mlp.fc2.weight", &L.w2)); TRY(to_f32(e, p + "mlp.fc2.bias", &L.b2));
        if (e->i8) {
            TRY(quantize(e, &L.wqkv, 3 * d.enc_d, d.enc_d, &L.qqkv, false)); TRY(quantize(e, &L.wo, d.enc_d, d.enc_d, &L.qo, false));
            TRY(quantize(e, &L.w1, d.enc_ff, d.enc_d, &L.q1, false)); TRY(quantize(e, &L.w2, d.enc_d, d.enc_ff, &L.q2, false));
        }
    }
    TRY(to_f32(e, at + "norm.weight", &e->enc_nw)); TRY(to_f32(e, at + "norm.bias", &e->enc_nb));
    TRY(keep_raw(e, pj + "linear_1.weight", &e->pj1w)); TRY(to_f32(e, pj + "linear_1.bias", &e->pj1b));
    TRY(keep_raw(e, pj + "linear_2.weight", &e->pj2w)); TRY(to_f32(e, pj + "linear_2.bias", &e->pj2b));
    if (e->i8) {   // both projector linears are swapped: the reference's skip pattern 'audio_proj' does not match 'multi_modal_projector'
        TRY(quantize(e, &e->pj1w, 2 * d.dec_d, d.enc_d * d.merge, &e->qpj1, false)); TRY(quantize(e, &e->pj2w, d.dec_d, 2 * d.dec_d, &e->qpj2, false));
    }
    TRY(keep_raw(e, lm + "embed_tokens.weight", &e->embed));
    e->dec.resize(d.dec_layers);
    for (int i = 0; i < d.dec_layers; ++i) {
        const std::string p = lm + "layers." + std::to_string(i) + ".";
        DecLayerW& L = e->dec[i];
        TRY(to_f32(e, p + "input_layernorm.weight", &L.ln1)); TRY(to_f32(e, p + "post_attention_layernorm.weight", &L.ln2));
        TRY(concat_rows(e, {p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"}, &L.wqkv));
        TRY(keep_raw(e, p + "self_attn.o_proj.weight", &L.wo));
        // gate / up interleaved in 16-row groups (EPI_SWIGLU, swiglu_slab_kernel)
        DevTensor *g, *u; TRY(need(e, p + "mlp.gate_proj.weight", &g)); TRY(need(e, p + "mlp.up_proj.weight", &u));
        TRY(dalloc(e, &L.wgu, g->n * 2, false));
        const size_t blk = (size_t)16 * d.dec_d * 2;
        HIPC(e, hipMemcpy2DAsync(L.wgu, 2 * blk, g->p, blk, blk, d.dec_ff / 16, hipMemcpyDeviceToDevice, e->st));
        HIPC(e, hipMemcpy2DAsync((char*)L.wgu + blk, 2 * blk, u->p, blk, blk, d.dec_ff / 16, hipMemcpyDeviceToDevice, e->st));
        e->weight_bytes += (int64_t)g->n * 4;
        TRY(keep_raw(e, p + "mlp.down_proj.weight", &L.wdown));
        auto tiled = [&](const bf16_t* w, bf16_t** out, int N, int K) -> int {
            TRY(dalloc(e, out, (size_t)N * K, false));
            launch_tile_weights(w, *out, N, K, e->st);
            e->weight_bytes += (int64_t)N * K * 2;
            return SONIC_OK;
        };
        L.wgu_t8 = nullptr; L.wqkv_t = L.wo_t = L.wgu_t = L.wdown_t = nullptr;
        if (e->i8) {
            TRY(quantize(e, &L.wqkv, e->qkvN, d.dec_d, &L.qqkv, true)); TRY(quantize(e, &L.wo, d.dec_d, e->QD, &L.qo, true, true));
            TRY(quantize(e, &L.wgu, 2 * d.dec_ff, d.dec_d, &L.qgu, true)); TRY(quantize(e, &L.wdown, d.dec_d, d.dec_ff, &L.qdown, true, true));
            continue;
        }
        TRY(tiled(L.wqkv, &L.wqkv_t, e->qkvN, d.dec_d)); TRY(tiled(L.wo, &L.wo_t, d.dec_d, e->QD));
        TRY(tiled(L.wdown, &L.wdown_t, d.dec_d, d.dec_ff));
        if (skinny_gu_eligible(1, 2 * d.dec_ff, d.dec_d)) {          // fused gate/up kernel's layout (8-row gate/up interleave); both 16-bit element types (round 5)
            // ONE decode copy of gate/up: the unfused path (A/B, shapes the fused kernel does not take) multiplies the same tiles and its SwiGLU pass
            // reads the columns in the 8-row interleave (round 4 kept a second tiled copy in the 16-row interleave: 1.4 GB of the full-size model)
            TRY(dalloc(e, &L.wgu_t8, (size_t)2 * d.dec_ff * d.dec_d, false));
            launch_tile_weights_gu8(L.wgu, L.wgu_t8, 2 * d.dec_ff, d.dec_d, e->st);
            e->weight_bytes += (int64_t)2 * d.dec_ff * d.dec_d * 2;
        } else {
            TRY(tiled(L.wgu, &L.wgu_t, 2 * d.dec_ff, d.dec_d));
        }
    }
    if (!e->i8 && !getenv("SONIC_KEEP_ROWMAJOR")) {
        // the row-major decoder projections were only the prefill GEMMs' operand: those read the tiled copies now (GemmArgs.w_tiled)
        HIPC(e, stream_sync(e));
        auto drop = [&](bf16_t** w, size_t n) {
            if (!*w) return;
            for (auto it = e->allocs.begin(); it != e->allocs.end(); ++it) if (*it == (void*)*w) { e->allocs.erase(it); break; }
            (void)hipFree(*w); *w = nullptr; e->alloc_bytes -= (int64_t)((n * 2 + 3) / 4 * 4); e->weight_bytes -= (int64_t)n * 2;
        };
        for (auto& L : e->dec) {
            drop(&L.wqkv, (size_t)e->qkvN * d.dec_d); drop(&L.wo, (size_t)d.dec_d * e->QD);
            drop(&L.wgu, (size_t)2 * d.dec_ff * d.dec_d); drop(&L.wdown, (size_t)d.dec_d * d.dec_ff);
        }
    }
    TRY(dalloc(e, &e->embed_t, (size_t)d.vocab * d.dec_d, false));
    launch_tile_weights(e->embed, e->embed_t, d.vocab, d.dec_d, e->st);
    e->weight_bytes += (int64_t)d.vocab * d.dec_d * 2;
    TRY(to_f32(e, lm + "norm.weight", &e->dec_nw));
    HIPC(e, stream_sync(e));
    for (auto& kv : e->raw) if (kv.second.p) { (void)hipFree(kv.second.p); kv.second.p = nullptr; e->alloc_bytes -= (int64_t)kv.second.n * 2; }
    e->raw.clear();
    e->finalized = true;
    return SONIC_OK;
}
