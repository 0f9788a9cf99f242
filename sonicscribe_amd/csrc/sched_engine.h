// What the scheduler units (dispatch.cpp, pipeline.cpp) ask of the engine beyond the C ABI of include/sonic_hip.h, declared once: they include this header, and so
// do the units that define these functions (through engine_internal.h), so a signature that drifts is a compile error.  Plus the handle set both create functions
// check.  Depends on include/sonic_hip.h alone: the scheduler units use nothing of engine_internal.h.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/sonic_hip.h"

struct sonic_grammar;
extern "C" {
// options of one handle (NULL: off)
int engine_token_logprobs_on(sonic_engine* e);
int engine_top_logprobs(sonic_engine* e);                      // K: its log-probability records hold 1 + 2K floats (0 with token_logprobs off)
int engine_forced_parallel_on(sonic_engine* e);                // a scoring handle: both schedulers refuse it
int engine_request_bias_on(sonic_engine* e);
int engine_sampling_on(sonic_engine* e);
int engine_truncation_on(sonic_engine* e);                     // option truncation
int engine_grammar_on(sonic_engine* e);
int engine_lm_on(sonic_engine* e);                             // option lm (the bulk pipeline carries no language-model state: refused there)
int engine_draft_verify_on(sonic_engine* e);                  // (the bulk pipeline takes no drafts: refused there)
int engine_fetch_stream_on(sonic_engine* e);                   // option fetch_stream (A/B): its fetches take about a chunk's time, the bulk pipeline queues a chunk ahead of them
int engine_tok_cap(sonic_engine* e);                          // the tokens one prefill of the handle holds
// one request's values, checked at its submit (the message goes to the calling thread's sonic_last_error(NULL))
int engine_bias_validate(sonic_engine* e, const int32_t* seq_ids, const int32_t* seq_off, const float* bias, int n);   // a table against the caps and this handle's vocabulary
int engine_sampling_validate(float temperature);               // 0 or 1e-3 .. 100
int engine_truncation_validate(const float* row);              // one (top_k, top_p, min_p)
int engine_draft_validate(sonic_engine* e, const int32_t* ids, int n);   // a draft's ids against this handle's model: in the vocabulary, neither the audio placeholder nor an EOS id
// (none of the four takes an engine lock - a decoding handle holds its own for a chunk at a time -, and neither do the next two: the owner's registry lock alone)
sonic_grammar* engine_grammar_ref_id(sonic_engine* e, int id); // grammar `id` of e's weight owner with a reference, or NULL (no such live grammar) ...
void engine_grammar_unref(sonic_grammar* g);                   // ... and the reference's return
int engine_set_request_grammar(sonic_engine* e, sonic_grammar* const* grammars, int R);   // a batch's grammars (NULL: a free request) for the handle's next prefill
// a message from outside a handle's calls: to the calling thread's sonic_last_error(NULL) / on a handle (sonic_last_error(e)); returns code
int engine_thread_fail(int code, const char* msg);
int engine_fail(sonic_engine* e, int code, const char* msg);
}

// The (decoders, n_dec, prefills, n_pre) of a create function as one list: decoders first, then prefills.
struct sched_handles {
    std::vector<sonic_engine*> h;
    std::vector<int32_t> max_batch;                                // per handle, filled by check()
    size_t n_dec = 0;
    sched_handles(sonic_engine* const* decoders, int n_decoders, sonic_engine* const* prefills, int n_prefills) : h(decoders, decoders + n_decoders), n_dec((size_t)n_decoders) {
        h.insert(h.end(), prefills, prefills + n_prefills);
    }
    bool check() {                                                 // every handle live and there once, all on one weight copy and one device
        const void* w0 = nullptr; int32_t dev0 = -1;
        max_batch.assign(h.size(), 0);
        for (size_t i = 0; i < h.size(); ++i) {
            int32_t dev = 0; const void* wid = nullptr;
            if (!h[i] || sonic_engine_info(h[i], &max_batch[i], nullptr, nullptr, &dev, &wid) != SONIC_OK) return false;
            if (std::find(h.begin(), h.begin() + i, h[i]) != h.begin() + i) return false;
            if (i == 0) { w0 = wid; dev0 = dev; }
            if (wid != w0 || dev != dev0) return false;
        }
        return true;
    }
    template <class P> bool every(P p) const { return std::all_of(h.begin(), h.end(), p); }
    template <class P> bool any(P p) const { return std::any_of(h.begin(), h.end(), p); }
};
