// The dispatcher's packers: the values its requests bring, one request at a time, into the per-batch forms a prefill takes.  The same two formats as
// engine.pack_request_bias and engine.pack_request_draft on the Python side (tests/test_dispatch_pack_host.py compares them word for word).  Pure host code: no HIP,
// no engine types.
#pragma once
#include <stdint.h>

#include <vector>

namespace dispatch_pack {

// a submit's host_off over W >= 1 windows: 0 == off[0] <= off[1] <= ... <= off[W], so that every window is a range of the request's samples
inline bool offsets_ok(const int64_t* off, int W) {
    if (off[0] != 0) return false;
    for (int w = 0; w < W; ++w) if (off[w + 1] < off[w]) return false;
    return true;
}

// one request's sequence-bias table: sequence i is ids[off[i] .. off[i + 1]) with bias val[i]; off[0] == 0; off empty: no table
struct BiasTable { std::vector<int32_t> ids, off; std::vector<float> val; };

// a copy of a table of n sequences as a submit gets it: its offsets may start anywhere in seq_ids, the copy's start at 0
inline BiasTable bias_table(const int32_t* seq_ids, const int32_t* seq_off, const float* bias, int n) {
    BiasTable t;
    if (n <= 0) return t;
    t.off.assign(seq_off, seq_off + n + 1);
    t.ids.assign(seq_ids + seq_off[0], seq_ids + seq_off[n]);
    t.val.assign(bias, bias + n);
    for (auto& o : t.off) o -= seq_off[0];
    return t;
}

// sonic_set_request_bias's four arrays for a batch: request r's sequences are seq_off / bias entries req_off[r] .. req_off[r + 1]
struct BiasBatch { std::vector<int32_t> seq_ids, seq_off{0}, req_off{0}; std::vector<float> bias; };

inline BiasBatch pack_bias(const std::vector<const BiasTable*>& tables) {
    BiasBatch b;
    for (const BiasTable* t : tables) {
        for (int i = 0; i + 1 < (int)t->off.size(); ++i) {
            b.seq_ids.insert(b.seq_ids.end(), t->ids.begin() + t->off[i], t->ids.begin() + t->off[i + 1]);
            b.seq_off.push_back((int32_t)b.seq_ids.size());
        }
        b.bias.insert(b.bias.end(), t->val.begin(), t->val.end());
        b.req_off.push_back((int32_t)b.bias.size());
    }
    return b;
}

// the words sonic_load_tensor "request_draft" takes for a batch of R drafts (empty: a request without one): R | off[0 .. R] | ids
inline std::vector<int32_t> pack_drafts(const std::vector<const std::vector<int32_t>*>& drafts) {
    std::vector<int32_t> w{(int32_t)drafts.size(), 0};
    for (const auto* d : drafts) w.push_back(w.back() + (int32_t)d->size());
    for (const auto* d : drafts) w.insert(w.end(), d->begin(), d->end());
    return w;
}

}   // namespace dispatch_pack
