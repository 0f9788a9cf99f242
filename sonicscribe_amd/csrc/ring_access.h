// What the VAD handle (vad.cpp) may know about the engine's device rings (engine_ingest.cpp keeps struct sonic_ring to itself): sample
// ranges of rings are checked and pinned here, by the rules of stage_mixed_locked, and come back as plain buffer views.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <string>
#include <vector>

struct sonic_engine;
struct sonic_ring;

struct RingView {
    const int16_t* buf;     // ring buffer in HBM
    int64_t cap;            // capacity in samples
};

// Looks every ring up in the registry of e's weight owner (a destroyed or foreign ring is refused, never dereferenced), refuses rings on
// another device than `device`, locks the rings in one global order, checks every piece [start, start + n) against [head - cap, head)
// and makes `st` wait for each ring's last append.  On SONIC_OK view[p] describes piece p's ring and `held` owns the ring locks: the
// caller keeps it until the kernel that reads the rings has COMPLETED (appends carry no device-side wait on readers, see
// sonic_ring_append).  On failure `err` says why and nothing stays locked.
int ring_ranges_acquire(sonic_engine* e, sonic_ring* const* ring, const int64_t* start, const int32_t* n, int64_t P, int device, hipStream_t st,
                        RingView* view, std::vector<std::unique_lock<std::mutex>>& held, std::string& err);
