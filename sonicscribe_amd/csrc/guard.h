// What the kernels that apply HF's logits processors share (greedy.hip: greedy_kernel<T, LP, true, ...>; verify.hip: verify_rows_kernel<T, true, .>):
// one id's bit into a vocabulary bitmap of the history - "seen" (its ids) or "banned" (the n-gram continuations and the suppress list) - and the score of one id
// under the two.
#pragma once
#include "common.h"

__device__ __forceinline__ float guard_score(float r, unsigned seen, unsigned banned, float p) {
    if (seen & 1u) r = r < 0.f ? r * p : __fdiv_rn(r, p);
    return (banned & 1u) ? -INFINITY : r;
}
__device__ __forceinline__ void guard_set(unsigned* map, int id, int V) {
    if ((unsigned)id < (unsigned)V) atomicOr(&map[id >> 5], 1u << (id & 31));
}
