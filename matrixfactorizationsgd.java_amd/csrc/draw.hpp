// draw.hpp -- the draw of mfsgd_sample_unseen (include/mfsgd.h) as device functions, integers only: ONE definition,
// shared by sample.hip (every draw goes to memory), hardneg.hip (the draws are scored and only the best leaves the
// kernel) and warp.hip (the draws are walked to the first that violates a margin), so that the candidates of
// mfsgd_sample_unseen_hard and mfsgd_sample_unseen_violating are mfsgd_sample_unseen's by construction.
// A draw is a pure function of (seed, its counter c), the user's sorted, distinct list S (length s) and the item count:
//     r   = draw_mix32(seed, c): the upper 32 bits of splitmix64's output for the state seed + golden * (c + 1)
//     t   = (r * cnt) >> 32 with cnt = n_items - s: the rank of the draw among the unseen items, in [0, cnt)
//     out = draw_unseen_at(S, s, t) = t + p, p = the number of positions q < s with S[q] - q <= t
// S[q] - q is the number of unseen items below S[q] and never decreases, so p is a binary search; t + p is the t-th
// unseen item in ascending order.  Exact and without rejection: no draw is ever retried, whatever share of the items
// the user has seen, and a draw costs O(log s) dependent loads.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfsgd {
namespace {

__device__ __forceinline__ unsigned long long draw_mix32(const unsigned long long seed, const unsigned long long c) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (c + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) >> 32;
}

// The t-th (from 0, ascending) item that is not in list[0 .. s), t below the number of such items.
__device__ __forceinline__ int32_t draw_unseen_at(const int32_t* __restrict__ list, const long long s, const long long t) {
    long long lo = 0, hi = s;  // the first q in 0 .. s with list[q] - q > t
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if ((long long)list[mid] - mid <= t) lo = mid + 1;
        else hi = mid;
    }
    return (int32_t)(t + lo);
}

}  // namespace
}  // namespace mfsgd
