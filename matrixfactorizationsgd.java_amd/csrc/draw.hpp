// draw.hpp -- the draws of mfsgd_sample_unseen and mfsgd_sample_unseen_weighted (include/mfsgd.h) as device functions,
// integers only: ONE definition each.  The uniform one is shared by sample.hip (every draw goes to memory), pick.hip
// (the draws are scored and only the best leaves the kernel, or walked to the first that violates a margin) and
// foldin_pairwise.hip (a chain draws its own negatives), so that the candidates of mfsgd_sample_unseen_hard and
// mfsgd_sample_unseen_violating are mfsgd_sample_unseen's by construction; the weighted one is shared the same way, so
// that those of the _weighted calls are mfsgd_sample_unseen_weighted's.  The kernels that score their draws take either
// as a policy (UniformDraw, WeightedDraw, at the end of this file).
// A uniform draw is a pure function of (seed, its counter c), the user's sorted, distinct list S (length s) and the item
// count:
//     r   = draw_mix32(seed, c): the upper 32 bits of splitmix64's output for the state seed + golden * (c + 1)
//     t   = (r * cnt) >> 32 with cnt = n_items - s: the rank of the draw among the unseen items, in [0, cnt)
//     out = draw_unseen_at(S, s, t) = t + p, p = the number of positions q < s with S[q] - q <= t
// S[q] - q is the number of unseen items below S[q] and never decreases, so p is a binary search; t + p is the t-th
// unseen item in ascending order.  Exact and without rejection: no draw is ever retried, whatever share of the items
// the user has seen, and a draw costs O(log s) dependent loads.
// A weighted draw replaces "number of unseen items below S[q]" by their weight.  With C the exclusive prefix of the item
// weights (n_items + 1 entries, C[n_items] = W) and g[q] the weight of the unseen items below S[q] (handle.hpp, Seen::mass):
//     z    = draw_mix64(seed, c): all 64 bits of the same mix
//     cnt  = draw_unseen_mass(...) = W if s == 0, else g[s - 1] + W - C[S[s - 1] + 1]: the weight of the user's unseen items
//     t    = (z * cnt) >> 64, the upper half of the 128-bit product: a rank among the unseen mass, in [0, cnt)
//     p    = the number of positions q < s with g[q] <= t                              one binary search over g
//     base = C[S[p]] - g[p] if p < s, W - cnt otherwise: the seen mass below the gap the draw falls in
//     out  = (the number of x in [0, n_items] with C[x] <= t + base) - 1               one binary search over C
// g never decreases along a list, C never decreases, and t + base < W: the unseen item x comes out for exactly
// C[x + 1] - C[x] values of t, so an item of weight 0 is never drawn, and unit weights give draw_unseen_at(S, s, t).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfsgd {
namespace {

__device__ __forceinline__ unsigned long long draw_mix64(const unsigned long long seed, const unsigned long long c) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (c + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long draw_mix32(const unsigned long long seed, const unsigned long long c) {
    return draw_mix64(seed, c) >> 32;
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

// The weight of the items that are not in list[0 .. s): mass[q] is that of those below list[q], C the weights' prefix.
__device__ __forceinline__ unsigned long long draw_unseen_mass(const int32_t* __restrict__ list,
                                                               const unsigned long long* __restrict__ mass, const long long s,
                                                               const unsigned long long* __restrict__ C, const int n_items) {
    const unsigned long long W = C[n_items];
    return s == 0 ? W : mass[s - 1] + W - C[list[s - 1] + 1];
}

// The item that is not in list[0 .. s) and holds position t of the unseen weight, t below cnt = draw_unseen_mass(...) > 0.
__device__ __forceinline__ int32_t draw_weighted_at(const int32_t* __restrict__ list, const unsigned long long* __restrict__ mass,
                                                    const long long s, const unsigned long long* __restrict__ C, const int n_items,
                                                    const unsigned long long cnt, const unsigned long long t) {
    long long lo = 0, hi = s;  // the first q in 0 .. s with mass[q] > t
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (mass[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    const unsigned long long v = t + (lo < s ? C[list[lo]] - mass[lo] : C[n_items] - cnt);
    long long a = 0, b = n_items;  // the first x in 0 .. n_items with C[x] > v: C[0] = 0 <= v < C[n_items]
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (C[mid] <= v) a = mid + 1;
        else b = mid;
    }
    return (int32_t)(a - 1);
}

// What a draw knows of a user: the sorted, distinct list of the items the user HAS seen (list[0 .. s), which starts at
// items[from] of the index) and cnt = n_items - s, the number of those the user has not.  off == nullptr: an index
// without pairs, every list is empty.
struct Unseen {
    long long s = 0, from = 0, cnt = 0;
    const int32_t* list = nullptr;
    Unseen() = default;
    __device__ __forceinline__ Unseen(const long long* off, const int32_t* items, const int u, const int n_items)
        : Unseen(off, items, [u] { return u; }, n_items) {}
    // user() is asked for the user only where there are lists (sample.hip divides for the row of a draw only then).
    template <class User>
    __device__ __forceinline__ Unseen(const long long* off, const int32_t* items, User&& user, const int n_items) {
        if (off) {
            const int u = user();
            from = off[u];
            s = off[u + 1] - from;
        }
        list = items + from;
        cnt = (long long)n_items - s;
    }
};

// The uniform draw of counter c among the items that are not in the set's list: the mix, the rank, the search.  cnt > 0.
__device__ __forceinline__ int32_t draw_uniform(const Unseen& set, const unsigned long long seed, const unsigned long long c) {
    const unsigned long long r = draw_mix32(seed, c);
    return draw_unseen_at(set.list, set.s, (long long)((r * (unsigned long long)set.cnt) >> 32));
}

// The weighted draw of counter c for a user whose unseen weight cnt > 0 is known: the mix, the rank within cnt, the two
// searches.  mass is the index's table (parallel to its items), C the prefix of the n_items weights.
__device__ __forceinline__ int32_t draw_weighted_of(const Unseen& set, const unsigned long long* __restrict__ mass,
                                                    const unsigned long long* __restrict__ C, const int n_items,
                                                    const unsigned long long cnt, const unsigned long long seed,
                                                    const unsigned long long c) {
    return draw_weighted_at(set.list, mass + set.from, set.s, C, n_items, cnt, __umul64hi(draw_mix64(seed, c), cnt));
}

// The same for a caller that does not know it: cnt receives the unseen weight of the set's user, and the draw is -1 when
// that is 0: everything of positive weight is seen.
__device__ __forceinline__ int32_t draw_weighted(const Unseen& set, const unsigned long long* __restrict__ mass,
                                                 const unsigned long long* __restrict__ C, const int n_items,
                                                 const unsigned long long seed, const unsigned long long c,
                                                 unsigned long long& cnt) {
    cnt = draw_unseen_mass(set.list, mass + set.from, set.s, C, n_items);
    int32_t item = -1;
    if (cnt > 0) item = draw_weighted_of(set, mass, C, n_items, cnt, seed, c);
    return item;
}

// The draw as a policy of the kernels that score their draws (pick.hip, foldin_pairwise.hip), so that each of them is
// ONE definition for both draws.  A policy says what a user has to draw from -- mass(): the number of unseen items, or
// their weight; nothing is drawn for a user whose mass is 0 -- makes the draw of a counter for a user whose mass is
// known and above 0, and carries what the draw reads beside the lists.  Both are passed to kernels by value.
struct UniformDraw {
    __device__ __forceinline__ unsigned long long mass(const Unseen& set, const int) const { return (unsigned long long)set.cnt; }
    __device__ __forceinline__ int32_t draw(const Unseen& set, const int, const unsigned long long,
                                            const unsigned long long seed, const unsigned long long c) const {
        return draw_uniform(set, seed, c);
    }
    __device__ __forceinline__ void report(const long long, const unsigned long long) const {}
};

// g: the unseen-mass table of the lists the kernel draws from (parallel to their items; never read where every list is
// empty), C: the prefix of the n_items weights, row_mass (nullable): where report() puts the mass of row x.
struct WeightedDraw {
    const unsigned long long* g;
    const unsigned long long* C;
    long long* row_mass;
    __device__ __forceinline__ unsigned long long mass(const Unseen& set, const int n_items) const {
        return draw_unseen_mass(set.list, g + set.from, set.s, C, n_items);
    }
    __device__ __forceinline__ int32_t draw(const Unseen& set, const int n_items, const unsigned long long cnt,
                                            const unsigned long long seed, const unsigned long long c) const {
        return draw_weighted_of(set, g, C, n_items, cnt, seed, c);
    }
    __device__ __forceinline__ void report(const long long x, const unsigned long long cnt) const {
        if (row_mass) row_mass[x] = (long long)cnt;
    }
};

}  // namespace
}  // namespace mfsgd
