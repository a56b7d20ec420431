// sample.hip -- uniform draws among the items a user has NOT seen (mfsgd_sample_unseen), read off the seen-item index
// where it lies (handle.hpp, Seen; seen.hip).  Integers only.
// A draw is a pure function of (seed, its counter c), the user's sorted, distinct list S (length s) and the item count:
//     r   = the upper 32 bits of splitmix64's output for the state seed + golden * (c + 1)
//     t   = (r * cnt) >> 32 with cnt = n_items - s: the rank of the draw among the unseen items, in [0, cnt)
//     out = t + p, p = the number of positions q < s with S[q] - q <= t
// S[q] - q is the number of unseen items below S[q] and never decreases, so p is a binary search; t + p is the t-th
// unseen item in ascending order.  Exact and without rejection: no draw is ever retried, whatever share of the items
// the user has seen, and a draw costs O(log s) dependent loads.  One thread per draw, one store per draw.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace mfsgd {

namespace {

constexpr int kSampleThreads = 256;

__device__ __forceinline__ unsigned long long splitmix64(const unsigned long long seed, const unsigned long long c) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (c + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// out[x] for the draws x < n_draws of a piece: draw x belongs to row x / m of users and has the counter first + x.
// off == nullptr: an index without pairs, every list is empty.
__global__ void __launch_bounds__(kSampleThreads) sample_unseen_kernel(const long long* __restrict__ off,
                                                                       const int32_t* __restrict__ items,
                                                                       const int32_t* __restrict__ users, const long long n_draws,
                                                                       const int m, const int n_items,
                                                                       const unsigned long long seed,
                                                                       const unsigned long long first,
                                                                       int32_t* __restrict__ out) {
    const long long x = (long long)blockIdx.x * kSampleThreads + threadIdx.x;
    if (x >= n_draws) return;
    long long from = 0, s = 0;
    if (off) {
        const int u = users[x / m];
        from = off[u];
        s = off[u + 1] - from;
    }
    const long long cnt = (long long)n_items - s;
    int32_t item = -1;  // the user has seen everything
    if (cnt > 0) {
        const unsigned long long r = splitmix64(seed, first + (unsigned long long)x) >> 32;
        const long long t = (long long)((r * (unsigned long long)cnt) >> 32);
        const int32_t* __restrict__ list = items + from;
        long long lo = 0, hi = s;  // the first q in 0 .. s with list[q] - q > t
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if ((long long)list[mid] - mid <= t) lo = mid + 1;
            else hi = mid;
        }
        item = (int32_t)(t + lo);
    }
    out[x] = item;
}

}  // namespace

hipError_t sample_unseen_draws(const long long* off, const int32_t* items, const int32_t* users, int64_t n_draws, int32_t m,
                               int32_t n_items, int64_t seed, uint64_t first, int32_t* out, hipStream_t st) {
    if (n_draws <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n_draws + kSampleThreads - 1) / kSampleThreads);  // (a piece: below 2^31 draws)
    hipLaunchKernelGGL(sample_unseen_kernel, dim3(blocks), dim3(kSampleThreads), 0, st, off, items, users, (long long)n_draws,
                       (int)m, (int)n_items, (unsigned long long)seed, (unsigned long long)first, out);
    return hipGetLastError();
}

}  // namespace mfsgd
