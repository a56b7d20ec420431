// sample.hip -- draws among the items a user has NOT seen, uniform (mfsgd_sample_unseen) or in proportion to the items'
// weights (mfsgd_sample_unseen_weighted), read off the seen-item index where it lies (handle.hpp, Seen; seen.hip).
// Integers only.  The draws themselves are draw.hpp's, which states them: the mix of (seed, counter), the rank t among
// the unseen items or their weight, and the search for what holds that rank.
// One thread per draw, one store per draw (the first draw of a row also stores the row's unseen weight, when asked).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "draw.hpp"
#include "kernels.hpp"

namespace mfsgd {

namespace {

constexpr int kSampleThreads = 256;

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
    const Unseen set(off, items, [&] { return users[x / m]; }, n_items);
    int32_t item = -1;  // the user has seen everything
    if (set.cnt > 0) item = draw_uniform(set, seed, first + (unsigned long long)x);
    out[x] = item;
}

// The same with weights: mass parallels items, C is the prefix of the n_items weights; row_mass[x / m] (nullable)
// receives the unseen weight of the row's user.
__global__ void __launch_bounds__(kSampleThreads) sample_weighted_kernel(
    const long long* __restrict__ off, const int32_t* __restrict__ items, const unsigned long long* __restrict__ mass,
    const unsigned long long* __restrict__ C, const int32_t* __restrict__ users, const long long n_draws, const int m,
    const int n_items, const unsigned long long seed, const unsigned long long first, int32_t* __restrict__ out,
    long long* __restrict__ row_mass) {
    const long long x = (long long)blockIdx.x * kSampleThreads + threadIdx.x;
    if (x >= n_draws) return;
    const Unseen set(off, items, [&] { return users[x / m]; }, n_items);
    unsigned long long cnt;
    out[x] = draw_weighted(set, mass, C, n_items, seed, first + (unsigned long long)x, cnt);
    if (row_mass && x % m == 0) row_mass[x / m] = (long long)cnt;
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

hipError_t sample_weighted_draws(const long long* off, const int32_t* items, const unsigned long long* mass,
                                 const unsigned long long* C, const int32_t* users, int64_t n_draws, int32_t m, int32_t n_items,
                                 int64_t seed, uint64_t first, int32_t* out, long long* row_mass, hipStream_t st) {
    if (n_draws <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n_draws + kSampleThreads - 1) / kSampleThreads);  // (a piece: below 2^31 draws)
    hipLaunchKernelGGL(sample_weighted_kernel, dim3(blocks), dim3(kSampleThreads), 0, st, off, items, mass, C, users,
                       (long long)n_draws, (int)m, (int)n_items, (unsigned long long)seed, (unsigned long long)first, out, row_mass);
    return hipGetLastError();
}

}  // namespace mfsgd
