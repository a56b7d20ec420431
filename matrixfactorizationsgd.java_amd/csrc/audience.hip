// audience.hip -- the seen-item index read by item (mfsgd_recommend_users_unseen): the index is CSR by user, and the
// audience of an item leaves out "the users whose list holds this item".  Nothing by item is kept in the handle: per
// call one pass over the D pairs of the index picks those of the requested items and emits them as the keys
// slot << 32 | user, which then go the way of a caller's exclusion pairs (recommend_excl_lists: sorted and distinct,
// one ascending user list per slot).  Integers only.
// Cost per call: two passes (one that counts, one that writes) of 4 D bytes of items read each, a search of
// log2(n_users) steps through the offsets for each pair that is kept, and one 8-byte key written per kept pair; the
// host stages 20 bytes per kept pair for them (two key buffers for the sort and the lists' 4-byte users, serve_lists.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"

namespace mfsgd {

namespace {

constexpr int kAudienceThreads = 256;

// One thread per pair q of the index {off, items}: where its item has a slot (slot_of_item[n_items], -1 for the rest),
// the pair's user u -- the one with off[u] <= q < off[u + 1], found by one binary search over off[0 .. n_users]; lists
// that are empty share their start with the next one and never own a pair -- goes to keys[...] as slot << 32 | u.  One
// atomic per wave, as in excl_filter_kernel; keys == nullptr: the pairs are counted only.  At most cap keys are written.
__global__ void __launch_bounds__(kAudienceThreads) audience_keys_kernel(const int32_t* __restrict__ slot_of_item,
                                                                         const int n_items, const long long* __restrict__ off,
                                                                         const int32_t* __restrict__ items, const int n_users,
                                                                         const long long total,
                                                                         unsigned long long* __restrict__ keys,
                                                                         unsigned long long* __restrict__ count,
                                                                         const unsigned long long cap) {
    const int lane = threadIdx.x & 63;
    for (long long q0 = (long long)blockIdx.x * kAudienceThreads; q0 < total; q0 += (long long)gridDim.x * kAudienceThreads) {
        const long long q = q0 + threadIdx.x;
        int s = -1;
        if (q < total) {
            const unsigned item = (unsigned)items[q];
            if (item < (unsigned)n_items) s = slot_of_item[item];
        }
        const unsigned long long m = __ballot(s >= 0);
        if (m == 0ull) continue;  // wave-uniform
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(count, (unsigned long long)__popcll(m));
        if (!keys) continue;  // (a kernel argument: uniform)
        base = __shfl(base, 0, 64);
        const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (s >= 0 && at < cap) {
            int lo = 0, hi = n_users - 1;  // the first u with off[u + 1] > q: the entries above off[n_users] are not read
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (off[mid + 1] <= q) lo = mid + 1;
                else hi = mid;
            }
            keys[at] = ((unsigned long long)(unsigned)s << 32) | (unsigned)lo;
        }
    }
}

}  // namespace

hipError_t seen_audience_keys(const int32_t* slot_of_item, int32_t n_items, const long long* off, const int32_t* items,
                              int32_t n_users, int64_t total, unsigned long long* keys, unsigned long long* count, int64_t cap,
                              hipStream_t st) {
    if (total <= 0 || n_users <= 0 || n_items <= 0) return hipSuccess;
    const long long blocks = std::min<long long>((total + kAudienceThreads - 1) / kAudienceThreads, 4096);
    hipLaunchKernelGGL(audience_keys_kernel, dim3((unsigned)blocks), dim3(kAudienceThreads), 0, st, slot_of_item, (int)n_items,
                       off, items, (int)n_users, (long long)total, keys, count, (unsigned long long)cap);
    return hipGetLastError();
}

}  // namespace mfsgd
