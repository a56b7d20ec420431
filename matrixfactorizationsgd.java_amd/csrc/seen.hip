// seen.hip -- the seen-item index of a handle (mfsgd_set_seen, mfsgd_mark_seen, mfsgd_get_seen): one sorted, distinct
// item list per user in CSR form, items[off[u] .. off[u + 1]), off having an entry per user of capacity plus one (every
// entry from the user count on holds the total), and beside it the identity slot table through which the EXCL kernels
// of recommend.hip reach a list by user id.  Integers only.
// Building it from pairs is recommend.hip's (recommend_excl_lists); what lives here is the first step of that (a pair
// to its key user << 32 | item), the merge of a sorted distinct batch into an index that is not sorted again, the
// tables of a larger capacity, the gather of requested lists, the histogram of the items over the lists
// (mfsgd_seen_item_counts), and the unseen-mass table of the weighted draw (Seen::mass): the pairs' weights, one
// device-wide exclusive scan of them (rocPRIM), and per pair the weight below its item less the seen weight before it in
// its list.
// The merge: every output element is placed on its own.  A batch key is new when a binary search of its user's old list
// misses it; off' = off + the new keys of the users before; an old element lands at off'[u] + its old position + the
// user's new keys below it, a new key at off'[u] + its position among the user's new keys + the old items below it.
// No loop runs over a user's list, so a user with 10^5 items costs what 10^5 users with one do.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"

namespace mfsgd {

namespace {

constexpr int kSeenThreads = 256;

inline unsigned seen_blocks(long long work) {
    return (unsigned)std::min<long long>((work + kSeenThreads - 1) / kSeenThreads, 4096);
}

// first position in a[lo .. hi) whose element is not below v
template <class T>
__device__ __forceinline__ long long lower_bound(const T* __restrict__ a, long long lo, long long hi, const T v) {
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kSeenThreads) pair_keys_kernel(const int32_t* __restrict__ u, const int32_t* __restrict__ i,
                                                                 const long long n, unsigned long long* __restrict__ keys) {
    const long long stride = (long long)gridDim.x * kSeenThreads;
    for (long long x = (long long)blockIdx.x * kSeenThreads + threadIdx.x; x < n; x += stride)
        keys[x] = ((unsigned long long)(unsigned)u[x] << 32) | (unsigned)i[x];
}

// off2[x] = old_off[x] for x <= old_cap and `total` above (off2 == nullptr: not written); slot[x] = x for x < new_cap
__global__ void __launch_bounds__(kSeenThreads) tables_kernel(const long long* __restrict__ old_off, const int old_cap,
                                                              const long long total, const int new_cap,
                                                              long long* __restrict__ off2, int32_t* __restrict__ slot) {
    const long long stride = (long long)gridDim.x * kSeenThreads;
    for (long long x = (long long)blockIdx.x * kSeenThreads + threadIdx.x; x <= new_cap; x += stride) {
        if (off2) off2[x] = x <= old_cap ? old_off[x] : total;
        if (x < new_cap) slot[x] = (int32_t)x;
    }
}

// flags[x] = 1 where batch key x (of the *n_keys sorted distinct ones; flags has m >= *n_keys entries) is not in the index
__global__ void __launch_bounds__(kSeenThreads) flag_new_kernel(const unsigned long long* __restrict__ keys,
                                                                const unsigned* __restrict__ n_keys, const long long m,
                                                                const long long* __restrict__ off,
                                                                const int32_t* __restrict__ items,
                                                                unsigned char* __restrict__ flags) {
    const long long n = *n_keys;
    const long long stride = (long long)gridDim.x * kSeenThreads;
    for (long long x = (long long)blockIdx.x * kSeenThreads + threadIdx.x; x < m; x += stride) {
        unsigned char fresh = 0;
        if (x < n) {
            const int u = (int)(keys[x] >> 32), item = (int)(keys[x] & 0xFFFFFFFFull);
            const long long hi = off[u + 1], at = lower_bound(items, off[u], hi, item);
            fresh = !(at < hi && items[at] == item);
        }
        flags[x] = fresh;
    }
}

// off2[u] = off[u] + the new keys of the users before u, for u = 0 .. cap
__global__ void __launch_bounds__(kSeenThreads) merge_off_kernel(const long long* __restrict__ off, const int cap,
                                                                 const unsigned long long* __restrict__ fresh,
                                                                 const long long n_fresh, long long* __restrict__ off2) {
    const long long stride = (long long)gridDim.x * kSeenThreads;
    for (long long u = (long long)blockIdx.x * kSeenThreads + threadIdx.x; u <= cap; u += stride)
        off2[u] = off[u] + lower_bound(fresh, 0, n_fresh, (unsigned long long)u << 32);
}

// the old elements to their new places.  The user of position x is the last u with off[u] <= x (an empty list shares
// its start with the next one; off[cap] = total lies above every x).
__global__ void __launch_bounds__(kSeenThreads) merge_old_kernel(const long long* __restrict__ off,
                                                                 const int32_t* __restrict__ items, const long long total,
                                                                 const int cap, const unsigned long long* __restrict__ fresh,
                                                                 const long long* __restrict__ off2,
                                                                 int32_t* __restrict__ items2) {
    const long long stride = (long long)gridDim.x * kSeenThreads;
    for (long long x = (long long)blockIdx.x * kSeenThreads + threadIdx.x; x < total; x += stride) {
        long long lo = 0, hi = cap;  // the first u in 0 .. cap with off[u] > x
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (off[mid] <= x) lo = mid + 1;
            else hi = mid;
        }
        const long long u = lo - 1;
        const int item = items[x];
        const long long f0 = off2[u] - off[u], f1 = off2[u + 1] - off[u + 1];  // the user's new keys: fresh[f0 .. f1)
        long long below = 0;
        if (f1 > f0) below = lower_bound(fresh, f0, f1, ((unsigned long long)u << 32) | (unsigned)item) - f0;
        items2[off2[u] + (x - off[u]) + below] = item;
    }
}

// ... and the new keys to theirs
__global__ void __launch_bounds__(kSeenThreads) merge_new_kernel(const unsigned long long* __restrict__ fresh,
                                                                 const long long n_fresh, const long long* __restrict__ off,
                                                                 const int32_t* __restrict__ items,
                                                                 const long long* __restrict__ off2,
                                                                 int32_t* __restrict__ items2) {
    const long long stride = (long long)gridDim.x * kSeenThreads;
    for (long long x = (long long)blockIdx.x * kSeenThreads + threadIdx.x; x < n_fresh; x += stride) {
        const int u = (int)(fresh[x] >> 32), item = (int)(fresh[x] & 0xFFFFFFFFull);
        const long long f0 = off2[u] - off[u];
        const long long below = lower_bound(items, off[u], off[u + 1], item) - off[u];
        items2[off2[u] + (x - f0) + below] = item;
    }
}

__global__ void __launch_bounds__(kSeenThreads) lengths_kernel(const long long* __restrict__ off,
                                                               const int32_t* __restrict__ users, const int n,
                                                               long long* __restrict__ len) {
    const int stride = (int)gridDim.x * kSeenThreads;
    for (int b = (int)blockIdx.x * kSeenThreads + threadIdx.x; b < n; b += stride) len[b] = off[users[b] + 1] - off[users[b]];
}

// out[row_ptr[b] ...] = the list of users[b]: workgroups (x, y) take the rows x, x + gridDim.x, ... and of each the
// positions of part y
__global__ void __launch_bounds__(kSeenThreads) gather_kernel(const long long* __restrict__ off,
                                                              const int32_t* __restrict__ items,
                                                              const int32_t* __restrict__ users, const int n,
                                                              const long long* __restrict__ row_ptr, int32_t* __restrict__ out) {
    const long long stride = (long long)gridDim.y * kSeenThreads;
    for (int b = (int)blockIdx.x; b < n; b += (int)gridDim.x) {
        const long long from = off[users[b]], len = off[users[b] + 1] - from, to = row_ptr[b];
        for (long long x = (long long)blockIdx.y * kSeenThreads + threadIdx.x; x < len; x += stride) out[to + x] = items[from + x];
    }
}

// C[min(x, n_w)]: the prefix of n_w item weights read for an item count that may have grown past them (items appended
// since weigh nothing)
__device__ __forceinline__ unsigned long long prefix_at(const unsigned long long* __restrict__ C, const int n_w, const long long x) {
    return C[x < n_w ? x : n_w];
}

// w[x] = the weight of items[x]
__global__ void __launch_bounds__(kSeenThreads) pair_weights_kernel(const int32_t* __restrict__ items, const long long total,
                                                                    const unsigned long long* __restrict__ C, const int n_w,
                                                                    unsigned long long* __restrict__ w) {
    const long long stride = (long long)gridDim.x * kSeenThreads;
    for (long long x = (long long)blockIdx.x * kSeenThreads + threadIdx.x; x < total; x += stride)
        w[x] = prefix_at(C, n_w, (long long)items[x] + 1) - prefix_at(C, n_w, items[x]);
}

// mass[x] = C[items[x]] - (G[x] - G[off[u]]), u the user of position x (found as merge_old_kernel finds it) and G the
// exclusive scan of the pairs' weights over the whole index, which wraps: only differences inside one list are used
__global__ void __launch_bounds__(kSeenThreads) unseen_mass_kernel(const long long* __restrict__ off,
                                                                   const int32_t* __restrict__ items, const long long total,
                                                                   const int cap, const unsigned long long* __restrict__ C,
                                                                   const int n_w, const unsigned long long* __restrict__ G,
                                                                   unsigned long long* __restrict__ mass) {
    const long long stride = (long long)gridDim.x * kSeenThreads;
    for (long long x = (long long)blockIdx.x * kSeenThreads + threadIdx.x; x < total; x += stride) {
        long long lo = 0, hi = cap;  // the first u in 0 .. cap with off[u] > x
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (off[mid] <= x) lo = mid + 1;
            else hi = mid;
        }
        mass[x] = prefix_at(C, n_w, items[x]) - (G[x] - G[off[lo - 1]]);
    }
}

// counts[items[x]] += 1: integer atomics, so the sums do not depend on the order of arrival
__global__ void __launch_bounds__(kSeenThreads) item_counts_kernel(const int32_t* __restrict__ items, const long long total,
                                                                   unsigned long long* __restrict__ counts) {
    const long long stride = (long long)gridDim.x * kSeenThreads;
    for (long long x = (long long)blockIdx.x * kSeenThreads + threadIdx.x; x < total; x += stride)
        atomicAdd(&counts[items[x]], 1ull);
}

// bits of a key user << 32 | item that a sort has to look at, users being below n_users
inline unsigned key_bits(int32_t n_users) {
    unsigned end_bit = 33;
    while (end_bit < 64 && ((unsigned long long)(n_users - 1) >> (end_bit - 32)) != 0) ++end_bit;
    return end_bit;
}

}  // namespace

hipError_t seen_pair_keys(const int32_t* u, const int32_t* i, int64_t n, unsigned long long* keys, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pair_keys_kernel, dim3(seen_blocks(n)), dim3(kSeenThreads), 0, st, u, i, (long long)n, keys);
    return hipGetLastError();
}

hipError_t seen_tables(const long long* old_off, int32_t old_cap, int64_t total, int32_t new_cap, long long* off2, int32_t* slot,
                       hipStream_t st) {
    hipLaunchKernelGGL(tables_kernel, dim3(seen_blocks((long long)new_cap + 1)), dim3(kSeenThreads), 0, st, old_off, (int)old_cap,
                       (long long)total, (int)new_cap, off2, slot);
    return hipGetLastError();
}

hipError_t seen_batch_fresh(unsigned long long* keys, unsigned long long* keys_tmp, int64_t m, int32_t n_users,
                            const long long* off, const int32_t* items, unsigned char* flags, unsigned* counts, DevBuf& temp,
                            hipStream_t st) {
    const unsigned end_bit = key_bits(n_users);
    size_t need_sort = 0, need_uniq = 0, need_sel = 0;
    hipError_t e = rocprim::radix_sort_keys(nullptr, need_sort, keys, keys_tmp, (size_t)m, 0u, end_bit, st);
    if (e == hipSuccess)
        e = rocprim::unique(nullptr, need_uniq, keys_tmp, keys, counts, (size_t)m, rocprim::equal_to<unsigned long long>(), st);
    if (e == hipSuccess) e = rocprim::select(nullptr, need_sel, keys, flags, keys_tmp, counts + 1, (size_t)m, st);
    if (e == hipSuccess) e = temp.alloc(std::max(need_sort, std::max(need_uniq, need_sel)));
    if (e == hipSuccess) e = rocprim::radix_sort_keys(temp.get(), need_sort, keys, keys_tmp, (size_t)m, 0u, end_bit, st);
    if (e == hipSuccess)
        e = rocprim::unique(temp.get(), need_uniq, keys_tmp, keys, counts, (size_t)m, rocprim::equal_to<unsigned long long>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(flag_new_kernel, dim3(seen_blocks(m)), dim3(kSeenThreads), 0, st, keys, counts, (long long)m, off, items,
                       flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return rocprim::select(temp.get(), need_sel, keys, flags, keys_tmp, counts + 1, (size_t)m, st);
}

hipError_t seen_merge(const long long* off, const int32_t* items, int64_t total, int32_t cap, const unsigned long long* fresh,
                      int64_t n_fresh, long long* off2, int32_t* items2, hipStream_t st) {
    hipLaunchKernelGGL(merge_off_kernel, dim3(seen_blocks((long long)cap + 1)), dim3(kSeenThreads), 0, st, off, (int)cap, fresh,
                       (long long)n_fresh, off2);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(merge_old_kernel, dim3(seen_blocks(total)), dim3(kSeenThreads), 0, st, off, items, (long long)total, (int)cap,
                       fresh, off2, items2);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(merge_new_kernel, dim3(seen_blocks(n_fresh)), dim3(kSeenThreads), 0, st, fresh, (long long)n_fresh, off, items,
                       off2, items2);
    return hipGetLastError();
}

hipError_t seen_unseen_mass(const long long* off, const int32_t* items, int64_t total, int32_t cap, const unsigned long long* C,
                            int32_t n_w, unsigned long long* G, unsigned long long* mass, DevBuf& temp, hipStream_t st) {
    if (total <= 0) return hipSuccess;
    size_t need = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, need, mass, G, 0ull, (size_t)total, rocprim::plus<unsigned long long>(), st);
    if (e == hipSuccess) e = temp.alloc(need);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pair_weights_kernel, dim3(seen_blocks(total)), dim3(kSeenThreads), 0, st, items, (long long)total, C, (int)n_w,
                       mass);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = rocprim::exclusive_scan(temp.get(), need, mass, G, 0ull, (size_t)total, rocprim::plus<unsigned long long>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(unseen_mass_kernel, dim3(seen_blocks(total)), dim3(kSeenThreads), 0, st, off, items, (long long)total, (int)cap,
                       C, (int)n_w, G, mass);
    return hipGetLastError();
}

hipError_t seen_item_counts(const int32_t* items, int64_t total, unsigned long long* counts, hipStream_t st) {
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(item_counts_kernel, dim3(seen_blocks(total)), dim3(kSeenThreads), 0, st, items, (long long)total, counts);
    return hipGetLastError();
}

hipError_t seen_lengths(const long long* off, const int32_t* users, int32_t n, long long* len, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(lengths_kernel, dim3(seen_blocks(n)), dim3(kSeenThreads), 0, st, off, users, (int)n, len);
    return hipGetLastError();
}

hipError_t seen_gather(const long long* off, const int32_t* items, const int32_t* users, int32_t n, const long long* row_ptr,
                       int64_t longest, int32_t* out, hipStream_t st) {
    if (n <= 0 || longest <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<int32_t>(n, 4096),
                    (unsigned)std::min<long long>((longest + kSeenThreads - 1) / kSeenThreads, 64));
    hipLaunchKernelGGL(gather_kernel, grid, dim3(kSeenThreads), 0, st, off, items, users, (int)n, row_ptr, out);
    return hipGetLastError();
}

}  // namespace mfsgd
