// rank.hip -- where held-out items land in a user's recommendation order (mfsgd_rank_items): for each pair
// (user, item t) the number of eligible items that come before t, "before" being the order of recommend.hip -- the
// larger canonical dot, ties by the smaller item index.  A rank is a count, so nothing is selected or sorted and no
// score goes to memory: a workgroup holds the rows of kRankUsers distinct users in registers, streams Q once and dots
// every row it loads with all of them.  A user's held-out items are thresholds: scored first, sorted in LDS as 64-bit
// keys (order_key << 32 | ~item, so that "comes before" is "has the larger key"), and every scored item is counted
// into the bucket of the number of thresholds it beats; suffix sums over the buckets are the ranks.  A second pass
// over the user's exclusion list (the sorted distinct lists of recommend.hip) scores those items again and takes
// them out of the buckets.  A key that equals a threshold's is that item itself: neither counted nor taken out.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "canon.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {

namespace {

// float -> unsigned whose order is the float order (-0 counts as +0, as a comparison would): recommend.hip's
__device__ __forceinline__ unsigned order_key(float f) {
    unsigned u = __builtin_bit_cast(unsigned, f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long rank_key(float d, int item) {
    return ((unsigned long long)order_key(d) << 32) | (unsigned)~item;
}

// Users per workgroup.  Each costs one float4 of row per lane and one dot per loaded Q row, and every Q row loaded is
// used that many times.  What limits the count is the register file at L = 64 (k = 256): hipcc
// -Rpass-analysis=kernel-resource-usage (gfx950) gives, for 2 / 4 / 8 users, 78 / 108 / 156 VGPRs, no scratch in any
// of them, hence 6 / 4 / 3 waves per SIMD = 3 / 2 / 1 workgroups of 8 waves per CU (LDS: 14 / 28 / 56 KiB each, never
// the limit).  4 and 8 users both keep 8 users' rows resident per CU, but 8 do it with half the waves, and the loop is
// a row gather from L2 that lives on the loads in flight; 2 users halve the reuse of every load.  Hence 4.  It is also
// what the counting step can use at k <= 16: one user per lane of a 4-lane group.
constexpr int kRankUsers = 4;
constexpr int kRankCap = 512;      // thresholds per user and round; a user with more pairs takes several rounds
constexpr int kRankThreads = 512;  // 8 waves
static_assert(kRankThreads / 64 >= kRankUsers, "the suffix sums take one wave per user");
static_assert(kRankCap % 64 == 0 && (kRankCap & (kRankCap - 1)) == 0, "bitonic sort, 64-lane suffix scan");

// thresholds below `key` among the n2 (a power of two, padded with all-ones) sorted keys of one user
__device__ __forceinline__ int beaten(const unsigned long long* thr, const int n2, const unsigned long long key) {
    int c = 0;
    for (int step = n2; step > 0; step >>= 1)
        if (c + step <= n2 && thr[c + step - 1] < key) c += step;
    return c;
}

// Slot s = blockIdx.x * kRankUsers + j is user rows[s]; its pairs are items[off[s] - base .. off[s + 1] - base), and
// out[...] at the same places receives their ranks.  ex_off / ex_items: RecommendExcl's lists of the same slots
// (ex_off == nullptr: none).  BY_USER: the lists are indexed by user instead, slot s having that of rows[s] (the
// seen-item index of the handle, read where it lies).
template <int L, bool BY_USER>
__global__ void __launch_bounds__(kRankThreads) rank_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                            const int32_t* __restrict__ rows, const int n_slots,
                                                            const long long* __restrict__ off, const long long base,
                                                            const int32_t* __restrict__ items, const int32_t n_items,
                                                            const long long* __restrict__ ex_off,
                                                            const int32_t* __restrict__ ex_items, int32_t* __restrict__ out) {
    constexpr int NT = kRankThreads, UPW = kRankUsers, CAP = kRankCap;
    constexpr int KP = 4 * L;
    constexpr int GPB = NT / L;
    constexpr int R = (UPW + L - 1) / L;  // users a lane counts for: lane `lig` of a group takes users lig, lig + L, ...
    __shared__ unsigned long long keys[UPW][CAP];  // the thresholds of the round, ascending
    __shared__ unsigned short place[UPW][CAP];     // ... and which pair of the round each is
    __shared__ int bucket[UPW][CAP + 1];           // [c]: items that beat exactly the c lowest thresholds (c >= 1)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lig = tid % L, grp = tid / L;
    const int s0 = (int)blockIdx.x * UPW;

    float4 p[UPW];
    int t_n[UPW];  // pairs of each user
    int rounds = 0;
#pragma unroll
    for (int j = 0; j < UPW; ++j) {
        const bool have = s0 + j < n_slots;  // (the last workgroup may hold fewer users: the others have no pairs)
        const int s = have ? s0 + j : s0;
        p[j] = *reinterpret_cast<const float4*>(P + (size_t)rows[s] * KP + lig * 4);
        t_n[j] = have ? (int)(off[s + 1] - off[s]) : 0;
        rounds = max(rounds, (t_n[j] + CAP - 1) / CAP);
    }

    // A round is a pass over Q for the whole workgroup: the users with fewer pairs than its longest dot every row again
    // for nothing in the later rounds.  The host hands the slots over sorted by pair count, so that users who need
    // several rounds sit in the same workgroups.
    for (int rd = 0; rd < rounds; ++rd) {
        int n[UPW], n2[UPW];
        // ---- the thresholds of this round: scored, then sorted ---------------------------------------------------
#pragma unroll
        for (int j = 0; j < UPW; ++j) {
            n[j] = min(max(t_n[j] - rd * CAP, 0), CAP);
            n2[j] = n[j] <= 1 ? 1 : 1 << (32 - __builtin_clz((unsigned)(n[j] - 1)));  // the power of two >= n
            const long long at = n[j] > 0 ? off[s0 + j] - base + (long long)rd * CAP : 0;
            const int iters = (n[j] + GPB - 1) / GPB;  // uniform trip count: the DPP reduction needs every lane live
            for (int it = 0; it < iters; ++it) {
                const int x = grp + it * GPB;
                const bool ok = x < n[j];
                const int item = ok ? items[at + x] : 0;
                const float4 q = *reinterpret_cast<const float4*>(Q + (size_t)item * KP + lig * 4);
                const float d = group_allreduce<L>(chunk_dot(p[j], q));
                if (ok && lig == 0) {
                    keys[j][x] = rank_key(d, item);
                    place[j][x] = (unsigned short)x;
                }
            }
            for (int x = n[j] + tid; x < n2[j]; x += NT) {
                keys[j][x] = ~0ull;  // (sorts behind every real key: none is all-ones but a NaN score's at item 0)
                place[j][x] = 0;
            }
            for (int x = tid; x <= n[j]; x += NT) bucket[j][x] = 0;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < UPW; ++j)
            for (int size = 2; size <= n2[j]; size <<= 1)
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int x = tid; x < n2[j] / 2; x += NT) {
                        const int i0 = 2 * x - (x & (stride - 1)), i1 = i0 + stride;
                        const bool up = (i0 & size) == 0;
                        const unsigned long long a0 = keys[j][i0], a1 = keys[j][i1];
                        if ((a0 > a1) == up) {
                            const unsigned short b0 = place[j][i0];
                            keys[j][i0] = a1;
                            keys[j][i1] = a0;
                            place[j][i0] = place[j][i1];
                            place[j][i1] = b0;
                        }
                    }
                    __syncthreads();
                }
        // what this lane counts: its users' lowest and highest thresholds stay in registers, since most items lie
        // below the one or above the other; the items above every threshold are counted in a register too
        unsigned long long t_min[R], t_max[R];
        int above[R], t_n2[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int uu = r * L + lig;
            int nn = 0;
            t_n2[r] = 1;
#pragma unroll
            for (int j = 0; j < UPW; ++j) {
                nn = uu == j ? n[j] : nn;
                t_n2[r] = uu == j ? n2[j] : t_n2[r];
            }
            const bool any = uu < UPW && nn > 0;
            t_min[r] = any ? keys[uu][0] : ~0ull;  // (no key is above all-ones)
            t_max[r] = any ? keys[uu][nn - 1] : ~0ull;
            above[r] = 0;
        }
        // ---- every item against the users' rows -----------------------------------------------------------------
        // d[r]: the item's score for user r * L + lig
        auto count = [&](const float (&d)[R], const int item) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const unsigned long long key = rank_key(d[r], item);
                if (key > t_max[r]) {
                    ++above[r];
                } else if (key > t_min[r]) {
                    const int uu = r * L + lig;
                    atomicAdd(&bucket[uu][beaten(keys[uu], t_n2[r], key)], 1);
                }
            }
        };
        // the scores of one Q row for all users, each lane keeping those of the users it counts for
        auto scores = [&](const float4 q, float (&d)[R]) {
#pragma unroll
            for (int j = 0; j < UPW; ++j) {
                const float dj = group_allreduce<L>(chunk_dot(p[j], q));
#pragma unroll
                for (int r = 0; r < R; ++r) d[r] = (j == 0 || r * L + lig == j) ? dj : d[r];
            }
        };
        const int iters = (n_items + GPB - 1) / GPB;  // uniform trip count, two rows in flight
        int it = 0;
        for (; it + 1 < iters; it += 2) {
            const int i0 = grp + it * GPB, i1 = i0 + GPB;
            const bool ok1 = i1 < n_items;
            const float4 q0 = *reinterpret_cast<const float4*>(Q + (size_t)i0 * KP + lig * 4);
            const float4 q1 = *reinterpret_cast<const float4*>(Q + (size_t)(ok1 ? i1 : 0) * KP + lig * 4);
            float d0[R], d1[R];
            scores(q0, d0);
            scores(q1, d1);
            count(d0, i0);
            if (ok1) count(d1, i1);
        }
        for (; it < iters; ++it) {
            const int i = grp + it * GPB;
            const bool ok = i < n_items;
            const float4 q = *reinterpret_cast<const float4*>(Q + (size_t)(ok ? i : 0) * KP + lig * 4);
            float d[R];
            scores(q, d);
            if (ok) count(d, i);
        }
        // ---- the excluded items were counted like any other: out again -------------------------------------------
#pragma unroll
        for (int j = 0; j < UPW; ++j) {
            if (n[j] == 0 || !ex_off) continue;  // (uniform)
            const int xs = BY_USER ? rows[s0 + j] : s0 + j;  // (n[j] > 0: the slot exists)
            const long long x_at = ex_off[xs], len = ex_off[xs + 1] - x_at;
            const long long xiters = (len + GPB - 1) / GPB;
            for (long long xt = 0; xt < xiters; ++xt) {
                const long long x = grp + xt * GPB;
                const bool ok = x < len;
                const int item = ok ? ex_items[x_at + x] : 0;
                const float4 q = *reinterpret_cast<const float4*>(Q + (size_t)item * KP + lig * 4);
                const float d = group_allreduce<L>(chunk_dot(p[j], q));
                if (ok && lig == 0) {
                    const int c = beaten(keys[j], n2[j], rank_key(d, item));
                    if (c > 0) atomicSub(&bucket[j][c], 1);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int uu = r * L + lig;
            int nn = 0;
#pragma unroll
            for (int j = 0; j < UPW; ++j) nn = uu == j ? n[j] : nn;
            if (uu < UPW && above[r] != 0) atomicAdd(&bucket[uu][nn], above[r]);
        }
        __syncthreads();
        // ---- rank of the threshold at place x = the items in the buckets above x: wave j sums user j's ------------
        if (wave < UPW) {
            int nn = 0;
#pragma unroll
            for (int j = 0; j < UPW; ++j) nn = wave == j ? n[j] : nn;
            const long long at = nn > 0 ? off[s0 + wave] - base + (long long)rd * CAP : 0;
            constexpr int PER = CAP / 64;  // lane l owns buckets l * PER + 1 .. l * PER + PER
            int b[PER], own = 0;
#pragma unroll
            for (int y = 0; y < PER; ++y) {
                const int c = lane * PER + 1 + y;
                b[y] = c <= nn ? bucket[wave][c] : 0;
                own += b[y];
            }
            int incl = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_down(incl, d, 64);
                if (lane + d < 64) incl += o;
            }
            int run = incl - own;  // the buckets of the lanes above
#pragma unroll
            for (int y = PER - 1; y >= 0; --y) {
                run += b[y];
                const int x = lane * PER + y;  // bucket x + 1 and everything above it
                if (x < nn) out[at + place[wave][x]] = run;
            }
        }
        __syncthreads();  // the tables are rebuilt in the next round
    }
}

}  // namespace

hipError_t launch_rank_items(int L, const float* P, const float* Q, const int32_t* rows, int n_slots, const long long* off,
                             long long base, const int32_t* items, int32_t n_items, const RecommendExcl& ex,
                             int32_t* out, hipStream_t st, bool ex_by_user) {
    if (n_slots <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n_slots + kRankUsers - 1) / kRankUsers));
    return with_L(L, [&](auto l) {
        if (ex_by_user)
            hipLaunchKernelGGL((rank_kernel<l(), true>), grid, dim3(kRankThreads), 0, st, P, Q, rows, n_slots, off, base, items,
                               n_items, ex.off, ex.items, out);
        else
            hipLaunchKernelGGL((rank_kernel<l(), false>), grid, dim3(kRankThreads), 0, st, P, Q, rows, n_slots, off, base, items,
                               n_items, ex.off, ex.items, out);
        return hipGetLastError();
    });
}

}  // namespace mfsgd
