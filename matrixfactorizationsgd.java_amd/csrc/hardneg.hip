// hardneg.hip -- hard negatives for pairwise ranking (mfsgd_sample_unseen_hard; DESIGN.md, "Hard negatives"): per row,
// the m candidates mfsgd_sample_unseen would draw for the row's user are drawn, scored under the current factors and
// only the best-scoring one leaves the kernel.  The candidates never exist in memory.
//
// The draw is draw.hpp's (sample.hip's, by construction); the score is the canonical dot of canon.hpp, the bits
// predict_kernel returns; the pick is the rule of include/mfsgd.h: the largest non-NaN score, equal scores to the
// smaller d, a NaN loses to every non-NaN, and d = 0 when every score is a NaN.
// Build with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "canon.hpp"
#include "dispatch.hpp"
#include "draw.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {
namespace {

// Candidates of one group whose Q rows are in flight together: one 16-byte load per lane each (validate.hip,
// kPairsDepth, is the idiom).
constexpr int kHardDepth = 4;

// One lane group of L lanes per row x < n of the piece; the P row of users[x] is loaded once.  The candidates are taken
// in rounds of L: in round r lane `lig` of the group draws d = r * L + lig (counter first + x * m + d), so the binary
// searches of a round run side by side; the item ids are then handed round the group (a lane permute, no LDS memory)
// and each candidate's Q row is gathered by the whole group, kHardDepth of them in flight, and reduced.  Candidates
// are examined in ascending d, and the running best (score, d, item) is the same in every lane of the group.
// m is the same for every row, so every lane of the launch runs the same trip counts (the DPP levels of
// group_allreduce need their partner lanes live).  A step past the last candidate of a round repeats the round's first
// candidate and is dropped by a select; the groups behind row n - 1, and a row whose user has seen everything, compute
// on zeros and issue no Q loads (a branch the whole group takes alike, around the load alone).
// off == nullptr: an index without pairs, every list is empty.
template <int L, int D>
__global__ void __launch_bounds__(256) hard_negative_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                            const long long* __restrict__ off,
                                                            const int32_t* __restrict__ items,
                                                            const int32_t* __restrict__ users, const long long n,
                                                            const int m, const int n_items, const unsigned long long seed,
                                                            const unsigned long long first, int32_t* __restrict__ out_items,
                                                            float* __restrict__ out_scores, int32_t* __restrict__ out_draw) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;  // groups per block
    const int lig = threadIdx.x % L;
    const long long x = (long long)blockIdx.x * GPB + threadIdx.x / L;
    const bool row = x < n;
    long long from = 0, s = 0;
    int u = 0;
    if (row) {
        u = users[x];
        if (off) {
            from = off[u];
            s = off[u + 1] - from;
        }
    }
    const long long cnt = (long long)n_items - s;
    const bool live = row && cnt > 0;  // the same in every lane of a group
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) p = *reinterpret_cast<const float4*>(P + (size_t)u * KP + lig * 4);
    const int32_t* __restrict__ list = items + from;
    const unsigned long long c0 = first + (unsigned long long)x * (unsigned long long)m;

    float best_s = __builtin_bit_cast(float, kQuietNaN);
    int32_t best_d = -1, best_item = -1;
    for (long long d0 = 0; d0 < m; d0 += L) {
        const int steps = (long long)m - d0 < L ? (int)(m - d0) : L;  // candidates of this round: 1 .. L
        int32_t mine = 0;                                             // this lane's draw of the round
        if (live && lig < steps) {
            const unsigned long long r = draw_mix32(seed, c0 + (unsigned long long)(d0 + lig));
            mine = draw_unseen_at(list, s, (long long)((r * (unsigned long long)cnt) >> 32));
        }
        for (int e0 = 0; e0 < steps; e0 += D) {
            int32_t it[D];
            float4 q[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const int e = e0 + j < steps ? e0 + j : 0;
                it[j] = L == 1 ? mine : __shfl(mine, e, L);
                q[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (live) q[j] = *reinterpret_cast<const float4*>(Q + (size_t)it[j] * KP + lig * 4);
            }
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float sc = group_allreduce<L>(chunk_dot(p, q[j]));
                const long long d = d0 + e0 + j;
                // ascending d: a later candidate takes over only with a larger score, or a number after nothing but NaNs
                const bool take = e0 + j < steps && (d == 0 || sc > best_s || (best_s != best_s && sc == sc));
                best_s = take ? sc : best_s;
                best_d = take ? (int32_t)d : best_d;
                best_item = take ? it[j] : best_item;
            }
        }
    }
    if (row && lig == 0) {
        const bool none = cnt <= 0;  // the user has seen everything
        out_items[x] = none ? -1 : best_item;
        if (out_scores) out_scores[x] = none ? __builtin_bit_cast(float, kQuietNaN) : best_s;
        if (out_draw) out_draw[x] = none ? -1 : best_d;
    }
}

}  // namespace

hipError_t launch_hard_negatives(int L, const float* P, const float* Q, const long long* off, const int32_t* items,
                                 const int32_t* users, int64_t n, int32_t m, int32_t n_items, int64_t seed, uint64_t first,
                                 int32_t* out_items, float* out_scores, int32_t* out_draw, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (m < 1) return hipErrorInvalidValue;
    const int gpb = 256 / L;
    const dim3 grid((unsigned)((n + gpb - 1) / gpb)), block(256);  // (a piece: at most 2^22 rows)
    return with_L(L, [&](auto l) {
        hipLaunchKernelGGL((hard_negative_kernel<l(), kHardDepth>), grid, block, 0, st, P, Q, off, items, users, (long long)n,
                           (int)m, (int)n_items, (unsigned long long)seed, (unsigned long long)first, out_items, out_scores,
                           out_draw);
        return hipGetLastError();
    });
}

}  // namespace mfsgd
