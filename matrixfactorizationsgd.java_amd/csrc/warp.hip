// warp.hip -- the negative of a WARP step (mfsgd_sample_unseen_violating; DESIGN.md, "WARP"): per row, the m candidates
// mfsgd_sample_unseen would draw for the row's user are walked in ascending d until one violates the margin against the
// row's positive, and that one leaves the kernel with the number of draws it took.  The candidates never exist in memory.
//
// The draw is draw.hpp's (sample.hip's, by construction); the dots are the canonical dot of canon.hpp, the bits
// predict_kernel returns; x[d] = sp - dot(P[u], Q[cand[d]]) is one fp32 subtraction, the bits pairwise.hip reports as
// the margin of (u, i, cand[d]); the pick is the rule of include/mfsgd.h: the smallest d with cand[d] != i and
// x[d] < margin.  Everything past the pick is skipped; nothing of the result depends on what was skipped.
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

// Candidates of one group whose Q rows are in flight together (hardneg.hip, kHardDepth).
constexpr int kWarpDepth = 4;

// One lane group of L lanes per row x < n of the piece; P[users[x]] and Q[pos[x]] are loaded once and sp reduced once.
// The candidates are taken in rounds of L as in hardneg.hip: in round r lane `lig` draws d = r * L + lig, the item ids
// are handed round the group (a lane permute, no LDS memory), each candidate's Q row is gathered by the whole group, D
// of them in flight, and reduced; candidates are examined in ascending d, so the first violator seen is the pick.
// `need` -- the row has candidates and no pick yet -- is the same in every lane of a group.  A group without it
// branches around its draws and its Q loads (the branch hardneg.hip takes for a row without candidates) and computes
// on zeros, which a select drops: the permutes and the DPP levels of group_allreduce are never inside a branch, so
// their partner lanes are live whatever the neighbouring groups of the wave have found.  The loops are left only when
// no group of the WAVE needs anything more: a ballot, so every lane of the wave leaves at the same trip, and a wave
// shares nothing with the other waves of its workgroup (no LDS, no barrier).
// off == nullptr: an index without pairs, every list is empty.
template <int L, int D>
__global__ void __launch_bounds__(256) first_violating_kernel(
    const float* __restrict__ P, const float* __restrict__ Q, const long long* __restrict__ off, const int32_t* __restrict__ items,
    const int32_t* __restrict__ users, const int32_t* __restrict__ pos, const long long n, const int m, const float margin,
    const int n_items, const unsigned long long seed, const unsigned long long first, int32_t* __restrict__ out_items,
    int32_t* __restrict__ out_draw, float* __restrict__ out_margin, int32_t* __restrict__ out_rank) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;  // groups per block
    const int lig = threadIdx.x % L;
    const long long x = (long long)blockIdx.x * GPB + threadIdx.x / L;
    const bool row = x < n;
    long long from = 0, s = 0;
    int u = 0, ip = 0;
    if (row) {
        u = users[x];
        ip = pos[x];
        if (off) {
            from = off[u];
            s = off[u + 1] - from;
        }
    }
    const long long cnt = (long long)n_items - s;
    const bool live = row && cnt > 0;  // the same in every lane of a group
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f), qp = p;
    if (live) {
        p = *reinterpret_cast<const float4*>(P + (size_t)u * KP + lig * 4);
        qp = *reinterpret_cast<const float4*>(Q + (size_t)ip * KP + lig * 4);
    }
    const float sp = group_allreduce<L>(chunk_dot(p, qp));
    const int32_t* __restrict__ list = items + from;
    const unsigned long long c0 = first + (unsigned long long)x * (unsigned long long)m;

    float pick_x = __builtin_bit_cast(float, kQuietNaN);
    int32_t pick_d = -1, pick_item = -1;
    bool need = live;
    for (long long d0 = 0; d0 < m; d0 += L) {
        if (__builtin_amdgcn_ballot_w64(need) == 0) break;            // wave-uniform
        const int steps = (long long)m - d0 < L ? (int)(m - d0) : L;  // candidates of this round: 1 .. L
        int32_t mine = 0;                                             // this lane's draw of the round
        if (need && lig < steps) {
            const unsigned long long r = draw_mix32(seed, c0 + (unsigned long long)(d0 + lig));
            mine = draw_unseen_at(list, s, (long long)((r * (unsigned long long)cnt) >> 32));
        }
        for (int e0 = 0; e0 < steps; e0 += D) {
            if (__builtin_amdgcn_ballot_w64(need) == 0) break;  // wave-uniform; the round loop then ends at its own check
            const bool loaded = need;                           // what this group's q[] hold: rows of Q, or zeros
            int32_t it[D];
            float4 q[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const int e = e0 + j < steps ? e0 + j : 0;
                it[j] = L == 1 ? mine : __shfl(mine, e, L);
                q[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (loaded) q[j] = *reinterpret_cast<const float4*>(Q + (size_t)it[j] * KP + lig * 4);
            }
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float xd = sp - group_allreduce<L>(chunk_dot(p, q[j]));
                // ascending d: the first violator is the pick; a NaN xd compares false
                const bool take = loaded && pick_d < 0 && e0 + j < steps && it[j] != ip && xd < margin;
                pick_x = take ? xd : pick_x;
                pick_item = take ? it[j] : pick_item;
                pick_d = take ? (int32_t)(d0 + e0 + j) : pick_d;
            }
            need = live && pick_d < 0;
        }
    }
    if (row && lig == 0) {
        const bool none = cnt <= 0;  // the user has seen everything
        const bool hit = pick_d >= 0;
        out_items[x] = pick_item;
        if (out_draw) out_draw[x] = none ? -1 : hit ? pick_d : m;
        if (out_margin) out_margin[x] = pick_x;
        if (out_rank) {
            const long long rk = hit ? cnt / ((long long)pick_d + 1) : 0;
            out_rank[x] = hit ? (int32_t)(rk < 1 ? 1 : rk) : 0;
        }
    }
}

}  // namespace

hipError_t launch_first_violating(int L, const float* P, const float* Q, const long long* off, const int32_t* items,
                                  const int32_t* users, const int32_t* pos, int64_t n, int32_t m, float margin, int32_t n_items,
                                  int64_t seed, uint64_t first, int32_t* out_items, int32_t* out_draw, float* out_margin,
                                  int32_t* out_rank, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (m < 1) return hipErrorInvalidValue;
    const int gpb = 256 / L;
    const dim3 grid((unsigned)((n + gpb - 1) / gpb)), block(256);  // (a piece: at most 2^22 rows)
    return with_L(L, [&](auto l) {
        hipLaunchKernelGGL((first_violating_kernel<l(), kWarpDepth>), grid, block, 0, st, P, Q, off, items, users, pos, (long long)n,
                           (int)m, margin, (int)n_items, (unsigned long long)seed, (unsigned long long)first, out_items, out_draw,
                           out_margin, out_rank);
        return hipGetLastError();
    });
}

}  // namespace mfsgd
