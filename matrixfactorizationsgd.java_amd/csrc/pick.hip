// pick.hip -- the two kernels that pick one of a row's m unseen candidates under the current factors: per row, the m
// candidates mfsgd_sample_unseen would draw for the row's user are drawn and scored, and one leaves the kernel: the
// best-scoring one (mfsgd_sample_unseen_hard; DESIGN.md, "Hard negatives"), or the first in d that violates a margin
// against the row's positive, with the number of draws it took (mfsgd_sample_unseen_violating; DESIGN.md, "WARP").  The
// candidates never exist in memory.  The draw is draw.hpp's (sample.hip's, by construction); the dots are the canonical
// dot of canon.hpp, the bits predict_kernel returns.  What the kernels share -- a row's prologue, a round's draws, a
// chunk's gather, the launch -- is stated once; the loops and the rules are each kernel's own.
// The draw is a policy of the kernels (draw.hpp: UniformDraw, WeightedDraw), not a second copy of them: with
// WeightedDraw the candidates are mfsgd_sample_unseen_weighted's (mfsgd_sample_unseen_hard_weighted,
// mfsgd_sample_unseen_violating_weighted; DESIGN.md, "Weighted picks"), everything else alike.
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
constexpr int kPickDepth = 4;

// What both kernels know of their group: one lane group of L lanes per row x < n of the piece; the P row of users[x] is
// loaded once.  The groups behind row n - 1, and a row whose user has nothing to draw from (mass == 0: every item is
// seen, or with weights every item of positive weight), are not `live`: they compute on zeros and issue no loads.  Draw
// d of the row has the counter c0 + d.
// off == nullptr: an index without pairs, every list is empty.
template <int L, class Draw>
struct PickRow {
    static constexpr int KP = 4 * L;
    static constexpr int GPB = 256 / L;  // groups per block
    const int lig = threadIdx.x % L;
    const long long x = (long long)blockIdx.x * GPB + threadIdx.x / L;
    const bool row;
    const Draw& dr;
    const int n_items;
    int u = 0;
    Unseen set;                   // (empty, with nothing unseen, behind row n - 1)
    unsigned long long mass = 0;  // what the row's user has to draw from: the policy's measure of the unseen items
    bool live;                    // the same in every lane of a group
    const unsigned long long c0;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    __device__ __forceinline__ PickRow(const Draw& draw_, const float* __restrict__ P, const long long* __restrict__ off,
                                       const int32_t* __restrict__ items, const int32_t* __restrict__ users, const long long n,
                                       const int m, const int n_items_, const unsigned long long first)
        : row(x < n), dr(draw_), n_items(n_items_), c0(first + (unsigned long long)x * (unsigned long long)m) {
        if (row) {
            u = users[x];
            set = Unseen(off, items, u, n_items);
            mass = dr.mass(set, n_items);
        }
        live = row && mass > 0;
        if (live) p = q_row(P, u);
    }

    // This lane's chunk of row i of a factor matrix.
    __device__ __forceinline__ float4 q_row(const float* __restrict__ M, const int32_t i) const {
        return *reinterpret_cast<const float4*>(M + (size_t)i * KP + lig * 4);
    }

    // The candidates are taken in rounds of L: in the round that starts at candidate d0, lane `lig` of the group draws
    // d = d0 + lig (counter c0 + d), so the binary searches of a round run side by side (with weights, two a lane: one
    // over the mass table, one over the weights' prefix).  This lane's draw of a round of
    // `steps` candidates (1 .. L); 0 past them and for a group that is not `on` (a branch the whole group takes alike).
    __device__ __forceinline__ int32_t draw(const unsigned long long seed, const long long d0, const int steps, const bool on) const {
        int32_t mine = 0;
        if (on && lig < steps) mine = dr.draw(set, n_items, mass, seed, c0 + (unsigned long long)(d0 + lig));
        return mine;
    }

    // Candidates e0 .. e0 + D - 1 of a round: their ids are handed round the group (a lane permute, no LDS memory) and
    // each one's Q row is gathered by the whole group, D of them in flight; zeros in their place when not `load` (a branch
    // the whole group takes alike, around the load alone).  A step past the last candidate of the round repeats the
    // round's first candidate, which the caller drops by a select.  The permutes are never inside a branch, so their
    // partner lanes are live whatever the neighbouring groups of the wave are doing.
    template <int D>
    __device__ __forceinline__ void gather(const float* __restrict__ Q, const int32_t mine, const int e0, const int steps,
                                           const bool load, int32_t (&it)[D], float4 (&q)[D]) const {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int e = e0 + j < steps ? e0 + j : 0;
            it[j] = L == 1 ? mine : __shfl(mine, e, L);
            q[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (load) q[j] = q_row(Q, it[j]);
        }
    }
};

// The pick is the rule of include/mfsgd.h: the largest non-NaN score, equal scores to the
// smaller d, a NaN loses to every non-NaN, and d = 0 when every score is a NaN.  Candidates are examined in ascending
// d, and the running best (score, d, item) is the same in every lane of the group.
// m is the same for every row, so every lane of the launch runs the same trip counts (the DPP levels of
// group_allreduce need their partner lanes live).
template <int L, int D, class Draw>
__global__ void __launch_bounds__(256) hard_negative_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                            const long long* __restrict__ off,
                                                            const int32_t* __restrict__ items,
                                                            const int32_t* __restrict__ users, const long long n,
                                                            const int m, const int n_items, const unsigned long long seed,
                                                            const unsigned long long first, int32_t* __restrict__ out_items,
                                                            float* __restrict__ out_scores, int32_t* __restrict__ out_draw,
                                                            const Draw dr) {
    const PickRow<L, Draw> R(dr, P, off, items, users, n, m, n_items, first);
    float best_s = __builtin_bit_cast(float, kQuietNaN);
    int32_t best_d = -1, best_item = -1;
    for (long long d0 = 0; d0 < m; d0 += L) {
        const int steps = (long long)m - d0 < L ? (int)(m - d0) : L;  // candidates of this round: 1 .. L
        const int32_t mine = R.draw(seed, d0, steps, R.live);
        for (int e0 = 0; e0 < steps; e0 += D) {
            int32_t it[D];
            float4 q[D];
            R.template gather<D>(Q, mine, e0, steps, R.live, it, q);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float sc = group_allreduce<L>(chunk_dot(R.p, q[j]));
                const long long d = d0 + e0 + j;
                // ascending d: a later candidate takes over only with a larger score, or a number after nothing but NaNs
                const bool take = e0 + j < steps && (d == 0 || sc > best_s || (best_s != best_s && sc == sc));
                best_s = take ? sc : best_s;
                best_d = take ? (int32_t)d : best_d;
                best_item = take ? it[j] : best_item;
            }
        }
    }
    if (R.row && R.lig == 0) {
        const bool none = R.mass == 0;  // the user has nothing to draw from
        dr.report(R.x, R.mass);
        out_items[R.x] = none ? -1 : best_item;
        if (out_scores) out_scores[R.x] = none ? __builtin_bit_cast(float, kQuietNaN) : best_s;
        if (out_draw) out_draw[R.x] = none ? -1 : best_d;
    }
}

// Q[pos[x]] is loaded once and sp reduced once.  x[d] = sp - dot(P[u], Q[cand[d]]) is one fp32 subtraction, the bits
// pairwise.hip reports as the margin of (u, i, cand[d]); the pick is the rule of include/mfsgd.h: the smallest d with
// cand[d] != i and x[d] < margin.  Candidates are examined in ascending d, so the first violator seen is the pick;
// everything past it is skipped, and nothing of the result depends on what was skipped.
// `need` -- the row has candidates and no pick yet -- is the same in every lane of a group.  A group without it
// branches around its draws and its Q loads and computes on zeros, which a select drops: the DPP levels of
// group_allreduce, like the permutes of the gather, are never inside a branch.  The loops are left only when no group of
// the WAVE needs anything more: a ballot, so every lane of the wave leaves at the same trip, and a wave shares nothing
// with the other waves of its workgroup (no LDS, no barrier).
template <int L, int D, class Draw>
__global__ void __launch_bounds__(256) first_violating_kernel(
    const float* __restrict__ P, const float* __restrict__ Q, const long long* __restrict__ off, const int32_t* __restrict__ items,
    const int32_t* __restrict__ users, const int32_t* __restrict__ pos, const long long n, const int m, const float margin,
    const int n_items, const unsigned long long seed, const unsigned long long first, int32_t* __restrict__ out_items,
    int32_t* __restrict__ out_draw, float* __restrict__ out_margin, int32_t* __restrict__ out_rank, const Draw dr) {
    const PickRow<L, Draw> R(dr, P, off, items, users, n, m, n_items, first);
    const int ip = R.row ? pos[R.x] : 0;
    float4 qp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (R.live) qp = R.q_row(Q, ip);
    const float sp = group_allreduce<L>(chunk_dot(R.p, qp));

    float pick_x = __builtin_bit_cast(float, kQuietNaN);
    int32_t pick_d = -1, pick_item = -1;
    bool need = R.live;
    for (long long d0 = 0; d0 < m; d0 += L) {
        if (__builtin_amdgcn_ballot_w64(need) == 0) break;            // wave-uniform
        const int steps = (long long)m - d0 < L ? (int)(m - d0) : L;  // candidates of this round: 1 .. L
        const int32_t mine = R.draw(seed, d0, steps, need);
        for (int e0 = 0; e0 < steps; e0 += D) {
            if (__builtin_amdgcn_ballot_w64(need) == 0) break;  // wave-uniform; the round loop then ends at its own check
            const bool loaded = need;                           // what this group's q[] hold: rows of Q, or zeros
            int32_t it[D];
            float4 q[D];
            R.template gather<D>(Q, mine, e0, steps, loaded, it, q);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float xd = sp - group_allreduce<L>(chunk_dot(R.p, q[j]));
                // ascending d: the first violator is the pick; a NaN xd compares false
                const bool take = loaded && pick_d < 0 && e0 + j < steps && it[j] != ip && xd < margin;
                pick_x = take ? xd : pick_x;
                pick_item = take ? it[j] : pick_item;
                pick_d = take ? (int32_t)(d0 + e0 + j) : pick_d;
            }
            need = R.live && pick_d < 0;
        }
    }
    if (R.row && R.lig == 0) {
        const bool none = R.mass == 0;  // the user has nothing to draw from
        const bool hit = pick_d >= 0;
        dr.report(R.x, R.mass);
        out_items[R.x] = pick_item;
        if (out_draw) out_draw[R.x] = none ? -1 : hit ? pick_d : m;
        if (out_margin) out_margin[R.x] = pick_x;
        if (out_rank) {
            const long long rk = hit ? R.set.cnt / ((long long)pick_d + 1) : 0;  // (the unseen COUNT under either draw)
            out_rank[R.x] = hit ? (int32_t)(rk < 1 ? 1 : rk) : 0;
        }
    }
}

// One lane group per row of a piece (at most 2^22 rows): launch(l, grid, block) starts the instantiation for L = l().
template <class Launch>
hipError_t launch_pick(const int L, const int64_t n, const int32_t m, Launch&& launch) {
    if (n <= 0) return hipSuccess;
    if (m < 1) return hipErrorInvalidValue;
    const int gpb = 256 / L;
    const dim3 grid((unsigned)((n + gpb - 1) / gpb)), block(256);
    return with_L(L, [&](auto l) {
        launch(l, grid, block);
        return hipGetLastError();
    });
}

// The weighted policy of a launch: no weights (C == nullptr) is the uniform draw.
WeightedDraw weighted(const PickWeights& w) { return WeightedDraw{w.mass, w.C, w.out_mass}; }

}  // namespace

hipError_t launch_hard_negatives(int L, const float* P, const float* Q, const long long* off, const int32_t* items,
                                 const int32_t* users, int64_t n, int32_t m, int32_t n_items, int64_t seed, uint64_t first,
                                 int32_t* out_items, float* out_scores, int32_t* out_draw, hipStream_t st, const PickWeights& w) {
    return launch_pick(L, n, m, [&](auto l, const dim3 grid, const dim3 block) {
        auto go = [&](auto dr) {
            hipLaunchKernelGGL((hard_negative_kernel<l(), kPickDepth, decltype(dr)>), grid, block, 0, st, P, Q, off, items, users,
                               (long long)n, (int)m, (int)n_items, (unsigned long long)seed, (unsigned long long)first, out_items,
                               out_scores, out_draw, dr);
        };
        if (w.C) go(weighted(w));
        else go(UniformDraw{});
    });
}

hipError_t launch_first_violating(int L, const float* P, const float* Q, const long long* off, const int32_t* items,
                                  const int32_t* users, const int32_t* pos, int64_t n, int32_t m, float margin, int32_t n_items,
                                  int64_t seed, uint64_t first, int32_t* out_items, int32_t* out_draw, float* out_margin,
                                  int32_t* out_rank, hipStream_t st, const PickWeights& w) {
    return launch_pick(L, n, m, [&](auto l, const dim3 grid, const dim3 block) {
        auto go = [&](auto dr) {
            hipLaunchKernelGGL((first_violating_kernel<l(), kPickDepth, decltype(dr)>), grid, block, 0, st, P, Q, off, items, users,
                               pos, (long long)n, (int)m, margin, (int)n_items, (unsigned long long)seed, (unsigned long long)first,
                               out_items, out_draw, out_margin, out_rank, dr);
        };
        if (w.C) go(weighted(w));
        else go(UniformDraw{});
    });
}

}  // namespace mfsgd
