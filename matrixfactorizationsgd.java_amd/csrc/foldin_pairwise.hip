// foldin_pairwise.hip -- pairwise fold-in of new users (mfsgd_fold_in_users_pairwise; DESIGN.md, "Pairwise fold-in"): a BPR
// chain per new user over the user's positives alone, against the fixed Q, the chain drawing its own negatives.  The
// shape is foldin.hip's: one lane group of L lanes per new user keeps that user's row in registers for the whole chain,
// every lane runs the trip count of the longest chain in its wave, and a group whose chain has ended keeps its row by a
// select.  What a step adds to foldin.hip's: a negative, the pick among m unseen draws.
//
// The draw is draw.hpp's (mfsgd_sample_unseen's by construction), the score the canonical dot of canon.hpp, the pick the
// rule of pick.hip's hard negatives, the update the P line of pairwise.hip's step with canon.hpp's lsig: nothing is
// restated here but that rule's one line (through a shared function these kernels compile to other code).
// A draw is a function of its counter and the user's list S, never of the row, so the draws, their binary searches and
// the Q gathers of the positive and of the candidates run ahead of the chain; on the chain are the m scores, the pick,
// lsig and the update.  A draw is made by ONE lane of the group and handed round (a lane permute, no LDS memory): the L
// lanes of a group make L different draws side by side.
// Build with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "canon.hpp"
#include "dispatch.hpp"
#include "draw.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {
namespace {

// m == 1.  Steps the two Q gathers run ahead of the chain; the (positive, negative) ids run another kPairDepth ahead of
// the gathers (foldin.hip, kFoldDepth, is the idiom).  6, not kFoldDepth's 8: two rows a step are twice the registers, and
// at 8 the kernel has room for two waves a SIMD where it has room for three at 6 ("Pairwise fold-in": measured).
constexpr int kPairDepth = 6;
// The same with the weighted draw, which holds a second search's state per draw and the user's unseen weight: at 6 it
// needs 170 to 174 registers for L = 1, 4, 8, 16 (two waves a SIMD), at 5 it stays within the 168 of three.
constexpr int kPairDepthWeighted = 5;
// m > 1.  Candidates of one group whose Q rows are in flight together (pick.hip, kPickDepth); the next chunk is
// gathered while the chunk in hand is scored, across the end of a step too.
constexpr int kPairChunk = 4;

// What both kernels know of their group.  Group g of the launch folds in new user x = perm[g] of the batch: positives
// ptr[x] .. ptr[x + 1] of ids (ptr counts from the batch's first positive), the sorted distinct list
// s_items[s_off[x] .. s_off[x + 1]), row `rows + x * k` (dense; read once at the start, written once at the end).
// The draw is a policy (draw.hpp: UniformDraw, or WeightedDraw over the batch's own mass table for
// mfsgd_fold_in_users_pairwise_weighted): `mass` is what the user has to draw from, the number of unseen items or their
// weight, and a user whose mass is 0 takes no step.
template <int L, class Draw>
struct Group {
    static constexpr int GPB = 256 / L;  // groups per block
    const Draw& dr;
    int lig, x;
    bool live, draws;
    long long p0, len, at, steps, trip;
    Unseen set;  // of the batch's own lists; filled below by selects (Unseen's constructor branches: other code)
    unsigned long long mass;
    float4 row;

    __device__ __forceinline__ Group(const PairwiseFold& a, const Draw& draw_) : dr(draw_) {
        lig = threadIdx.x % L;
        const long long g = (long long)blockIdx.x * GPB + threadIdx.x / L;
        live = g < a.nb;
        x = live ? a.perm[g] : 0;
        p0 = live ? a.ptr[x] : 0;
        len = live ? a.ptr[x + 1] - p0 : 0;
        set.from = live ? a.s_off[x] : 0;
        set.s = live ? a.s_off[x + 1] - set.from : 0;
        set.list = a.s_items + set.from;
        set.cnt = (long long)a.n_items - set.s;
        mass = dr.mass(set, a.n_items);  // (a group that is not live has an empty list: nothing of it is read)
        draws = live && mass > 0;        // a group without draws gathers row 0 of Q in their place
        // a group without positives reads entry 0 of the batch (the launcher sends no batch without positives)
        at = len > 0 ? p0 : 0;
        steps = mass > 0 ? len * a.epochs : 0;  // the list names every item (of positive weight): no step is taken
        // trip count of the wave: the longest chain among its groups
        trip = steps;
        for (int w = L; w < 64; w <<= 1) {
            const long long o = __shfl_xor(trip, w);
            trip = o > trip ? o : trip;
        }
        trip = __builtin_amdgcn_readfirstlane((int)(trip >> 32)) * (1LL << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)trip);
        const float* src = a.rows + (size_t)x * a.k + lig * 4;
        const int f = lig * 4;
        row.x = live && f + 0 < a.k ? src[0] : 0.0f;
        row.y = live && f + 1 < a.k ? src[1] : 0.0f;
        row.z = live && f + 2 < a.k ? src[2] : 0.0f;
        row.w = live && f + 3 < a.k ? src[3] : 0.0f;
    }

    // The item of the user's draw number n (counter c0 + n); 0 for a group without draws.
    __device__ __forceinline__ int32_t draw(const PairwiseFold& a, const unsigned long long c0, const long long n) const {
        return dr.draw(set, a.n_items, mass, a.seed, c0 + (unsigned long long)n);
    }

    // One step of the chain on the row: the margin before it, the P line of the pairwise step, kept when `on`.
    __device__ __forceinline__ float step(const PairwiseFold& a, const float di, const float dj, const float4 qi, const float4 qj,
                                          const bool on) {
        const float xm = di - dj;
        const float sz = a.lr * lsig(xm);
        const float4 nw = axpy_row(sz, make_float4(qi.x - qj.x, qi.y - qj.y, qi.z - qj.z, qi.w - qj.w), a.c, row);
        row.x = on ? nw.x : row.x;
        row.y = on ? nw.y : row.y;
        row.z = on ? nw.z : row.z;
        row.w = on ? nw.w : row.w;
        return xm;
    }

    __device__ __forceinline__ void report(const PairwiseFold& a, const long long tau, const float xm, const int32_t j) const {
        if (lig != 0) return;
        if (a.out_margin) a.out_margin[p0 * a.epochs + tau] = xm;
        if (a.out_neg) a.out_neg[p0 * a.epochs + tau] = j;
    }

    __device__ __forceinline__ void finish(const PairwiseFold& a) const {
        if (!live) return;
        if (mass == 0)  // no step was taken: the user's margins and negatives say so
            for (long long e = lig; e < len * a.epochs; e += L) {
                if (a.out_margin) a.out_margin[p0 * a.epochs + e] = __builtin_bit_cast(float, kQuietNaN);
                if (a.out_neg) a.out_neg[p0 * a.epochs + e] = -1;
            }
        float* dst = a.rows + (size_t)x * a.k + lig * 4;
        const int f = lig * 4;
        if (f + 0 < a.k) dst[0] = row.x;
        if (f + 1 < a.k) dst[1] = row.y;
        if (f + 2 < a.k) dst[2] = row.z;
        if (f + 3 < a.k) dst[3] = row.w;
    }
};

// m == 1: the negative of step tau is the user's draw number tau.  Every D steps the group makes the D draws that the
// id stream takes up next, lane `lig` those of the steps e = lig, lig + L, ... < D of the block, so the binary searches
// of a block run side by side; the ids are handed round when their step's entry is fetched.
template <int L, int D, class Draw>
__global__ void __launch_bounds__(256) fold_in_pairwise_kernel(const PairwiseFold a, const Draw dr) {
    constexpr int KP = 4 * L;
    constexpr int DR = (D + L - 1) / L;  // draws of one lane per block of D steps
    Group<L, Draw> G(a, dr);
    if (G.trip > 0) {  // wave-uniform
        const unsigned long long c0 = a.first + (unsigned long long)(a.base + G.p0) * (unsigned long long)a.epochs;
        const long long wrap = G.len > 0 ? G.len : 1;
        long long ja = 0;  // position in the list of the next positive to fetch
        int32_t mine[DR];  // this lane's draws of the block whose entries are fetched next
        int32_t it[D], jt[D];  // positives and negatives of steps t + D .. t + 2D - 1
        float4 qi[D], qj[D];   // their Q rows for steps t .. t + D - 1
        int32_t jn[D];         // ... and the negatives' ids, for out_neg
        auto draw_block = [&](const long long n0) {
#pragma unroll
            for (int r = 0; r < DR; ++r) {
                const int e = r * L + G.lig;
                mine[r] = 0;
                if (G.draws && e < D) mine[r] = G.draw(a, c0, n0 + e);
            }
        };
        // The positives are read with relaxed atomic loads of wavefront scope, which the compiler leaves where they are
        // written (foldin.hip: with plain loads it moves every load of the pipeline next to its use).
        auto fetch_entry = [&](const int d) {
            it[d] = __hip_atomic_load(a.ids + G.at + ja, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            ja = ja + 1 == wrap ? 0 : ja + 1;
            jt[d] = L == 1 ? mine[d / L] : __shfl(mine[d / L], d % L, L);
        };
        auto fetch_rows = [&](const int d) {
            qi[d] = *reinterpret_cast<const float4*>(a.Q + (size_t)it[d] * KP + G.lig * 4);
            qj[d] = *reinterpret_cast<const float4*>(a.Q + (size_t)jt[d] * KP + G.lig * 4);
            jn[d] = jt[d];
        };
        draw_block(0);
#pragma unroll
        for (int d = 0; d < D; ++d) fetch_entry(d);
        draw_block(D);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            fetch_rows(d);
            fetch_entry(d);
        }
        for (long long t = 0; t < G.trip; t += D) {
            draw_block(t + 2 * D);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float4 qid = qi[d], qjd = qj[d];
                const int32_t j = jn[d];
                fetch_rows(d);   // step t + d + D
                fetch_entry(d);  // step t + d + 2D
                const float pi = chunk_dot(G.row, qid), pj = chunk_dot(G.row, qjd);
                const float di = group_allreduce<L>(pi), dj = group_allreduce<L>(pj);  // back to back
                const bool on = t + d < G.steps;
                const float xm = G.step(a, di, dj, qid, qjd, on);
                if (on) G.report(a, t + d, xm, j);
            }
        }
    }
    G.finish(a);
}

// m > 1: step tau scores the user's draws tau * m .. tau * m + m - 1, DC at a time.  The draws are one stream per user
// (the counters of consecutive steps are consecutive), made L at a time, lane `lig` making draw b * L + lig of batch b;
// two batches are held (w0: batch wb, w1: batch wb + 1), which is enough for a chunk of DC <= L consecutive draws.
// m is the same for every user, so every lane of the launch walks the same chunks.  A place past the step's last
// candidate repeats the chunk's first and is dropped by a select.
template <int L, int D, class Draw>
__global__ void __launch_bounds__(256) fold_in_pairwise_hard_kernel(const PairwiseFold a, const Draw dr) {
    constexpr int KP = 4 * L;
    constexpr int DC = D < L ? D : L;
    Group<L, Draw> G(a, dr);
    if (G.trip > 0) {  // wave-uniform
        const int m = a.m;
        const unsigned long long c0 =
            a.first + (unsigned long long)(a.base + G.p0) * (unsigned long long)a.epochs * (unsigned long long)m;
        const long long wrap = G.len > 0 ? G.len : 1;
        long long ja = 0;
        auto draw_batch = [&](const long long b) { return G.draws ? G.draw(a, c0, b * L + G.lig) : 0; };
        long long wb = 0;
        int32_t w0 = draw_batch(0), w1 = draw_batch(1);
        // the candidates e0 .. e0 + DC - 1 of step tau: their ids out of the window, their Q rows on the way
        auto gather = [&](const long long tau, const int e0, int32_t (&oi)[DC], float4 (&oq)[DC]) {
            const long long n0 = tau * m + e0;
            while (wb < n0 / L) {  // (the same in every lane of the launch)
                w0 = w1;
                w1 = draw_batch(wb + 2);
                ++wb;
            }
#pragma unroll
            for (int j = 0; j < DC; ++j) {
                const long long n = n0 + (e0 + j < m ? j : 0);
                const int32_t w = n / L > wb ? w1 : w0;
                oi[j] = L == 1 ? w : __shfl(w, (int)(n % L), L);
                oq[j] = *reinterpret_cast<const float4*>(a.Q + (size_t)oi[j] * KP + G.lig * 4);
            }
        };
        auto fetch_positive = [&]() {  // (relaxed atomic: it stays where it is written, as in the kernel above)
            const int32_t i = __hip_atomic_load(a.ids + G.at + ja, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            ja = ja + 1 == wrap ? 0 : ja + 1;
            return i;
        };
        auto q_row = [&](const int32_t i) { return *reinterpret_cast<const float4*>(a.Q + (size_t)i * KP + G.lig * 4); };
        int32_t ci[DC];
        float4 cq[DC];
        gather(0, 0, ci, cq);
        float4 qi_next = q_row(fetch_positive());  // the positive's row, a step ahead; its id, two
        int32_t i_next = fetch_positive();
        for (long long tau = 0; tau < G.trip; ++tau) {
            const float4 qi = qi_next;
            qi_next = q_row(i_next);
            i_next = fetch_positive();
            float best_s = 0.0f, di = 0.0f;
            int32_t best_j = 0;
            float4 best_q = cq[0];
            for (int e0 = 0; e0 < m; e0 += DC) {
                int32_t ni[DC];
                float4 nq[DC];
                const bool last = e0 + DC >= m;
                gather(last ? tau + 1 : tau, last ? 0 : e0 + DC, ni, nq);
                float part[DC], sc[DC];
#pragma unroll
                for (int j = 0; j < DC; ++j) part[j] = chunk_dot(G.row, cq[j]);
                const float pi = chunk_dot(G.row, qi);
#pragma unroll
                for (int j = 0; j < DC; ++j) sc[j] = group_allreduce<L>(part[j]);  // back to back, the positive's behind them
                if (e0 == 0) di = group_allreduce<L>(pi);
#pragma unroll
                for (int j = 0; j < DC; ++j) {
                    const int d = e0 + j;
                    // ascending d: a later candidate takes over only with a larger score, or a number after nothing but NaNs
                    const bool take = d < m && (d == 0 || sc[j] > best_s || (best_s != best_s && sc[j] == sc[j]));
                    best_s = take ? sc[j] : best_s;
                    best_j = take ? ci[j] : best_j;
                    best_q.x = take ? cq[j].x : best_q.x;
                    best_q.y = take ? cq[j].y : best_q.y;
                    best_q.z = take ? cq[j].z : best_q.z;
                    best_q.w = take ? cq[j].w : best_q.w;
                }
#pragma unroll
                for (int j = 0; j < DC; ++j) {
                    ci[j] = ni[j];
                    cq[j] = nq[j];
                }
            }
            const bool on = tau < G.steps;
            const float xm = G.step(a, di, best_s, qi, best_q, on);  // (the pick's score is its dot with the row as it is now)
            if (on) G.report(a, tau, xm, best_j);
        }
    }
    G.finish(a);
}

}  // namespace

hipError_t launch_fold_in_pairwise(int L, const PairwiseFold& a, hipStream_t st) {
    if (a.nb <= 0) return hipSuccess;
    if (a.m < 1) return hipErrorInvalidValue;
    const int gpb = 256 / L;
    const dim3 grid((unsigned)((a.nb + gpb - 1) / gpb)), block(256);
    return with_L(L, [&](auto l) {
        auto go = [&](auto dr) {
            constexpr int depth = std::is_same_v<decltype(dr), WeightedDraw> ? kPairDepthWeighted : kPairDepth;
            if (a.m == 1)
                hipLaunchKernelGGL((fold_in_pairwise_kernel<l(), depth, decltype(dr)>), grid, block, 0, st, a, dr);
            else
                hipLaunchKernelGGL((fold_in_pairwise_hard_kernel<l(), kPairChunk, decltype(dr)>), grid, block, 0, st, a, dr);
        };
        if (a.C) go(WeightedDraw{a.s_mass, a.C, nullptr});  // (the batch's own table: the lists are the batch's)
        else go(UniformDraw{});
        return hipGetLastError();
    });
}

}  // namespace mfsgd
