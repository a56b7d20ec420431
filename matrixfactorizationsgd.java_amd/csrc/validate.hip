// validate.hip -- the sum of squared errors of arbitrary (user, item, rating) pairs under the current factors
// ("Held-out validation and early stopping"): what mfsgd_validation_rmse, mfsgd_rmse_pairs and
// mfsgd_train_early_stop measure.  No schedule and no LDS image: the pairs are streamed as they were given, one lane
// group of L lanes per pair as in predict_kernel, with the two row gathers of the next kPairsDepth pairs in flight
// while the current ones are reduced.
//
// The error of a pair is the fp32 number the oracle forms, r - dot(P[u], Q[i]) with the canonical dot of canon.hpp
// (the bits predict_kernel returns); the squares are summed in fp64.  The order of that sum is fixed by the pair list
// alone: pair j belongs to partial j mod kPairsSlots, every partial adds its pairs in ascending j, and the partials
// are folded by reduce_sse_kernel, whose order depends on nothing but their number.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "canon.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {
namespace {

// Pairs of one group whose rows are in flight while the previous kPairsDepth are reduced: 2 x kPairsDepth 16-byte
// loads per lane.  At 16 waves per CU (kPairsSlots groups of 16 lanes on 256 CUs) that is 128 KiB in flight per CU,
// beyond what a random-row gather needs to hide an HBM miss; the index triples run another kPairsDepth ahead of the
// rows, since a row address needs its index first.
// What the fixed slot count (kernels.hpp: it is part of the sum's order) costs elsewhere, none of it measured: at
// L = 1 and L = 2 (k <= 8) a launch is 256 or 512 waves, one or two per CU, far from what hides a miss; and a list
// shorter than the slot count gives every group one pair and three unrolled steps on pair 0, dropped by the select.
constexpr int kPairsDepth = 4;

// Group `slot` of the launch owns the pairs slot, slot + S, slot + 2 S, ... (S = kPairsSlots) and leaves their fp64 sum
// in partial[slot].  The launch covers the slots below min(n, S), rounded up to whole workgroups: a group whose slot
// is not below n computes on pair 0 and stores exactly 0.0.
// Every lane of a wave runs the trip count of the wave's first group, which has the most pairs (the DPP levels of
// group_allreduce need their partner lanes live); a step past a group's last pair is computed on pair 0 and dropped
// by a select, so nothing of pair 0 (a NaN, say) reaches a sum it does not belong to.
template <int L, int D>
__global__ void __launch_bounds__(256) pairs_sse_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                        const int32_t* __restrict__ u, const int32_t* __restrict__ i,
                                                        const float* __restrict__ r, const long long n,
                                                        double* __restrict__ partial) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;  // groups per block
    constexpr long long S = kPairsSlots;
    const int lig = threadIdx.x % L;
    const long long slot = (long long)blockIdx.x * GPB + threadIdx.x / L;
    const long long slot0 = (long long)blockIdx.x * GPB + (threadIdx.x & ~63) / L;  // first group of this wave
    long long trip = slot0 < n ? (n - slot0 + S - 1) / S : 0;
    trip = __builtin_amdgcn_readfirstlane((int)(trip >> 32)) * (1LL << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)trip);

    double acc = 0.0;
    if (trip > 0) {  // wave-uniform
        long long ja = slot;  // pair of the next index triple to fetch
        int iu[D], ii[D];     // triples of steps t + D .. t + 2D - 1
        float ir[D];
        float4 p[D], q[D];    // rows and ratings of steps t .. t + D - 1
        float rr[D];
        // The triples are read with relaxed atomic loads of wavefront scope: the same global_load instructions, but
        // the compiler leaves them where they are written (foldin.hip: with plain loads it moves each next to its use,
        // and every step then waits for an index and after that for its rows).
        auto fetch_triple = [&](int d) {
            const long long jj = ja < n ? ja : 0;
            iu[d] = __hip_atomic_load(u + jj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            ii[d] = __hip_atomic_load(i + jj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            ir[d] = __hip_atomic_load(r + jj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            ja += S;
        };
        auto fetch_rows = [&](int d) {
            p[d] = *reinterpret_cast<const float4*>(P + (size_t)iu[d] * KP + lig * 4);
            q[d] = *reinterpret_cast<const float4*>(Q + (size_t)ii[d] * KP + lig * 4);
            rr[d] = ir[d];
        };
#pragma unroll
        for (int d = 0; d < D; ++d) fetch_triple(d);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            fetch_rows(d);
            fetch_triple(d);
        }
        long long jc = slot;  // pair of the step being reduced
        for (long long t = 0; t < trip; t += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float4 pd = p[d], qd = q[d];
                const float rd = rr[d];
                fetch_rows(d);    // step t + d + D
                fetch_triple(d);  // step t + d + 2D
                const float e = rd - group_allreduce<L>(chunk_dot(pd, qd));
                const double sq = (double)e * (double)e;
                acc += jc < n ? sq : 0.0;
                jc += S;
            }
        }
    }
    if (lig == 0) partial[slot] = acc;
}

}  // namespace

int64_t pairs_sse_partials(int64_t n) { return n < kPairsSlots ? n : (int64_t)kPairsSlots; }

hipError_t launch_pairs_sse(int L, const float* P, const float* Q, const int32_t* u, const int32_t* i, const float* r,
                            int64_t n, double* partial, double* out, hipStream_t st) {
    if (n <= 0) return hipErrorInvalidValue;
    const int gpb = 256 / L;
    const int64_t slots = pairs_sse_partials(n);
    const dim3 grid((unsigned)((slots + gpb - 1) / gpb)), block(256);
    const hipError_t e = with_L(L, [&](auto l) {
        hipLaunchKernelGGL((pairs_sse_kernel<l(), kPairsDepth>), grid, block, 0, st, P, Q, u, i, r, (long long)n, partial);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    // (the groups behind slot n - 1 of the last workgroup stored 0.0: left out here, which changes no bit of the sum)
    return launch_reduce_sse(partial, slots, out, st);
}

}  // namespace mfsgd
