// foldin.hip -- fold-in of new rows against the fixed factors of the other side ("Fold-in"): one half of
// the canonical update of section 3, run over each new row's ratings alone.  New users are folded in against Q, new
// items against P: the update is symmetric in its two rows and both matrices have the stride kp, so the kernel reads
// "the fixed side" F and never asks which it is.  F is only read, new rows are independent of each other, so there is
// no block schedule and no LDS image: one lane group of L lanes per new row keeps that row in registers for the whole
// chain, fed by a gather of F rows that runs kFoldDepth steps ahead of the arithmetic.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "canon.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {
namespace {

// Steps the F gather runs ahead of the chain; the (id, rating) stream runs another kFoldDepth ahead of the gather,
// since an F address needs its id first.
constexpr int kFoldDepth = 8;

// Group g of the launch folds in new row perm[g] of the batch: ratings row_ptr[x] - base .. row_ptr[x + 1] - base of
// ids / ratings, row `rows + x * k` (dense; read once at the start, written once at the end).
// The chain of a group is its list repeated `epochs` times: len * epochs steps, the position in the list wrapping
// round.  Every lane runs the trip count of the longest chain in its wave (the DPP levels of group_allreduce need
// their partner lanes live); a group whose chain has ended keeps loading, from its own list, and keeps its row by a
// select.
template <int L, int D>
__global__ void __launch_bounds__(256) fold_in_kernel(const float* __restrict__ F, float* __restrict__ rows, const int k,
                                                      const long long* __restrict__ row_ptr, const long long base,
                                                      const int32_t* __restrict__ perm, const int nb,
                                                      const int32_t* __restrict__ ids,
                                                      const float* __restrict__ ratings, const int epochs,
                                                      const float lr, const float c) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;  // groups per block
    const int lig = threadIdx.x % L;
    const long long g = (long long)blockIdx.x * GPB + threadIdx.x / L;
    const bool live = g < nb;
    const int x = live ? perm[g] : 0;
    const long long len = live ? row_ptr[x + 1] - row_ptr[x] : 0;
    // a group without ratings reads entry 0 of the batch (the launcher sends no batch without ratings)
    const long long first = len > 0 ? row_ptr[x] - base : 0;
    const long long steps = len * epochs;
    // trip count of the wave: the longest chain among its groups
    long long trip = steps;
    for (int m = L; m < 64; m <<= 1) {
        const long long o = __shfl_xor(trip, m);
        trip = o > trip ? o : trip;
    }
    trip = __builtin_amdgcn_readfirstlane((int)(trip >> 32)) * (1LL << 32) |
           (unsigned)__builtin_amdgcn_readfirstlane((int)trip);

    float4 row;
    {
        const float* src = rows + (size_t)x * k + lig * 4;
        const int f = lig * 4;
        row.x = live && f + 0 < k ? src[0] : 0.0f;
        row.y = live && f + 1 < k ? src[1] : 0.0f;
        row.z = live && f + 2 < k ? src[2] : 0.0f;
        row.w = live && f + 3 < k ? src[3] : 0.0f;
    }
    if (trip > 0) {  // wave-uniform
        const long long wrap = len > 0 ? len : 1;
        long long ja = 0;  // position in the list of the next entry to fetch
        int it[D];         // entries of steps t + D .. t + 2D - 1
        float rr[D];
        float4 q[D];       // F rows and lr * rating of steps t .. t + D - 1
        float sr[D];
        // The entry stream is read with relaxed atomic loads of wavefront scope: the same global_load instructions, but
        // the compiler leaves them where they are written.  With plain loads it moves every load of the pipeline next to
        // its use (it carries the positions round the loop instead of the loaded values), and each step then waits for
        // an id and after that for its F row.
        auto fetch_entry = [&](int d) {
            it[d] = __hip_atomic_load(ids + first + ja, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            rr[d] = __hip_atomic_load(ratings + first + ja, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            ja = ja + 1 == wrap ? 0 : ja + 1;
        };
        auto fetch_row = [&](int d) {
            q[d] = *reinterpret_cast<const float4*>(F + (size_t)it[d] * KP + lig * 4);
            sr[d] = lr * rr[d];
        };
#pragma unroll
        for (int d = 0; d < D; ++d) fetch_entry(d);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            fetch_row(d);
            fetch_entry(d);
        }
        for (long long t = 0; t < trip; t += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float4 qd = q[d];
                const float srd = sr[d];
                fetch_row(d);    // step t + d + D
                fetch_entry(d);  // step t + d + 2D
                const float dot = group_allreduce<L>(chunk_dot(row, qd));
                const float s = __builtin_fmaf(-lr, dot, srd);
                const float4 nw = axpy_row(s, qd, c, row);
                const bool on = t + d < steps;
                row.x = on ? nw.x : row.x;
                row.y = on ? nw.y : row.y;
                row.z = on ? nw.z : row.z;
                row.w = on ? nw.w : row.w;
            }
        }
    }
    if (live) {
        float* dst = rows + (size_t)x * k + lig * 4;
        const int f = lig * 4;
        if (f + 0 < k) dst[0] = row.x;
        if (f + 1 < k) dst[1] = row.y;
        if (f + 2 < k) dst[2] = row.z;
        if (f + 3 < k) dst[3] = row.w;
    }
}

}  // namespace

hipError_t launch_fold_in(int L, const float* F, float* rows, int k, const long long* row_ptr, long long base,
                          const int32_t* perm, int nb, const int32_t* ids, const float* ratings, int epochs, float lr,
                          float c, hipStream_t st) {
    if (nb <= 0) return hipSuccess;
    const int gpb = 256 / L;
    const dim3 grid((unsigned)((nb + gpb - 1) / gpb)), block(256);
    return with_L(L, [&](auto l) {
        hipLaunchKernelGGL((fold_in_kernel<l(), kFoldDepth>), grid, block, 0, st, F, rows, k, row_ptr, base, perm, nb, ids,
                           ratings, epochs, lr, c);
        return hipGetLastError();
    });
}

}  // namespace mfsgd
