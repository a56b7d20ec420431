// online.hip -- fresh ratings applied to the live P and Q in the order given ("Online updates"): the whole
// canonical update of section 3, both halves, per rating.  The host has cut the list into dependency levels (online_update.cpp,
// online_levels_of): the ratings of one level share no user and no item, every rating's predecessors on either row lie
// in a lower level, so the levels in ascending order, each in any order, give the bits of the sequential loop.  No block
// schedule and no LDS image: one lane group of L lanes per rating, rows read from and written to global memory.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "canon.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {
namespace {

// Levels l0 .. l1 - 1 of the piece: level l is the ratings level_ptr[l] .. level_ptr[l + 1] - 1 of u / i / r, and
// orig[j] is the place of rating j in the caller's list, where its error goes (err == nullptr: nobody asked).
// The workgroups of the launch share a level's ratings, 256 / L per pass each, striding by the grid.  A launch of more
// than one level is a launch of ONE workgroup (the launcher sees to it): between two levels that workgroup makes its
// stores visible to its own waves, which is all it takes on one CU; nothing here lets one workgroup see what another
// stored within the launch.
// Every lane of a wave runs every pass its workgroup runs (the DPP levels of group_allreduce need their partner lanes
// live): a group behind the level's last rating computes on the first rating of its workgroup's pass and stores nothing.
template <int L>
__global__ void __launch_bounds__(256) apply_levels_kernel(float* P, float* Q, const int32_t* __restrict__ u,
                                                           const int32_t* __restrict__ i, const float* __restrict__ r,
                                                           const int32_t* __restrict__ orig,
                                                           const int32_t* __restrict__ level_ptr, const int l0, const int l1,
                                                           const int k, const float lr, const float c, float* __restrict__ err) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;  // groups per block
    const int lig = threadIdx.x % L;
    const int grp = threadIdx.x / L;
    const int stride = (int)gridDim.x * GPB;
    for (int l = l0; l < l1; ++l) {
        const int begin = level_ptr[l], end = level_ptr[l + 1];
        for (int base = begin + (int)blockIdx.x * GPB; base < end; base += stride) {  // workgroup-uniform
            const bool live = base + grp < end;
            const int j = live ? base + grp : base;
            float* prow = P + (size_t)u[j] * KP + lig * 4;
            float* qrow = Q + (size_t)i[j] * KP + lig * 4;
            const float rj = r[j];
            const float4 p = *reinterpret_cast<const float4*>(prow);
            const float4 q = *reinterpret_cast<const float4*>(qrow);
            const float dot = group_allreduce<L>(chunk_dot(p, q));
            const float e = rj - dot;
            const float s = __builtin_fmaf(-lr, dot, lr * rj);
            float4 np = axpy_row(s, q, c, p);
            float4 nq = axpy_row(s, p, c, q);
            // the pad columns (k .. KP - 1) stay +0.0: fma(s, 0, c * 0) is +0.0 for every finite s, but NaN for an infinite
            // one (an overflowing rating), and a NaN pad column would make every later dot of the row NaN where the k
            // columns of the definition are infinite at most
            const int pad_from = k - lig * 4;  // elements of this lane's chunk that are columns of the row
            if (pad_from < 4) {
                if (pad_from < 1) np.x = nq.x = 0.0f;
                if (pad_from < 2) np.y = nq.y = 0.0f;
                if (pad_from < 3) np.z = nq.z = 0.0f;
                np.w = nq.w = 0.0f;
            }
            if (live) {
                *reinterpret_cast<float4*>(prow) = np;
                *reinterpret_cast<float4*>(qrow) = nq;
                if (err && lig == 0) err[orig[j]] = e;
            }
        }
        if (l + 1 < l1) {  // uniform over the launch
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
}

}  // namespace

hipError_t launch_apply_levels(int L, float* P, float* Q, const int32_t* u, const int32_t* i, const float* r,
                               const int32_t* orig, const int32_t* level_ptr, int l0, int l1, int workgroups, int k,
                               float lr, float c, float* err, hipStream_t st) {
    if (l1 <= l0) return hipSuccess;
    if (workgroups < 1 || (l1 - l0 > 1 && workgroups != 1)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)workgroups), block(256);
    return with_L(L, [&](auto l) {
        hipLaunchKernelGGL((apply_levels_kernel<l()>), grid, block, 0, st, P, Q, u, i, r, orig, level_ptr, l0, l1, k, lr, c, err);
        return hipGetLastError();
    });
}

}  // namespace mfsgd
