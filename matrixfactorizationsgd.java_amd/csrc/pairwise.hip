// pairwise.hip -- (user, positive item, negative item) triples applied to the live P and Q in the order given (DESIGN.md,
// "Pairwise ranking (BPR)"): the three-row update of section 3 per triple.  The host has cut the list into dependency
// levels (online_update.cpp, online_levels_of with its third index array): the triples of one level share no user row and
// no item row, in either item position, and every triple's predecessors on any of its three rows lie in a lower level,
// so the levels in ascending order, each in any order, give the bits of the sequential loop.  As in online.hip there is
// no block schedule and no LDS image: one lane group of L lanes per triple, rows read from and written to global memory.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "canon.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {
namespace {

// Levels l0 .. l1 - 1 of the piece: level l is the triples level_ptr[l] .. level_ptr[l + 1] - 1 of u / i / jn, and
// orig[t] is the place of triple t in the caller's list, where its margin goes (margin == nullptr: nobody asked).
// Launch shape, the barrier between the levels of a one-workgroup launch and the rule that every lane runs every pass
// are online.hip's (apply_levels_kernel), for the reasons it states.
// WEIGHTED: the step size of triple t is lr * w[t], a weight the caller gives (mfsgd_apply_triples_weighted), in place of
// lr * lsig(x); without it w is not read and the kernel is the one it was.
template <int L, bool WEIGHTED>
__global__ void __launch_bounds__(256) apply_triple_levels_kernel(float* P, float* Q, const int32_t* __restrict__ u,
                                                                  const int32_t* __restrict__ i, const int32_t* __restrict__ jn,
                                                                  const float* __restrict__ w, const int32_t* __restrict__ orig,
                                                                  const int32_t* __restrict__ level_ptr, const int l0, const int l1,
                                                                  const int k, const float lr, const float c,
                                                                  float* __restrict__ margin) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;  // groups per block
    const int lig = threadIdx.x % L;
    const int grp = threadIdx.x / L;
    const int stride = (int)gridDim.x * GPB;
    for (int l = l0; l < l1; ++l) {
        const int begin = level_ptr[l], end = level_ptr[l + 1];
        for (int base = begin + (int)blockIdx.x * GPB; base < end; base += stride) {  // workgroup-uniform
            const bool live = base + grp < end;
            const int t = live ? base + grp : base;
            float* prow = P + (size_t)u[t] * KP + lig * 4;
            float* irow = Q + (size_t)i[t] * KP + lig * 4;
            float* jrow = Q + (size_t)jn[t] * KP + lig * 4;
            const float4 p = *reinterpret_cast<const float4*>(prow);
            const float4 qi = *reinterpret_cast<const float4*>(irow);
            const float4 qj = *reinterpret_cast<const float4*>(jrow);
            // the two dots are independent: both reductions are in flight before either is used
            const float ci = chunk_dot(p, qi), cj = chunk_dot(p, qj);
            const float di = group_allreduce<L>(ci);
            const float dj = group_allreduce<L>(cj);
            const float x = di - dj;  // the margin before the update
            float s;
            if constexpr (WEIGHTED) s = lr * w[t];
            else s = lr * lsig(x);
            float4 d;
            d.x = qi.x - qj.x, d.y = qi.y - qj.y, d.z = qi.z - qj.z, d.w = qi.w - qj.w;
            float4 np = axpy_row(s, d, c, p);
            float4 ni = axpy_row(s, p, c, qi);
            float4 nj = axpy_row(-s, p, c, qj);
            // the pad columns (k .. KP - 1) stay +0.0, as in online.hip: fma(s, 0, c * 0) is NaN for a NaN s (a NaN margin,
            // or a NaN weight), and a NaN pad column would make every later dot of the row NaN
            const int pad_from = k - lig * 4;  // elements of this lane's chunk that are columns of the row
            if (pad_from < 4) {
                if (pad_from < 1) np.x = ni.x = nj.x = 0.0f;
                if (pad_from < 2) np.y = ni.y = nj.y = 0.0f;
                if (pad_from < 3) np.z = ni.z = nj.z = 0.0f;
                np.w = ni.w = nj.w = 0.0f;
            }
            if (live) {
                *reinterpret_cast<float4*>(prow) = np;
                *reinterpret_cast<float4*>(irow) = ni;
                *reinterpret_cast<float4*>(jrow) = nj;
                if (margin && lig == 0) margin[orig[t]] = x;
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

hipError_t launch_apply_triple_levels(int L, float* P, float* Q, const int32_t* u, const int32_t* i, const int32_t* jn,
                                      const float* w, const int32_t* orig, const int32_t* level_ptr, int l0, int l1,
                                      int workgroups, int k, float lr, float c, float* margin, hipStream_t st) {
    if (l1 <= l0) return hipSuccess;
    if (workgroups < 1 || (l1 - l0 > 1 && workgroups != 1)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)workgroups), block(256);
    return with_L(L, [&](auto l) {
        if (w)
            hipLaunchKernelGGL((apply_triple_levels_kernel<l(), true>), grid, block, 0, st, P, Q, u, i, jn, w, orig, level_ptr, l0,
                               l1, k, lr, c, margin);
        else
            hipLaunchKernelGGL((apply_triple_levels_kernel<l(), false>), grid, block, 0, st, P, Q, u, i, jn, w, orig, level_ptr,
                               l0, l1, k, lr, c, margin);
        return hipGetLastError();
    });
}

}  // namespace mfsgd
