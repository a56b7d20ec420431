// similar.hip -- cosine neighbours (mfsgd_similar_items / _users / _rows): the inverse norms of the rows of a factor
// matrix.  The scores themselves, (dot * rn(a)) * rn(b) of DESIGN.md section 3, are computed inside recommend.hip's
// selection kernels (their CosScore policy), so that selection, ties, exclusions and padding exist once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "canon.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {

namespace {

// out[x] = rn(M[x]): one lane group per row.  sqrt and division are the correctly rounded IEEE ones (no rsq, no
// fast-math: this unit is built like every kernel whose roundings are part of the contract).
template <int L>
__global__ void __launch_bounds__(256) inv_norm_kernel(const float* __restrict__ M, const long long n_rows,
                                                       float* __restrict__ out) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const long long stride = (long long)gridDim.x * GPB;
    const long long iters = (n_rows + stride - 1) / stride;  // uniform trip count: DPP needs every lane live
    for (long long it = 0; it < iters; ++it) {
        const long long x = (long long)blockIdx.x * GPB + grp + it * stride;
        const bool ok = x < n_rows;
        const float4 m = *reinterpret_cast<const float4*>(M + (size_t)(ok ? x : 0) * KP + lig * 4);
        const float n2 = group_allreduce<L>(chunk_dot(m, m));
        if (ok && lig == 0) out[x] = n2 > 0.0f ? 1.0f / __builtin_sqrtf(n2) : 0.0f;
    }
}

}  // namespace

hipError_t launch_row_inv_norms(int L, const float* M, int64_t n_rows, float* out, hipStream_t st) {
    if (n_rows <= 0) return hipSuccess;
    return with_L(L, [&](auto l) {
        constexpr int GPB = 256 / l();
        const long long blocks = std::min<long long>((n_rows + GPB - 1) / GPB, 8192);
        hipLaunchKernelGGL((inv_norm_kernel<l()>), dim3((unsigned)blocks), dim3(256), 0, st, M, (long long)n_rows, out);
        return hipGetLastError();
    });
}

}  // namespace mfsgd
