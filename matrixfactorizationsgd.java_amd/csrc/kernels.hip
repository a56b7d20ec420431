// kernels.hip -- the small gfx950 kernels around training: predict_kernel (dot products of given pairs),
// init_rows_kernel (device-side seeding of the factors) and the occupy_kernel diagnostic.  The training kernels are
// epoch.hip and cells.hip; kernels.hpp declares the launchers of all of them.
//
// Arithmetic is the contract of DESIGN.md section 3 and must stay bit-for-bit
// what the CPU checker under oracle/ computes: build with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "canon.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)


namespace mfsgd {

namespace {

// out[j] = dot(P[u[j]], Q[i[j]]); one lane group per pair.
template <int L>
__global__ void __launch_bounds__(256) predict_kernel(const float* __restrict__ P,
                                                      const float* __restrict__ Q,
                                                      const int32_t* __restrict__ u,
                                                      const int32_t* __restrict__ i,
                                                      float* __restrict__ out, const int64_t n) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;  // groups per block
    const int lig = threadIdx.x % L;
    const int64_t grp0 = (int64_t)blockIdx.x * GPB + threadIdx.x / L;
    const int64_t stride = (int64_t)gridDim.x * GPB;
    // all lanes of a wave run the same number of iterations (DPP needs them live)
    const int64_t iters = (n + stride - 1) / stride;
    for (int64_t it = 0; it < iters; ++it) {
        const int64_t j = grp0 + it * stride;
        const bool ok = j < n;
        const int64_t jj = ok ? j : 0;
        const float4 p = *reinterpret_cast<const float4*>(P + (size_t)u[jj] * KP + lig * 4);
        const float4 q = *reinterpret_cast<const float4*>(Q + (size_t)i[jj] * KP + lig * 4);
        const float d = group_allreduce<L>(chunk_dot(p, q));
        if (ok && lig == 0) out[j] = d;
    }
}
}  // namespace

// Factor initialisation on the device: java.util.Random(seed).nextFloat() * scale, row-major, the stream
// position of row x being first_pos + x * k -- the 48-bit LCG jumped to that position per row (the same
// doubling recurrence as JRandom::skip), then k sequential draws.  Integer work plus one exact division and
// one multiply per element: the bits csrc/jrandom.hpp and the oracle produce.
__global__ void __launch_bounds__(256) init_rows_kernel(float* __restrict__ dst, const long long rows, const int k,
                                                        const int kp, const unsigned long long s0,
                                                        const unsigned long long first_pos, const float scale) {
    constexpr unsigned long long kMult = 0x5DEECE66DULL, kAdd = 0xBULL, kMask = (1ULL << 48) - 1;
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < rows; row += (long long)gridDim.x * 256) {
        unsigned long long n = first_pos + (unsigned long long)row * (unsigned long long)k;
        unsigned long long acc_a = 1, acc_c = 0, cur_a = kMult, cur_c = kAdd;
        while (n) {
            if (n & 1) {
                acc_a = (acc_a * cur_a) & kMask;
                acc_c = (acc_c * cur_a + cur_c) & kMask;
            }
            cur_c = ((cur_a + 1) * cur_c) & kMask;
            cur_a = (cur_a * cur_a) & kMask;
            n >>= 1;
        }
        unsigned long long s = (acc_a * s0 + acc_c) & kMask;
        float* out = dst + (size_t)row * kp;
        for (int f = 0; f < k; ++f) {
            s = (s * kMult + kAdd) & kMask;
            const int v = (int)(unsigned)(s >> 24);  // next(24)
            out[f] = (float)v / 16777216.0f * scale;
        }
        for (int f = k; f < kp; ++f) out[f] = 0.0f;
    }
}

hipError_t launch_init_rows(float* dst, long long rows, int k, int kp, long long seed, unsigned long long first_pos, float scale,
                            hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    const unsigned long long s0 = ((unsigned long long)seed ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1);
    long long g = (rows + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(init_rows_kernel, dim3((unsigned)g), dim3(256), 0, st, dst, rows, k, kp, s0, first_pos, scale);
    return hipGetLastError();
}

// Diagnostic: workgroups that hold a whole CU's LDS and spin for `ticks` of the 100 MHz clock.
__global__ void __launch_bounds__(64) occupy_kernel(const unsigned long long ticks, unsigned* __restrict__ started) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    smem[threadIdx.x] = 0;
    if (started && threadIdx.x == 0) __hip_atomic_fetch_add(started, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

hipError_t launch_occupy(int workgroups, int lds_bytes, unsigned long long ticks, unsigned* started, hipStream_t st) {
    hipError_t e = hipFuncSetAttribute((const void*)occupy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(occupy_kernel, dim3((unsigned)workgroups), dim3(64), (size_t)lds_bytes, st, ticks, started);
    return hipGetLastError();
}

hipError_t launch_predict(int L, const float* P, const float* Q, const int32_t* u, const int32_t* i,
                          float* out, int64_t n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int gpb = 256 / L;
    int64_t blocks = (n + gpb - 1) / gpb;
    if (blocks > 4096) blocks = 4096;
    const dim3 grid((unsigned)blocks), block(256);
    return with_L(L, [&](auto l) {
        hipLaunchKernelGGL((predict_kernel<l()>), grid, block, 0, st, P, Q, u, i, out, n);
        return hipGetLastError();
    });
}

}  // namespace mfsgd
