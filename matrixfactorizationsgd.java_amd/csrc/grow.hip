// grow.hip -- rows of the caller's into the live factors ("Growing a live model"): place_rows_kernel pads
// dense rows to the device stride and writes them where the model keeps its rows, so that an append never brings the
// old rows to the host.  No arithmetic: a NaN is made the library's quiet NaN (records.hpp), everything else is copied.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"
#include "records.hpp"

namespace mfsgd {
namespace {

// One thread per 16 bytes of dst: granule g is columns 4c .. 4c + 3 of row x, c = g % (kp / 4).  A row of kp floats
// starts on a 16-byte boundary, so every store is one float4.  The dense source does so only where k is a multiple of
// 4 (VEC): otherwise it is read float by float, and the columns from k on are zeros.
template <bool VEC>
__global__ void __launch_bounds__(256) place_rows_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                         const long long granules, const int k, const int kp) {
    const int gpr = kp / 4;  // granules per row
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < granules; g += (long long)gridDim.x * 256) {
        const long long x = g / gpr;
        const int f = (int)(g - x * gpr) * 4;
        const float* s = src + x * (long long)k + f;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (VEC) {
            if (f < k) v = *reinterpret_cast<const float4*>(s);
        } else {
            if (f + 0 < k) v.x = s[0];
            if (f + 1 < k) v.y = s[1];
            if (f + 2 < k) v.z = s[2];
            if (f + 3 < k) v.w = s[3];
        }
        v.x = canon_nan(v.x);
        v.y = canon_nan(v.y);
        v.z = canon_nan(v.z);
        v.w = canon_nan(v.w);
        *reinterpret_cast<float4*>(dst + g * 4) = v;
    }
}

}  // namespace

hipError_t launch_place_rows(float* dst, const float* src, long long rows, int k, int kp, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    if (k < 1 || kp < k || kp % 4 != 0 || ((uintptr_t)dst & 15) != 0) return hipErrorInvalidValue;
    const long long granules = rows * (long long)(kp / 4);
    long long g = (granules + 255) / 256;
    if (g > 4096) g = 4096;
    if (k % 4 == 0 && ((uintptr_t)src & 15) == 0)
        hipLaunchKernelGGL(place_rows_kernel<true>, dim3((unsigned)g), dim3(256), 0, st, dst, src, granules, k, kp);
    else
        hipLaunchKernelGGL(place_rows_kernel<false>, dim3((unsigned)g), dim3(256), 0, st, dst, src, granules, k, kp);
    return hipGetLastError();
}

}  // namespace mfsgd
