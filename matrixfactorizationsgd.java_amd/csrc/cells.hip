// cells.hip -- the kernels that run a schedule's cells one launch at a time: cell_kernel (one training round per
// launch -- what a DSGD sub-epoch and the not-resident fall-back run -- its diagnostic form with cycle stamps, and
// the one-cell-per-workgroup RMSE reference) and the persistent RMSE pass, sse_kernel + reduce_sse_kernel.  The
// persistent training kernel is epoch.hip; what a workgroup does with a cell is cell.hpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cell.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {

namespace {

// Deterministic sum of squared errors of one workgroup -> sse_partial[blockIdx.x].  Every lane of a group carries
// the group's sum: keep one copy, then a fixed butterfly over the wave, then waves in index order.
template <class CellT>
__device__ __forceinline__ void store_block_sse(const CellT& cx, const double acc, unsigned char* smem,
                                                double* __restrict__ sse_partial) {
    double v = cx.lig == 0 ? acc : 0.0;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();  // everyone is done reading the schedule buffer before it is reused
    double* wsum = reinterpret_cast<double*>(smem + 16);
    if (cx.lane == 0) wsum[cx.wave_all] = v;
    __syncthreads();
    if (cx.tid == 0) {
        double t = 0.0;
        for (int w = 0; w < CellT::NWV; ++w) t += wsum[w];
        sse_partial[blockIdx.x] = t;
    }
}

// One workgroup = one cell, one launch = one round.  TRAIN: round `rd` runs cells
// (b, (b + rd) % B), each workgroup walking the chunks of its cell.  !TRAIN: blockIdx.x
// is a chunk descriptor index (every chunk on its own), no writes, SSE out.
template <int L, int W, bool TRAIN, bool DIAG = false>
__global__ void __launch_bounds__(64 * W)
cell_kernel(float* __restrict__ P, float* __restrict__ Q, const CellDesc* __restrict__ cells,
            const uint32_t* __restrict__ rows, const SubDesc* __restrict__ subs,
            const Entry* __restrict__ entries, const int B, const int rd, const float lr,
            const float c, double* __restrict__ sse_partial, const int sched_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Cell<L, W> cx;
    cx.init_thread();
    int cell = TRAIN ? (int)blockIdx.x * B + ((int)blockIdx.x + rd) % B : (int)blockIdx.x;
    unsigned long long stamp0 = 0, stamp1 = 0, stamp2 = 0, real0 = 0;
    if constexpr (DIAG) {
        stamp0 = __builtin_amdgcn_s_memtime();
        real0 = __builtin_amdgcn_s_memrealtime();
    }
    double acc = 0.0;
    for (;;) {
        const CellDesc cd = load_desc(cells, (unsigned)cell);
        cx.bind(cd, smem, 0, sched_cap);
        if (cx.nrows == 0) break;  // uniform over the workgroup; an empty cell has no further chunk
        cx.stage_schedule(cd, cell, rows, subs, entries);
        __syncthreads();
        cx.gather(P, Q, 0, cx.nrows);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (DIAG) stamp1 = __builtin_amdgcn_s_memtime();
        if constexpr (DIAG)
            cx.template apply<TRAIN, true>(lr, c, acc, reinterpret_cast<unsigned long long*>(sse_partial) +
                                                           (size_t)gridDim.x * 6 + (size_t)blockIdx.x * W * W * 4);
        else
            cx.template apply<TRAIN>(lr, c, acc);
        if constexpr (DIAG) stamp2 = __builtin_amdgcn_s_memtime();
        if constexpr (!TRAIN) break;
        cx.template scatter<false>(P, Q, 0, cx.nrows);
        if (cd.next == 0) break;
        // next chunk of this cell: its gathers may read rows stored just now, and it reuses the LDS image
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cell = (int)cd.next;
    }
    if constexpr (TRAIN) {
        if constexpr (DIAG) {
            // diagnostic build only: phase stamps of this workgroup (of the last chunk it ran)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned long long stamp3 = __builtin_amdgcn_s_memtime();
            const unsigned long long real3 = __builtin_amdgcn_s_memrealtime();
            if (cx.tid == 0) {
                unsigned long long* o = reinterpret_cast<unsigned long long*>(sse_partial) + (size_t)blockIdx.x * 6;
                o[0] = stamp0;
                o[1] = stamp1;
                o[2] = stamp2;
                o[3] = stamp3;
                o[4] = real0;  // 100 MHz constant clock, common to all XCDs
                o[5] = real3;
            }
        }
    } else {
        store_block_sse(cx, acc, smem, sse_partial);
    }
}

// Sum of squared errors, persistent form: gridDim.x workgroups walk the B*B cells with a stride,
// the next cell's schedule prefetched (LDS-DMA) while the current one is applied; no writes.
// One fp64 partial per workgroup (fixed order inside it), reduced by reduce_sse_kernel.
template <int L, int W>
__global__ void __launch_bounds__(64 * (W + epoch_helpers<L, W>()))
sse_kernel(const float* __restrict__ P, const float* __restrict__ Q, const CellDesc* __restrict__ cells,
           const uint32_t* __restrict__ rows, const SubDesc* __restrict__ subs, const Entry* __restrict__ entries,
           const int n_cells, double* __restrict__ sse_partial, const int sched_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Cell<L, W, epoch_helpers<L, W>()> cx;
    cx.init_thread();
    const int stride = (int)gridDim.x;
    int c = (int)blockIdx.x;
    double acc = 0.0;
    if (c < n_cells) {
        CellDesc cd = load_desc(cells, (unsigned)c);
        CellDesc cd1 = c + stride < n_cells ? load_desc(cells, (unsigned)(c + stride)) : cd;
        int buf = 0;
        cx.bind(cd, smem, buf, sched_cap);
        cx.stage_schedule(cd, c, rows, subs, entries);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wg_barrier();
        for (; c < n_cells; c += stride) {
            const int c1 = c + stride, c2 = c + 2 * stride;
            cx.bind(cd, smem, buf, sched_cap);
            cx.zero_idle_rows();
            if (c1 < n_cells) cx.prefetch_schedule(cd1, c1, smem, buf ^ 1, sched_cap, rows, subs, entries);
            if (cx.nrows != 0) cx.gather(P, Q, 0, cx.nrows);
            CellDesc cd2 = cd1;
            if (c2 < n_cells) cd2 = load_desc(cells, (unsigned)c2);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // rows and the next schedule have landed
            wg_barrier();
            if (cx.nrows != 0) cx.template apply<false>(0.f, 0.f, acc);
            wg_barrier();  // every wave is done with the rows image and this schedule buffer
            buf ^= 1;
            cd = cd1;
            cd1 = cd2;
        }
    }
    store_block_sse(cx, acc, smem, sse_partial);
}

// Fixed-order reduction of the per-cell partial sums (one workgroup).
__global__ void __launch_bounds__(256) reduce_sse_kernel(const double* __restrict__ partial,
                                                         const int64_t n, double* __restrict__ out) {
    __shared__ double sh[256];
    double t = 0.0;
    for (int64_t x = threadIdx.x; x < n; x += 256) t += partial[x];
    sh[threadIdx.x] = t;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

template <int L, int W>
hipError_t launch_cell_LW(bool train, const CellLaunch& a, hipStream_t st) {
    const void* fn = train ? (const void*)cell_kernel<L, W, true> : (const void*)cell_kernel<L, W, false>;
    // > 64 KiB of dynamic LDS has to be granted per function; cheap to repeat.
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)a.grid), block(64 * W);
    if (train && a.diag) {
        const void* fd = (const void*)cell_kernel<L, W, true, true>;
        e = hipFuncSetAttribute(fd, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((cell_kernel<L, W, true, true>), grid, block, (size_t)a.lds_bytes, st, a.P, a.Q,
                           a.cells, a.rows, a.subs, a.entries, a.B, a.rd, a.lr, a.c, a.sse_partial, a.sched_cap);
    } else if (train)
        hipLaunchKernelGGL((cell_kernel<L, W, true>), grid, block, (size_t)a.lds_bytes, st, a.P, a.Q,
                           a.cells, a.rows, a.subs, a.entries, a.B, a.rd, a.lr, a.c, a.sse_partial, a.sched_cap);
    else
        hipLaunchKernelGGL((cell_kernel<L, W, false>), grid, block, (size_t)a.lds_bytes, st, a.P, a.Q,
                           a.cells, a.rows, a.subs, a.entries, a.B, a.rd, a.lr, a.c, a.sse_partial, a.sched_cap);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_cell(bool train, int L, int W, const CellLaunch& a, hipStream_t st) {
    return with_L(L, [&](auto l) { return with_W(W, [&](auto w) { return launch_cell_LW<l(), w()>(train, a, st); }); });
}

template <int L, int W>
hipError_t sse_LW(const CellLaunch& a, int n_cells, hipStream_t st) {
    const void* fn = (const void*)sse_kernel<L, W>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((sse_kernel<L, W>), dim3((unsigned)a.grid), dim3(64 * (W + epoch_helpers<L, W>())),
                       (size_t)a.lds_bytes, st, a.P, a.Q, a.cells, a.rows, a.subs, a.entries, n_cells, a.sse_partial,
                       a.sched_cap);
    return hipGetLastError();
}

hipError_t launch_sse_persistent(int L, int W, const CellLaunch& a, int n_cells, hipStream_t st) {
    return with_L(L, [&](auto l) { return with_W(W, [&](auto w) { return sse_LW<l(), w()>(a, n_cells, st); }); });
}

hipError_t launch_reduce_sse(const double* partial, int64_t n, double* out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_sse_kernel, dim3(1), dim3(256), 0, st, partial, n, out);
    return hipGetLastError();
}

}  // namespace mfsgd
