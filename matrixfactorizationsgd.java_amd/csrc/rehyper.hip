// rehyper.hip -- other hyper-parameters for a schedule that is already on the device ("Changing lr and
// lambda"): the pass of schedule.cpp's rehyper_schedule over entries the host may never have held (a device-packed
// schedule's exist here only).  lr and lambda sit in two words of every step entry (lr * r and the decay factor) and in
// one word of every solo record (lr * r); nothing else of a schedule depends on them.
//
// A pure streaming pass: each record is read once as one 16-byte vector (a wave covers 1 KiB of consecutive entries per
// instruction; word 2 is never used, so hipcc fetches words 0..1 with one dwordx2 and word 3 only for solo records --
// the same cache lines) and gets its words 2..3 (step entries, one 8-byte store) or its word 2 (solo records) back.  What a
// record IS follows from the chunk descriptor and the chunk's sub-cell table, never from the old values (with
// lambda == 0 the old decay factor is exactly 1.0f, like an idle run slot's).
//
// Decomposition: one wave per chunk descriptor, lane y taking entry y, y + 64, ... of the chunk -- flat over the chunk,
// not sub-cell by sub-cell (a MovieLens sub-cell is ~15 entries: a loop per sub-cell would idle three lanes in four).
// The W*W <= 64 sub-cell records stay in registers, lane x holding record x; an entry finds its sub-cell with a
// binary search over the sub-cells' first steps, read from the other lanes (they are non-decreasing in x: the packers
// lay the sub-cells out in table order).  No LDS, no barrier, no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {
namespace {

constexpr int kWavesPerBlock = 4;

__global__ void __launch_bounds__(64 * kWavesPerBlock) rehyper_kernel(const CellDesc* __restrict__ cells,
                                                                       const SubDesc* __restrict__ subs,
                                                                       Entry* __restrict__ entries, const long long n_descs,
                                                                       const long long n_entries, const int WW, const int lgG,
                                                                       const float lr, const float c) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long stride = (long long)gridDim.x * kWavesPerBlock;
    const uint4* ent4 = reinterpret_cast<const uint4*>(entries);
    for (long long d = wave0; d < n_descs; d += stride) {
        const CellDesc cd = cells[d];
        const unsigned n_steps = cd.n_steps & ~kCellCritical;
        if (n_steps == 0) continue;  // (an empty cell; uniform over the wave)
        // lane x < WW: sub-cell x of this chunk.  The other lanes hold a first step no entry reaches.
        SubDesc sd{0xFFFFu, 0u};
        if (lane < WW) sd = subs[d * WW + lane];
        const unsigned first = lane < WW ? (sd.off & 0xFFFFu) : 0xFFFFFFFFu;
        const long long base = (long long)cd.ent_off << lgG;
        const unsigned total = n_steps << lgG;          // entries of the chunk (n_steps <= 0x10001 steps of <= 64)
        const unsigned trailing = (n_steps - 2) << lgG;  // its two trailing idle steps start here
        for (unsigned y0 = 0; y0 < total; y0 += 64) {    // (uniform trip count: every lane takes part in the shuffles)
            const unsigned y = y0 + (unsigned)lane;
            const bool live = y < total && base + (long long)y < n_entries;
            const unsigned step = y >> lgG;
            // the last sub-cell whose first step is <= step (an empty sub-cell shares its first step with the next one)
            int x = 0;
            for (int h = WW >> 1; h >= 1; h >>= 1) {
                const unsigned f = (unsigned)__shfl((int)first, x + h);
                if (f <= step) x += h;
            }
            const unsigned off = (unsigned)__shfl((int)sd.off, x), n = (unsigned)__shfl((int)sd.n, x);
            if (!live) continue;
            const unsigned nsolo = off >> 16, ns = n & 0xFFFFu, nr = n >> 16;
            const unsigned rel = y - ((off & 0xFFFFu) << lgG);    // entry within the sub-cell
            const unsigned run_lo = ns << lgG, run_hi = (ns + nr) << lgG;
            const unsigned rec_lo = run_hi + ((unsigned)kSoloPad << lgG);  // the solo header (only when nsolo > 0)
            const uint4 e = ent4[base + y];  // {slots, r, lr * r, ce} or a solo record {slots, mailbox, lr * r, r}
            float* w = reinterpret_cast<float*>(entries + base + y);
            if (y >= trailing || rel < run_hi || (nsolo > 0 && rel < rec_lo)) {
                // a step entry; in a run step bit 31 of the slot word marks an idle slot, whose row must not decay
                const bool idle_run = y < trailing && rel >= run_lo && rel < run_hi && (e.x >> 31) != 0;
                float2 v;
                v.x = canon_nan(lr * __uint_as_float(e.y));
                v.y = idle_run ? 1.0f : c;
                *reinterpret_cast<float2*>(w + 2) = v;
            } else if (nsolo > 0 && rel > rec_lo && rel <= rec_lo + nsolo) {
                w[2] = canon_nan(lr * __uint_as_float(e.w));  // record t = rel - rec_lo - 1; the header and the tail hold no rating
            }
        }
    }
}

}  // namespace

hipError_t launch_rehyper(const CellDesc* cells, const SubDesc* subs, Entry* entries, int64_t n_descs, int64_t n_entries,
                          int W, int G, float lr, float c, hipStream_t st) {
    if (n_descs <= 0 || n_entries <= 0) return hipSuccess;
    int lgG = 0;
    while ((1 << lgG) < G) ++lgG;
    // (the kernel's search over a chunk's sub-cells halves W*W: a power of two, and no more than one record per lane)
    if ((1 << lgG) != G || W < 1 || W * W > 64 || (W & (W - 1)) != 0) return hipErrorInvalidValue;
    // memory bound: enough waves to fill the chip eight deep, the rest of the descriptors by stride
    const int64_t blocks = std::min<int64_t>((n_descs + kWavesPerBlock - 1) / kWavesPerBlock, 256 * 8);
    hipLaunchKernelGGL(rehyper_kernel, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, st, cells, subs, entries,
                       (long long)n_descs, (long long)n_entries, W * W, lgG, lr, c);
    return hipGetLastError();
}

}  // namespace mfsgd
