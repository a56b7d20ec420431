// recommend.hip -- top-N scoring: for each requested user the N items with
// the largest dot(P[u], Q[i]), ties broken by the smaller item index.  Scores use the canonical
// dot of DESIGN.md section 3, so they are bit-identical to mfsgd_predict() and to the oracle.
// Score pass: one lane group per (user, item) pair, the user's row held in registers across
// items.  Selection, for topn <= kTopnFused: fused behind the scores in ONE kernel -- a workgroup per
// user keeps the scores of a tile of items in LDS as order-preserving integers, finds the topn-th
// largest by a 4 x 8-bit radix select on LDS histograms, collects what lies above it (ties in
// ascending item order) and sorts only those; no score ever goes to memory.  Larger topn: scores to
// memory and one stable, descending segmented radix sort per batch of users (rocPRIM).
// Exclusions (mfsgd_recommend_excluding): one sorted, distinct item list per requested user, built here from
// the caller's (user, item) pairs; both paths have a variant that gives excluded items a key below every
// eligible one (0: eligible keys are clamped to >= 1) and pads a row that runs out of eligible items.
// What is scored is a compile-time policy of the kernels: the dot (recommend), or the cosine built on it with the rows'
// inverse norms (the similar calls, similar.hip) -- selection, ties, exclusions and padding exist once for both.
// Which rows of Q a request row scores is a second policy: every item, position x being item x, or the row's sorted,
// distinct candidate list (mfsgd_recommend_among), position x being the x-th item of it -- the kernels select on
// positions either way, and because a list ascends "ties by the smaller position" is "ties by the smaller item".
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <cstdint>

#include "canon.hpp"
#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {

namespace {

// float -> unsigned whose order is the float order (-0 counts as +0, as a comparison would)
__device__ __forceinline__ unsigned order_key(float f) {
    unsigned u = __builtin_bit_cast(unsigned, f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// with exclusions: 0 is the key of an excluded item, so eligible keys start at 1 (only the all-ones NaN moves)
__device__ __forceinline__ unsigned eligible_key(float f) { return max(order_key(f), 1u); }

// How a kernel below turns dot(P[u], Q[j]) into the score of (u, j) -- a compile-time policy, so that selection, ties,
// exclusions and the final rescoring exist once for both.  Plain: the dot itself (recommend).
struct DotScore {
    __device__ __forceinline__ float row(int) const { return 0.0f; }
    __device__ __forceinline__ float col(int) const { return 0.0f; }
    __device__ __forceinline__ float operator()(float d, float, float) const { return d; }
};
// Cosine (similar.hip): (dot * ra[u]) * rb[j], two roundings in this order, ra / rb the inverse
// norms of the rows of P / Q.  col(j) is loaded beside Q[j], ahead of the reduction that needs it.
struct CosScore {
    const float* __restrict__ ra;
    const float* __restrict__ rb;
    __device__ __forceinline__ float row(int u) const { return ra[u]; }
    __device__ __forceinline__ float col(int j) const { return rb[j]; }
    __device__ __forceinline__ float operator()(float d, float a, float b) const { return (d * a) * b; }
};

// Which rows of Q request row b scores -- the other compile-time policy.  row(b) is what the row scores: n positions,
// position x being item item(x), ascending in x.  seg(b) is where the row's scores start in the sort path's buffers.
// Every item: position x is item x.
struct AllItems {
    static constexpr bool kListed = false;
    int32_t n_items;
    struct Row {
        int n;
        __device__ __forceinline__ int item(int x) const { return x; }
    };
    __device__ __forceinline__ Row row(int) const { return {n_items}; }
    __device__ __forceinline__ long long seg(int b) const { return (long long)b * n_items; }
};
// The candidates of mfsgd_recommend_among: row b scores the sorted, distinct items[off[r] .. off[r + 1]), r = b with
// a list per request row (per_row == 1: off starts at the batch's first row) and 0 with one list for all of them.
struct ListedItems {
    static constexpr bool kListed = true;
    const long long* __restrict__ off;
    const int32_t* __restrict__ items;
    int per_row;
    struct Row {
        const int32_t* __restrict__ it;
        int n;
        __device__ __forceinline__ int item(int x) const { return it[x]; }
    };
    __device__ __forceinline__ Row row(int b) const {
        const int r = b * per_row;
        return {items + off[r], (int)(off[r + 1] - off[r])};
    }
    __device__ __forceinline__ long long seg(int b) const {
        return per_row ? off[b] - off[0] : (long long)b * (off[1] - off[0]);
    }
};

// Is `item` in the sorted, distinct list items[lo .. hi)?  (The listed kernels ask per candidate: a list's candidates are
// not a run of the exclusion list, as a tile of every item is.)
__device__ __forceinline__ bool in_sorted(const int32_t* __restrict__ items, long long lo, const long long hi, const int item) {
    const long long end = hi;
    long long h = hi;
    while (lo < h) {
        const long long mid = (lo + h) >> 1;
        if (items[mid] < item) lo = mid + 1;
        else h = mid;
    }
    return lo < end && items[lo] == item;
}

// scores[seg(b) + x] = score of (users[b], item x of the row) (KEYS: eligible_key of it, as unsigned; 0 for a listed
// item of the user's exclusion list -- of every item, exclude_kernel below does that); ids[...] = the item.
// grid = (item blocks, users)
template <int L, bool KEYS, class S, class Src>
__global__ void __launch_bounds__(256) score_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                    const int32_t* __restrict__ users, const Src src, const RecommendExcl ex,
                                                    const S sc, float* __restrict__ scores, int32_t* __restrict__ ids) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;
    const int lig = threadIdx.x % L;
    const int grp = threadIdx.x / L;
    const int b = blockIdx.y;
    const float4 p = *reinterpret_cast<const float4*>(P + (size_t)users[b] * KP + lig * 4);
    const float ra = sc.row(users[b]);
    const auto v = src.row(b);
    const size_t base = (size_t)src.seg(b);
    long long ex_lo = 0, ex_hi = 0;
    if constexpr (KEYS && Src::kListed) {
        const int s = ex.slot[users[b]];
        ex_lo = ex.off[s];
        ex_hi = ex.off[s + 1];
    }
    const int stride = (int)gridDim.x * GPB;
    const int iters = (v.n + stride - 1) / stride;  // uniform trip count: DPP needs every lane live
    for (int it = 0; it < iters; ++it) {
        const int x = (int)blockIdx.x * GPB + grp + it * stride;
        const bool ok = x < v.n;
        const int i = v.item(ok ? x : 0);
        const float4 q = *reinterpret_cast<const float4*>(Q + (size_t)i * KP + lig * 4);
        const float rb = sc.col(i);
        const float d = sc(group_allreduce<L>(chunk_dot(p, q)), ra, rb);
        if (ok && lig == 0) {
            if constexpr (KEYS) {
                unsigned key = eligible_key(d);
                if constexpr (Src::kListed)
                    if (in_sorted(ex.items, ex_lo, ex_hi, i)) key = 0u;
                reinterpret_cast<unsigned*>(scores)[base + x] = key;
            } else {
                scores[base + x] = d;
            }
            ids[base + x] = i;
        }
    }
}

// ---- fused score + select ----------------------------------------------------------------------------
constexpr int kTopnFused = 128;    // largest topn the fused kernel takes
constexpr int kTopnTile = 14336;   // items scored per tile (56 KiB of keys in LDS: two workgroups per CU)
constexpr int kTopnCand = 2048;    // candidates kept across tiles (tiles x topn must fit)

constexpr int kTopnThreads = 1024;  // 16 waves: the scores are a latency-bound row gather, so many loads in flight

// EXCL: the items of the user's exclusion list get key 0 in each tile and are never candidates; a tile selects
// min(topn, its eligible items), and a row with fewer than topn candidates in all is padded (-1, NaN) -- which a
// listed row (Src) can be without exclusions too: its list may be shorter than topn, or empty.
// (The same workgroup serves a list of a few hundred items, most of it idle through the selection's barriers: one of
// 256 threads and a 4,096-position tile was measured and gained too little to keep)
template <int L, bool EXCL, class S, class Src>
__global__ void __launch_bounds__(kTopnThreads) topn_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                            const int32_t* __restrict__ users, const Src src,
                                                            const int32_t topn, const RecommendExcl ex, const S sc,
                                                            float* __restrict__ out_s, int32_t* __restrict__ out_i) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = kTopnThreads, NW = NT / 64;
    unsigned* keys = reinterpret_cast<unsigned*>(smem);                                   // kTopnTile
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(keys + kTopnTile);   // kTopnCand
    unsigned* hist = reinterpret_cast<unsigned*>(cand + kTopnCand);                        // 256
    unsigned* wtot = hist + 256;                                                           // NW wave totals
    int* ctl = reinterpret_cast<int*>(wtot + NW);  // [0] candidates so far, [1] bin, [2] need, [3] excluded items so far
    constexpr int KP = 4 * L;
    constexpr int GPB = NT / L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lig = tid % L, grp = tid / L;
    const int b = blockIdx.x;
    const float4 p = *reinterpret_cast<const float4*>(P + (size_t)users[b] * KP + lig * 4);
    const float ra = sc.row(users[b]);
    const auto v = src.row(b);  // what this row scores: v.n positions, position x being item v.item(x)
    const int n_items = v.n;
    long long ex_at = 0, ex_end = 0;  // the user's exclusion list, consumed tile by tile (every item) or searched (listed)
    int ex_seen = 0;                  // its items met so far: ctl[3] counts them and is never reset, so no read races a reset
    if constexpr (EXCL) {
        const int s = ex.slot[users[b]];
        ex_at = ex.off[s];
        ex_end = ex.off[s + 1];
    }
    if (tid == 0) {
        ctl[0] = 0;
        if (EXCL) ctl[3] = 0;
    }
    __syncthreads();
    for (int tile0 = 0; tile0 < n_items; tile0 += kTopnTile) {
        const int nt = min(kTopnTile, n_items - tile0);
        // scores of the tile (uniform trip count: the DPP reduction needs every lane live), two rows in flight
        const int iters = (nt + GPB - 1) / GPB;
        int it = 0;
        for (; it + 1 < iters; it += 2) {
            const int x0 = grp + it * GPB, x1 = x0 + GPB;
            const bool ok1 = x1 < nt;
            const int i0 = v.item(tile0 + x0), i1 = v.item(ok1 ? tile0 + x1 : 0);  // (listed: both loads leave first)
            const float4 q0 = *reinterpret_cast<const float4*>(Q + (size_t)i0 * KP + lig * 4);
            const float4 q1 = *reinterpret_cast<const float4*>(Q + (size_t)i1 * KP + lig * 4);
            const float r0 = sc.col(i0), r1 = sc.col(i1);
            const float d0 = sc(group_allreduce<L>(chunk_dot(p, q0)), ra, r0);
            const float d1 = sc(group_allreduce<L>(chunk_dot(p, q1)), ra, r1);
            if (lig == 0) {
                keys[x0] = EXCL ? eligible_key(d0) : order_key(d0);
                if (ok1) keys[x1] = EXCL ? eligible_key(d1) : order_key(d1);
            }
        }
        for (; it < iters; ++it) {
            const int x = grp + it * GPB;
            const bool ok = x < nt;
            const int i = v.item(ok ? tile0 + x : 0);
            const float4 q = *reinterpret_cast<const float4*>(Q + (size_t)i * KP + lig * 4);
            const float r = sc.col(i);
            const float d = sc(group_allreduce<L>(chunk_dot(p, q)), ra, r);
            if (ok && lig == 0) keys[x] = EXCL ? eligible_key(d) : order_key(d);
        }
        __syncthreads();
        // radix select: the key of the need-th largest score of the tile
        int need = min(topn, nt);
        if constexpr (EXCL) {
            // the list is sorted and distinct, so its items in this tile are the next run of it, read from memory.
            // Each thread walks its own stride of the list up to the tile's end (one load per thread and tile rather
            // than a search: a chain of dependent loads cost 1.47x the plain kernel), keys to 0, counted in ctl[3].
            // A listed tile is no run of the exclusion list: each thread looks its own positions' items up in it
            // instead, log2(the user's exclusions) dependent loads per candidate, and the list is never consumed.
            int mine = 0;
            if constexpr (Src::kListed) {
                for (int x = tid; x < nt; x += NT)
                    if (in_sorted(ex.items, ex_at, ex_end, v.item(tile0 + x))) {
                        keys[x] = 0u;
                        ++mine;
                    }
            } else {
                for (long long x = ex_at + tid; x < ex_end; x += NT) {
                    const int item = ex.items[x];
                    if (item >= tile0 + nt) break;
                    keys[item - tile0] = 0u;
                    ++mine;
                }
            }
            if (mine) atomicAdd(&ctl[3], mine);
            __syncthreads();
            const int in_tile = ctl[3] - ex_seen;
            ex_seen += in_tile;
            if constexpr (!Src::kListed) ex_at += in_tile;
            need = min(topn, nt - in_tile);
            if (need == 0) continue;  // nothing eligible (need is uniform across the workgroup)
        }
        unsigned prefix = 0u, mask = 0u;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            // (LDS atomics on a handful of hot bins -- the first digit is sign + exponent -- were measured
            // faster than aggregating equal bins inside a wave first: 2.2 against 4.1 ms per 4,096 users)
            for (int x = tid; x < nt; x += NT) {
                const unsigned kx = keys[x];
                if ((kx & mask) == prefix) atomicAdd(&hist[(kx >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (wave == 0) {
                // bins from the top: lane l owns bins 255 - 4l .. 252 - 4l; counts above by a wave scan
                unsigned h[4], own = 0;
                for (int j = 0; j < 4; ++j) {
                    h[j] = hist[255 - 4 * lane - j];
                    own += h[j];
                }
                unsigned incl = own;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned o = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += o;
                }
                unsigned above = incl - own;  // scores in bins above this lane's
                if (above < (unsigned)need && incl >= (unsigned)need) {
                    for (int j = 0; j < 4; ++j) {
                        if (above + h[j] >= (unsigned)need) {
                            ctl[1] = 255 - 4 * lane - j;
                            ctl[2] = need - (int)above;
                            break;
                        }
                        above += h[j];
                    }
                }
            }
            __syncthreads();
            prefix |= (unsigned)ctl[1] << shift;
            mask |= 0xFFu << shift;
            need = ctl[2];
            __syncthreads();
        }
        // everything above the threshold, then `need` of the ties in ascending item order: each thread owns a
        // contiguous slice, so that "the first `need` by index" is a prefix over threads
        const unsigned T = prefix;
        const int per = (nt + NT - 1) / NT, lo = min(nt, tid * per), hi = min(nt, lo + per);
        int ties = 0;
        for (int x = lo; x < hi; ++x) ties += keys[x] == T ? 1 : 0;
        int incl = ties;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wtot[wave] = (unsigned)incl;
        __syncthreads();
        int tie_rank = incl - ties;
        for (int w2 = 0; w2 < wave; ++w2) tie_rank += (int)wtot[w2];
        for (int x = lo; x < hi; ++x) {
            const unsigned kx = keys[x];
            bool sel = kx > T;
            if (kx == T) {
                sel = tie_rank < need;
                ++tie_rank;
            }
            if (sel) {
                const int at = atomicAdd(&ctl[0], 1);
                // ascending sort of this = score descending, then item ascending
                if (at < kTopnCand) cand[at] = ((unsigned long long)(~kx) << 32) | (unsigned)(tile0 + x);
            }
        }
        __syncthreads();
    }
    // ---- the candidates of all tiles: bitonic sort, best first -----------------------------------------
    const int nc = min(ctl[0], kTopnCand);
    int n2 = 1;
    while (n2 < nc) n2 <<= 1;
    for (int x = nc + tid; x < n2; x += NT) cand[x] = ~0ull;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = tid; x < n2 / 2; x += NT) {
                const int i0 = 2 * x - (x & (stride - 1)), i1 = i0 + stride;
                const bool up = (i0 & size) == 0;
                const unsigned long long a0 = cand[i0], a1 = cand[i1];
                if ((a0 > a1) == up) {
                    cand[i0] = a1;
                    cand[i1] = a0;
                }
            }
            __syncthreads();
        }
    // the winners; their scores recomputed (plain: the canonical dot, the bits predict() returns).  Without
    // exclusions the whole catalogue always has at least topn candidates; with them, or with a list, the places past the
    // last are padded.
    const int iters = (topn + GPB - 1) / GPB;
    for (int it = 0; it < iters; ++it) {
        const int x = grp + it * GPB;
        const bool ok = x < topn;
        const bool won = !(EXCL || Src::kListed) || x < nc;
        const int item = ok && won ? v.item((int)(cand[x] & 0xFFFFFFFFull)) : 0;  // the position back to its item
        const float4 q = *reinterpret_cast<const float4*>(Q + (size_t)item * KP + lig * 4);
        const float d = sc(group_allreduce<L>(chunk_dot(p, q)), ra, sc.col(item));
        if (ok && lig == 0) {
            out_s[(size_t)b * topn + x] = won ? d : __builtin_nanf("");
            out_i[(size_t)b * topn + x] = won ? item : -1;
        }
    }
}

template <int L, bool EXCL, class S, class Src>
hipError_t topn_L(const float* P, const float* Q, const int32_t* users, int nb, const Src& src, int32_t topn,
                  const RecommendExcl& ex, const S& sc, float* out_s, int32_t* out_i, hipStream_t st) {
    const size_t lds = (size_t)kTopnTile * 4 + (size_t)kTopnCand * 8 + 256 * 4 + (kTopnThreads / 64) * 4 + 16;
    hipError_t e = hipFuncSetAttribute((const void*)topn_kernel<L, EXCL, S, Src>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((topn_kernel<L, EXCL, S, Src>), dim3((unsigned)nb), dim3(kTopnThreads), lds, st, P, Q, users, src, topn,
                       ex, sc, out_s, out_i);
    return hipGetLastError();
}

// The sorted rows lie at off[b] .. off[b + 1]; a row shorter than topn (a candidate list can be) is padded.
__global__ void __launch_bounds__(256) take_top_kernel(const float* __restrict__ s, const int32_t* __restrict__ id,
                                                       const long long* __restrict__ off, const int32_t topn,
                                                       float* __restrict__ out_s, int32_t* __restrict__ out_i) {
    const int b = blockIdx.x;
    const size_t o = (size_t)off[b];
    const long long len = off[b + 1] - off[b];
    for (int x = threadIdx.x; x < topn; x += 256) {
        const bool won = x < len;
        out_s[(size_t)b * topn + x] = won ? s[o + x] : __builtin_nanf("");
        out_i[(size_t)b * topn + x] = won ? id[o + x] : -1;
    }
}

// With exclusions the sorted keys are eligible_key()s, not scores: the first topn ids of each row are rescored (plain:
// the canonical dot), and an excluded one (key 0, sorted after every eligible item) ends the row's winners.
template <int L, class S>
__global__ void __launch_bounds__(256) take_top_excl_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                            const int32_t* __restrict__ users,
                                                            const unsigned* __restrict__ key, const int32_t* __restrict__ id,
                                                            const long long* __restrict__ off, const int32_t topn, const S sc,
                                                            float* __restrict__ out_s, int32_t* __restrict__ out_i) {
    constexpr int KP = 4 * L;
    constexpr int GPB = 256 / L;
    const int lig = threadIdx.x % L, grp = threadIdx.x / L;
    const int b = blockIdx.x;
    const float4 p = *reinterpret_cast<const float4*>(P + (size_t)users[b] * KP + lig * 4);
    const float ra = sc.row(users[b]);
    const size_t o = (size_t)off[b];
    const long long len = off[b + 1] - off[b];
    const int iters = (topn + GPB - 1) / GPB;  // uniform trip count: DPP needs every lane live
    for (int it = 0; it < iters; ++it) {
        const int x = grp + it * GPB;
        const bool ok = x < topn;
        const bool won = ok && x < len && key[o + x] != 0u;
        const int item = won ? id[o + x] : 0;
        const float4 q = *reinterpret_cast<const float4*>(Q + (size_t)item * KP + lig * 4);
        const float d = sc(group_allreduce<L>(chunk_dot(p, q)), ra, sc.col(item));
        if (ok && lig == 0) {
            out_s[(size_t)b * topn + x] = won ? d : __builtin_nanf("");
            out_i[(size_t)b * topn + x] = won ? item : -1;
        }
    }
}

// key[b * n_items + i] = 0 for every item i of the exclusion list of users[b]
__global__ void __launch_bounds__(256) exclude_kernel(const int32_t* __restrict__ users, const RecommendExcl ex,
                                                      const int32_t n_items, unsigned* __restrict__ key) {
    const int b = blockIdx.x;
    const int s = ex.slot[users[b]];
    const long long end = ex.off[s + 1];
    for (long long x = ex.off[s] + threadIdx.x; x < end; x += 256) key[(size_t)b * n_items + ex.items[x]] = 0u;
}

// off[x] = where row x starts among the rows of a batch: a fixed stride for every item, the lists' lengths otherwise
template <class Src>
__global__ void __launch_bounds__(256) offsets_kernel(long long* __restrict__ off, const int n, const Src src) {
    for (int x = threadIdx.x; x <= n; x += 256) off[x] = src.seg(x);
}

// stable descending segmented sort of nb rows, `total` (key, id) pairs in all, row b at d_off[b] .. d_off[b + 1];
// K = float (scores) or unsigned (keys)
template <class K>
hipError_t sort_rows(K* k_in, K* k_out, int32_t* id_in, int32_t* id_out, long long* d_off, int nb, long long total,
                     DevBuf& temp, hipStream_t st) {
    size_t need = 0;
    hipError_t e = rocprim::segmented_radix_sort_pairs_desc(nullptr, need, k_in, k_out, id_in, id_out, (unsigned)total,
                                                            (unsigned)nb, d_off, d_off + 1, 0u, 32u, st);
    if (e == hipSuccess) e = temp.alloc(need);
    if (e == hipSuccess)
        e = rocprim::segmented_radix_sort_pairs_desc(temp.get(), need, k_in, k_out, id_in, id_out, (unsigned)total,
                                                     (unsigned)nb, d_off, d_off + 1, 0u, 32u, st);
    return e;
}

// The sort path for nb rows that score `total` positions in all, the longest `longest` of them.
template <int L, class S, class Src>
hipError_t batch_L(const float* P, const float* Q, const int32_t* users, int nb, const Src& src, long long total,
                   long long longest, int32_t topn, const RecommendExcl& ex, const S& sc, float* s_in, float* s_out,
                   int32_t* id_in, int32_t* id_out, long long* d_off, DevBuf& temp, float* out_s, int32_t* out_i,
                   hipStream_t st) {
    if (total == 0) {  // nothing but empty lists: every place is padding
        hipLaunchKernelGGL(offsets_kernel<Src>, dim3(1), dim3(256), 0, st, d_off, nb, src);
        hipLaunchKernelGGL(take_top_kernel, dim3((unsigned)nb), dim3(256), 0, st, s_out, id_out, d_off, topn, out_s, out_i);
        return hipGetLastError();
    }
    const int gpb = 256 / L;
    const int bx = (int)std::min<long long>((longest + gpb - 1) / gpb, 64);
    const dim3 sgrid((unsigned)bx, (unsigned)nb);
    if (ex.slot)
        hipLaunchKernelGGL((score_kernel<L, true, S, Src>), sgrid, dim3(256), 0, st, P, Q, users, src, ex, sc, s_in, id_in);
    else
        hipLaunchKernelGGL((score_kernel<L, false, S, Src>), sgrid, dim3(256), 0, st, P, Q, users, src, ex, sc, s_in, id_in);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if constexpr (!Src::kListed) {  // (a listed row's exclusions were looked up as it was scored)
        if (ex.slot) {
            hipLaunchKernelGGL(exclude_kernel, dim3((unsigned)nb), dim3(256), 0, st, users, ex, src.n_items,
                               reinterpret_cast<unsigned*>(s_in));
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL(offsets_kernel<Src>, dim3(1), dim3(256), 0, st, d_off, nb, src);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!ex.slot) {
        e = sort_rows(s_in, s_out, id_in, id_out, d_off, nb, total, temp, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(take_top_kernel, dim3((unsigned)nb), dim3(256), 0, st, s_out, id_out, d_off, topn, out_s, out_i);
        return hipGetLastError();
    }
    unsigned* k_in = reinterpret_cast<unsigned*>(s_in);
    unsigned* k_out = reinterpret_cast<unsigned*>(s_out);
    e = sort_rows(k_in, k_out, id_in, id_out, d_off, nb, total, temp, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((take_top_excl_kernel<L, S>), dim3((unsigned)nb), dim3(256), 0, st, P, Q, users, k_out, id_out, d_off,
                       topn, sc, out_s, out_i);
    return hipGetLastError();
}

// ---- candidate lists -------------------------------------------------------------------------------------------
// keys[x0 + x] = row << 32 | items[x] for the candidates x0 .. x0 + n of a call: row is the request row whose CSR range
// ptr[row] .. ptr[row + 1] holds position x0 + x (ptr == nullptr: one list, row 0).  The keys then go the way of the
// exclusion pairs' (recommend_excl_lists): sorted and distinct, one ascending list per row.
__global__ void __launch_bounds__(256) cand_keys_kernel(const long long* __restrict__ ptr, const int n_rows,
                                                        const int32_t* __restrict__ items, const long long x0,
                                                        const long long n, unsigned long long* __restrict__ keys) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long x = (long long)blockIdx.x * 256 + threadIdx.x; x < n; x += stride) {
        int lo = 0;
        if (ptr) {  // the last row whose start is <= x0 + x (empty rows before it start there too)
            int hi = n_rows;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ptr[mid + 1] <= x0 + x) lo = mid + 1;
                else hi = mid;
            }
        }
        keys[x0 + x] = ((unsigned long long)lo << 32) | (unsigned)items[x];
    }
}

// ---- exclusion lists -------------------------------------------------------------------------------------------
// keys[...] = slot << 32 | item for each pair (u[x], i[x]) whose user has a slot; one atomic per wave
__global__ void __launch_bounds__(256) excl_filter_kernel(const int32_t* __restrict__ slot_of_user,
                                                          const int32_t* __restrict__ u, const int32_t* __restrict__ i,
                                                          const long long n, unsigned long long* __restrict__ keys,
                                                          unsigned long long* __restrict__ count,
                                                          const unsigned long long cap) {
    const int lane = threadIdx.x & 63;
    for (long long x0 = (long long)blockIdx.x * 256; x0 < n; x0 += (long long)gridDim.x * 256) {
        const long long x = x0 + threadIdx.x;
        const int s = x < n ? slot_of_user[u[x]] : -1;
        const unsigned long long m = __ballot(s >= 0);
        if (m == 0ull) continue;  // wave-uniform
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(count, (unsigned long long)__popcll(m));
        base = __shfl(base, 0, 64);
        const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (s >= 0 && at < cap) keys[at] = ((unsigned long long)s << 32) | (unsigned)i[x];
    }
}

// the sorted distinct keys -> items[x] and off[s] = first key of slot s (off[n_slots] = their count)
__global__ void __launch_bounds__(256) excl_lists_kernel(const unsigned long long* __restrict__ keys,
                                                         const unsigned* __restrict__ n_keys, const int n_slots,
                                                         long long* __restrict__ off, int32_t* __restrict__ items) {
    const long long n = *n_keys;
    const long long stride = (long long)gridDim.x * 256;
    for (long long x = (long long)blockIdx.x * 256 + threadIdx.x; x < n || x <= n_slots; x += stride) {
        if (x < n) items[x] = (int32_t)(keys[x] & 0xFFFFFFFFull);
        if (x <= n_slots) {
            const unsigned long long v = (unsigned long long)x << 32;
            long long lo = 0, hi = n;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (keys[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            off[x] = lo;
        }
    }
}

}  // namespace

bool recommend_is_fused(int64_t longest, int32_t topn) {
    const long long tiles = ((long long)longest + kTopnTile - 1) / kTopnTile;
    return topn <= kTopnFused && tiles * topn <= kTopnCand;
}

// The policies of a batch are chosen here, once: what is scored (every item, or the lists), the score (the dot, or the
// cosine), whether anything is excluded, and the path (without scratch: fused score + select, no score buffers at all).
// One dispatch over L per (path, source), fused before sorted and every item before the lists: the kernels lie in the
// code object in the order of these instantiations, and tools/kernel_identity.py compares it address for address.
hipError_t recommend_topn(const TopnJob& j, const TopnScratch* scratch, hipStream_t st) {
    if (j.among && j.cs.ra) return hipErrorInvalidValue;  // (candidates are scored by the dot: there is no such kernel)
    auto fused = [&](auto l, const auto& src, const auto& sc) {
        constexpr int LL = l();
        return j.ex.slot ? topn_L<LL, true>(j.P, j.Q, j.d_users, j.nb, src, j.topn, j.ex, sc, j.out_s, j.out_i, st)
                         : topn_L<LL, false>(j.P, j.Q, j.d_users, j.nb, src, j.topn, j.ex, sc, j.out_s, j.out_i, st);
    };
    auto sorted = [&](auto l, const auto& src, const auto& sc) {
        return batch_L<l()>(j.P, j.Q, j.d_users, j.nb, src, (long long)j.total, (long long)j.longest, j.topn, j.ex, sc,
                            scratch->s_in, scratch->s_out, scratch->id_in, scratch->id_out, scratch->d_off, *scratch->temp,
                            j.out_s, j.out_i, st);
    };
    const AllItems all{j.n_items};
    const CosScore cos{j.cs.ra, j.cs.rb};
    if (!j.among && !scratch) return with_L(j.L, [&](auto l) { return j.cs.ra ? fused(l, all, cos) : fused(l, all, DotScore{}); });
    if (!j.among) return with_L(j.L, [&](auto l) { return j.cs.ra ? sorted(l, all, cos) : sorted(l, all, DotScore{}); });
    const ListedItems listed{j.among->off, j.among->items, j.among->per_row};
    if (!scratch) return with_L(j.L, [&](auto l) { return fused(l, listed, DotScore{}); });
    return with_L(j.L, [&](auto l) { return sorted(l, listed, DotScore{}); });
}

hipError_t recommend_cand_keys(const long long* ptr, int32_t n_rows, const int32_t* items, int64_t x0, int64_t n,
                               unsigned long long* keys, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const long long blocks = std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(cand_keys_kernel, dim3((unsigned)blocks), dim3(256), 0, st, ptr, (int)n_rows, items, (long long)x0,
                       (long long)n, keys);
    return hipGetLastError();
}

hipError_t recommend_excl_filter(const int32_t* slot_of_user, const int32_t* u, const int32_t* i, int64_t n,
                                 unsigned long long* keys, unsigned long long* count, int64_t cap, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const long long blocks = std::min<long long>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(excl_filter_kernel, dim3((unsigned)blocks), dim3(256), 0, st, slot_of_user, u, i, (long long)n, keys,
                       count, (unsigned long long)cap);
    return hipGetLastError();
}

hipError_t recommend_excl_lists(unsigned long long* keys, unsigned long long* keys_tmp, int64_t n, int32_t n_slots,
                                unsigned* n_distinct, long long* off, int32_t* items, DevBuf& temp, hipStream_t st) {
    unsigned end_bit = 33;  // slot bits above the 32 of the item
    while (end_bit < 64 && ((unsigned long long)(n_slots - 1) >> (end_bit - 32)) != 0) ++end_bit;
    size_t need_sort = 0, need_uniq = 0;
    hipError_t e = rocprim::radix_sort_keys(nullptr, need_sort, keys, keys_tmp, (size_t)n, 0u, end_bit, st);
    if (e == hipSuccess)
        e = rocprim::unique(nullptr, need_uniq, keys_tmp, keys, n_distinct, (size_t)n,
                            rocprim::equal_to<unsigned long long>(), st);
    if (e == hipSuccess) e = temp.alloc(std::max(need_sort, need_uniq));
    if (e == hipSuccess) e = rocprim::radix_sort_keys(temp.get(), need_sort, keys, keys_tmp, (size_t)n, 0u, end_bit, st);
    if (e == hipSuccess)
        e = rocprim::unique(temp.get(), need_uniq, keys_tmp, keys, n_distinct, (size_t)n,
                            rocprim::equal_to<unsigned long long>(), st);
    if (e != hipSuccess) return e;
    const long long work = std::max<long long>(n, (long long)n_slots + 1);
    const long long blocks = std::min<long long>((work + 255) / 256, 4096);
    hipLaunchKernelGGL(excl_lists_kernel, dim3((unsigned)blocks), dim3(256), 0, st, keys, n_distinct, n_slots, off, items);
    return hipGetLastError();
}

}  // namespace mfsgd
