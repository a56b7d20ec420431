// solve.hip -- least-squares fold-in (include/mfsgd.h, "least-squares fold-in"; DESIGN.md, "Fold-in by least squares"):
// the Gram matrix of one side, and per new row the k x k system of its list, factored and solved out of LDS.
//
// Both accumulate sums of outer products f f^T in list order, and both do it with v_mfma_f32_16x16x4_f32: one
// instruction applies four rank-1 updates to a 16 x 16 tile, and its result is bit for bit the fmaf chain over its four
// k steps in ascending order -- which is the rule's chain, four entries at a time.  The A operand carries the row
// index p (scaled by a[j] first, one rounding), the B operand the column index q.  Only the lower triangle is kept:
// with NT tiles of 16 across kp, wave w of the workgroup owns the tile rows w and NT - 1 - w, NT + 1 tiles in all, so
// every wave has the same work and every accumulator a register index that is known at compile time.  A diagonal tile
// is computed whole and its upper half dropped.  A list is padded to a multiple of four with products (-0) * (+0):
// fmaf(-0, +0, x) is x for every x, -0 included.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dispatch.hpp"
#include "kernels.hpp"

#pragma clang fp contract(off)

namespace mfsgd {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int tiles_of(int L) { return (4 * L + 15) / 16; }                        // 16-wide tiles across kp
constexpr int waves_of(int L) { return tiles_of(L) >= 2 ? tiles_of(L) / 2 : 1; }  // waves of a workgroup

// A list of rows of F: ids[first .. first + len), or (ids == nullptr) the rows first .. first + len themselves; a
// nullable (all 1), b nullable (no right-hand side), both indexed like ids.
struct Entries {
    const int32_t* ids;
    const float *a, *b;
    long long first, len;
};

// The lower tiles of one wave: tile row r1 = wave (columns 0 .. r1: lo) and, NT >= 2, r2 = NT - 1 - wave (hi); the
// right-hand side of both tile rows, every column of a tile the same.
template <int NT>
struct Tiles {
    static constexpr int H = NT >= 2 ? NT / 2 : 1;
    f32x4 lo[H], hi[NT], rlo, rhi;
};

__device__ inline int tri(int p) { return p * (p + 1) / 2; }

// Sum over the list, in its order, of t f^T (lower tiles) and b f, on top of +0.0f.  Four entries per step: lane l
// holds entry l >> 4 of the step and column l & 15 of every tile.
template <int NT, int KP>
__device__ void accumulate(const float* __restrict__ F, const int k, const Entries e, const int r1, const int r2, Tiles<NT>& s) {
    constexpr int H = Tiles<NT>::H;
    const int lane = threadIdx.x & 63, kk = lane >> 4, c16 = lane & 15;
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < H; ++c) s.lo[c] = zero;
#pragma unroll
    for (int c = 0; c < NT; ++c) s.hi[c] = zero;
    s.rlo = s.rhi = zero;

    struct Ent {
        long long row;
        float a, b;
        bool valid;
    };
    struct Ops {
        float fB[NT], fA1, fA2, a, b;
    };
    auto load_entry = [&](long long j0) {
        const long long j = j0 + kk;
        Ent n;
        n.valid = j < e.len;
        const long long at = n.valid ? e.first + j : e.first;  // (never read where the list is empty: the callers return first)
        n.row = e.ids ? (long long)e.ids[at] : at;
        n.a = n.valid && e.a ? e.a[at] : 1.0f;
        n.b = n.valid && e.b ? e.b[at] : 0.0f;
        return n;
    };
    auto load_ops = [&](const Ent& n) {
        const float* f = F + (size_t)n.row * KP;
        Ops o;
#pragma unroll
        for (int c = 0; c < NT; ++c) {
            const int col = 16 * c + c16;
            const float v = col < k ? f[col] : 0.0f;  // pad columns never enter
            o.fB[c] = n.valid ? v : 0.0f;
        }
        const int c1 = 16 * r1 + c16, c2 = 16 * r2 + c16;
        const float v1 = c1 < k ? f[c1] : 0.0f, v2 = c2 < k ? f[c2] : 0.0f;
        o.fA1 = n.valid ? v1 : -0.0f;
        o.fA2 = n.valid ? v2 : -0.0f;
        o.a = n.a;
        o.b = n.b;
        return o;
    };
    // entries run two steps ahead of the arithmetic, rows of F one: an address needs its id first
    Ent e1 = load_entry(4);
    Ops o = load_ops(load_entry(0));
    for (long long j0 = 0; j0 < e.len; j0 += 4) {
        const Ent e2 = load_entry(j0 + 8);
        const Ops on = load_ops(e1);
        const float t1 = e.a ? o.a * o.fA1 : o.fA1, t2 = e.a ? o.a * o.fA2 : o.fA2;
#pragma unroll
        for (int c = 0; c < H; ++c)
            if (c <= r1) s.lo[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(t1, o.fB[c], s.lo[c], 0, 0, 0);
        if (NT >= 2) {
#pragma unroll
            for (int c = 0; c < NT; ++c)
                if (c <= r2) s.hi[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(t2, o.fB[c], s.hi[c], 0, 0, 0);
        }
        if (e.b) {
            s.rlo = __builtin_amdgcn_mfma_f32_16x16x4f32(o.fA1, o.b, s.rlo, 0, 0, 0);
            if (NT >= 2) s.rhi = __builtin_amdgcn_mfma_f32_16x16x4f32(o.fA2, o.b, s.rhi, 0, 0, 0);
        }
        o = on;
        e1 = e2;
    }
}

// put(p, q, v) for every element p >= q, p < k of the wave's tiles; put_rhs(p, v) for its rows of the right-hand side.
// (register r of lane l of a tile: row (l >> 4) * 4 + r, column l & 15)
template <int NT, class Put, class PutRhs>
__device__ void for_each_lower(const Tiles<NT>& s, const int r1, const int r2, const int k, Put put, PutRhs put_rhs) {
    constexpr int H = Tiles<NT>::H;
    const int lane = threadIdx.x & 63, rb = (lane >> 4) * 4, c16 = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p1 = 16 * r1 + rb + r, p2 = 16 * r2 + rb + r;
#pragma unroll
        for (int c = 0; c < H; ++c) {
            const int q = 16 * c + c16;
            if (c <= r1 && p1 < k && q <= p1) put(p1, q, s.lo[c][r]);
        }
        if (c16 == 0 && p1 < k) put_rhs(p1, s.rlo[r]);
        if (NT >= 2) {
#pragma unroll
            for (int c = 0; c < NT; ++c) {
                const int q = 16 * c + c16;
                if (c <= r2 && p2 < k && q <= p2) put(p2, q, s.hi[c][r]);
            }
            if (c16 == 0 && p2 < k) put_rhs(p2, s.rhi[r]);
        }
    }
}

// Workgroup t: the partial Gram of tile t, rows [t * tile_rows, min(n, (t + 1) * tile_rows)) of F in ascending order,
// lower triangle of partial[t] (k x k).
template <int L>
__global__ void __launch_bounds__(64 * waves_of(L)) gram_tile_kernel(const float* __restrict__ F, const long long n, const int k,
                                                                     const long long tile_rows, float* __restrict__ partial) {
    constexpr int NT = tiles_of(L);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r1 = wave, r2 = NT - 1 - wave;
    const long long first = (long long)blockIdx.x * tile_rows;
    const long long len = (first + tile_rows < n ? first + tile_rows : n) - first;
    Tiles<NT> s;
    accumulate<NT, 4 * L>(F, k, Entries{nullptr, nullptr, nullptr, first, len}, r1, r2, s);
    float* g = partial + (size_t)blockIdx.x * k * k;
    for_each_lower<NT>(s, r1, r2, k, [&](int p, int q, float v) { g[(size_t)p * k + q] = v; }, [](int, float) {});
}

// G = the partials added in tile order, element by element; the upper triangle a copy of the lower.
__global__ void __launch_bounds__(256) gram_sum_kernel(const float* __restrict__ partial, const int tiles, const int k,
                                                       float* __restrict__ G) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= k * k) return;
    const int p = e / k, q = e % k;
    if (q > p) return;
    float g = partial[e];
    for (int t = 1; t < tiles; ++t) g = g + partial[(size_t)t * k * k + e];
    G[(size_t)p * k + q] = g;
    G[(size_t)q * k + p] = g;
}

// Workgroup g: new row x = perm[g] of the batch.  LDS: A's lower triangle packed by rows (k (k + 1) / 2 floats), then
// rhs, the current column of L, the inverse pivots and y / x, k floats each.
template <int L>
__global__ void __launch_bounds__(64 * waves_of(L)) solve_rows_kernel(const SolveRows j) {
    constexpr int NT = tiles_of(L), T = 64 * waves_of(L), NY = T / 32;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int k = j.k, tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    float* A = reinterpret_cast<float*>(smem);
    float* rhs = A + tri(k);
    float* col = rhs + k;
    float* inv = col + k;
    float* xs = inv + k;
    const int x = j.perm[blockIdx.x];
    const long long len = j.ptr[x + 1] - j.ptr[x];
    float* out = j.rows + (size_t)x * k;
    if (len == 0) {  // the empty list: +0.0f and status 0, no solve
        if (tid < k) out[tid] = 0.0f;
        if (tid == 0 && j.status) j.status[x] = 0;
        return;
    }
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r1 = wave, r2 = NT - 1 - wave;
    {
        Tiles<NT> s;
        accumulate<NT, 4 * L>(j.F, k, Entries{j.ids, j.a, j.b, j.ptr[x] - j.base, len}, r1, r2, s);
        for_each_lower<NT>(s, r1, r2, k, [&](int p, int q, float v) { A[tri(p) + q] = v; }, [&](int p, float v) { rhs[p] = v; });
    }
    __syncthreads();
    if (j.alpha != 0.0f) {
        for (int p = ty; p < k; p += NY)
            for (int q = tx; q <= p; q += 32) A[tri(p) + q] = __builtin_fmaf(j.alpha, j.G[(size_t)p * k + q], A[tri(p) + q]);
        __syncthreads();
    }
    const float dg = __builtin_fmaf(j.ridge_per_entry, (float)len, j.ridge);
    for (int p = tid; p < k; p += T) A[tri(p) + p] = A[tri(p) + p] + dg;
    __syncthreads();
    // Cholesky, right-looking: column c of L, then its outer product off what is to the right of it.  Every element
    // meets the columns in ascending order, so its chain is the rule's.
    int failed = 0;
    for (int c = 0; c < k; ++c) {
        const float s = A[tri(c) + c];  // (every thread the same)
        if (!(s > 0.0f)) {
            failed = c + 1;
            break;
        }
        const float iv = 1.0f / __builtin_sqrtf(s);
        for (int i = c + 1 + tid; i < k; i += T) {
            const float v = A[tri(i) + c] * iv;
            A[tri(i) + c] = v;
            col[i] = v;
        }
        if (tid == 0) inv[c] = iv;
        __syncthreads();
        for (int i = c + 1 + ty; i < k; i += NY) {
            const float li = col[i];
            for (int q = c + 1 + tx; q <= i; q += 32) A[tri(i) + q] = __builtin_fmaf(-li, col[q], A[tri(i) + q]);
        }
        __syncthreads();
    }
    if (failed) {  // (uniform)
        if (tid < k) out[tid] = __builtin_bit_cast(float, 0x7FC00000u);
        if (tid == 0 && j.status) j.status[x] = failed;
        return;
    }
    // forward, by columns: once y[t] is there, every later row takes it off its sum
    float s = tid < k ? rhs[tid] : 0.0f;
    for (int t = 0; t < k; ++t) {
        if (tid == t) xs[t] = s * inv[t];
        __syncthreads();
        if (tid > t && tid < k) s = __builtin_fmaf(-A[tri(tid) + t], xs[t], s);
    }
    __syncthreads();
    s = tid < k ? xs[tid] : 0.0f;
    __syncthreads();  // every y is read before the first x takes its place
    float xv = 0.0f;
    for (int t = k - 1; t >= 0; --t) {
        if (tid == t) xs[t] = xv = s * inv[t];
        __syncthreads();
        if (tid < t) s = __builtin_fmaf(-A[tri(t) + tid], xs[t], s);
    }
    if (tid < k) out[tid] = xv;
    if (tid == 0 && j.status) j.status[x] = 0;
}

}  // namespace

int64_t gram_tile_rows(int64_t n) { return 256 * ((n + 65535) / 65536); }
int64_t gram_tiles(int64_t n) { return (n + gram_tile_rows(n) - 1) / gram_tile_rows(n); }

hipError_t launch_gram(int L, const float* F, int64_t n, int k, float* partial, float* G, hipStream_t st) {
    if (n <= 0) return hipErrorInvalidValue;
    const long long tile_rows = gram_tile_rows(n);
    const int tiles = (int)gram_tiles(n);
    const hipError_t e = with_L(L, [&](auto l) {
        hipLaunchKernelGGL((gram_tile_kernel<l()>), dim3((unsigned)tiles), dim3(64 * waves_of(l())), 0, st, F, (long long)n, k,
                           tile_rows, partial);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gram_sum_kernel, dim3((unsigned)((k * k + 255) / 256)), dim3(256), 0, st, partial, tiles, k, G);
    return hipGetLastError();
}

hipError_t launch_solve_rows(int L, const SolveRows& a, hipStream_t st) {
    if (a.nb <= 0) return hipSuccess;
    const int k = a.k;
    const int lds = (k * (k + 1) / 2 + 4 * k) * (int)sizeof(float);
    return with_L(L, [&](auto l) {
        const hipError_t e =
            hipFuncSetAttribute((const void*)solve_rows_kernel<l()>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((solve_rows_kernel<l()>), dim3((unsigned)a.nb), dim3(64 * waves_of(l())), lds, st, a);
        return hipGetLastError();
    });
}

}  // namespace mfsgd
