// ingest.hip -- the implementation of DeviceIngest (ingest.hpp), the only one.  Streaming passes over the COO triples:
// HBM-bound integer work (coalesced reads of u/i, random 4-byte gathers of the bin maps, one LSD radix sort), and the
// host side of the device packer (pack.hip).  Every allocation is a DevBuf; what emit() produces leaves in DevBufs.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "devmem.hpp"
#include "ingest.hpp"
#include "hugepages.hpp"
#include "pack.hpp"

namespace mfsgd {

namespace {

// What bucket_dev() and the COUNT pass leave on the device for the packer's later calls.  Dropping it is assigning an
// empty one: every buffer is freed by its owner.
struct PackState {
    DevBuf sorted;                   // unsigned x n: rating indices in bucket order
    DevBuf bptr;                     // long long x (nb + 1)
    int64_t nb = 0;
    DevBuf r;                        // float x n
    DevBuf orig;                     // long long x n, or empty
    DevBuf urank, irank;             // int32 per row
    DevBuf info;                     // PackCellInfo per cell
    DevBuf subs;                     // SubDesc x W*W per cell
    PackArgs args{};                 // as launched for COUNT; EMIT reuses it
    int64_t n_cells = 0;
    int rows_full = 0;               // the row capacity no cell (or part of one) can exceed
    // one-pass mode: what the COUNT pass already wrote
    struct OnePass {
        DevBuf srows;                // uint32: scratch rows (2 per rating)
        DevBuf sent;                 // Entry: scratch entries (worst-case strides)
        DevBuf order;                // long long x n: the canonical order, final
        DevBuf ord_off;              // long long per cell
    } one;
};

// A list of parts (chunks) on the device, as the packing kernel's cells (upload_parts)
struct PartList {
    DevBuf sorted, cptr, info, subs;
};

// The device ingest there is (ingest.hpp).  The loaded triples go to the device with the first call that needs them
// and stay there, with what was derived from them, until drop() or the next load().
struct Ingest final : DeviceIngest {
    const int device;
    const int32_t* u = nullptr;      // host: the loaded set
    const int32_t* i = nullptr;
    int64_t n = -1;
    DevBuf du, di;                   // int32 x n each: its copy, once a call needed it
    PackState pk;

    explicit Ingest(int dev) : device(dev) {}
    void load(const int32_t* u_, const int32_t* i_, int64_t n_) override {
        drop();
        u = u_;
        i = i_;
        n = n_;
    }
    void drop() override {
        unload();
        u = i = nullptr;
        n = -1;
    }
    int64_t loaded() const override { return n; }
    int degrees(int32_t U, int32_t I, int64_t* degu, int64_t* degi) override;
    int bucket(const int32_t* ubin, const int32_t* ibin, int32_t U, int32_t I, int B, int W, int giants, int64_t* bptr,
               int64_t* sorted) override;
    int bucket_dev(const int32_t* ubin, const int32_t* ibin, int32_t U, int32_t I, int B, int W, int giants,
                   int64_t* bptr) override;
    int fetch_sorted32(uint32_t* sorted) override;
    int fetch_sorted_ranges(int64_t n_ranges, const int64_t* lo, const int64_t* len, uint32_t* out) override;
    int pack_count(const PackRequest& q, std::vector<PackCellInfo>& info) override;
    int pack_count_parts(const PartsToEmit& parts, PackCellInfo* info) override;
    int emit(const CellOffsets& cells, const PartsToEmit* parts, DevicePacked& out) override;

    void unload();  // frees the device copy and what was derived from it
    bool ensure_triples();
    int bucket_on_device(const int32_t* ubin, const int32_t* ibin, int32_t U, int32_t I, int B, int W, int giants);
    int fetch_bptr(int64_t* bptr);
    int fetch_sorted(int64_t* sorted);
    bool upload_parts(const PartsToEmit& parts, PartList& pl, PackArgs& a);
};

// A HIP call failed: the call answers -1 (the host loops take over); what it allocated goes with its owners.
#define ING_CHK(call)                 \
    do {                              \
        if ((call) != hipSuccess) {   \
            (void)hipGetLastError();  \
            return -1;                \
        }                             \
    } while (0)

void Ingest::unload() {
    pk = PackState{};
    du.reset();
    di.reset();
}

bool Ingest::ensure_triples() {
    if (du) return true;
    if (n < 0) return false;
    if (hipSetDevice(device) != hipSuccess) return false;
    const size_t bytes = (size_t)(n > 0 ? n : 1) * sizeof(int32_t);
    if (du.alloc(bytes) != hipSuccess || di.alloc(bytes) != hipSuccess ||
        hipMemcpy(du.get(), u, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(di.get(), i, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        unload();
        return false;
    }
    return true;
}

__global__ void __launch_bounds__(256) degree_kernel(const int32_t* __restrict__ u, const int32_t* __restrict__ i,
                                                     const int64_t n, unsigned* __restrict__ degu,
                                                     unsigned* __restrict__ degi) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        atomicAdd(&degu[u[j]], 1u);
        atomicAdd(&degi[i[j]], 1u);
    }
}

// The same with ONE side's counts kept in the LDS and flushed at the end: the global atomics of a popular row all hit
// one address (232 K increments of one word at the Netflix shape: 11 ms for 100 M ratings); a workgroup's LDS takes
// them at LDS speed and hands on one sum per row it saw.  `small` = the side with at most kDegLdsRows rows.
constexpr int kDegLdsRows = 36 * 1024;  // x 4 B = 144 KiB of LDS
__global__ void __launch_bounds__(1024) degree_lds_kernel(const int32_t* __restrict__ big, const int32_t* __restrict__ small_ids,
                                                          const int64_t n, unsigned* __restrict__ deg_big,
                                                          unsigned* __restrict__ deg_small, const int n_small) {
    extern __shared__ unsigned hist[];
    for (int x = threadIdx.x; x < n_small; x += blockDim.x) hist[x] = 0u;
    __syncthreads();
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        atomicAdd(&deg_big[big[j]], 1u);
        atomicAdd(&hist[small_ids[j]], 1u);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < n_small; x += blockDim.x)
        if (hist[x] != 0u) atomicAdd(&deg_small[x], hist[x]);
}

__global__ void __launch_bounds__(256) key_kernel(const int32_t* __restrict__ u, const int32_t* __restrict__ i,
                                                  const int64_t n, const int32_t* __restrict__ ubin,
                                                  const int32_t* __restrict__ ibin, const int B, const int W,
                                                  const int giants, unsigned* __restrict__ key,
                                                  unsigned* __restrict__ val) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
        const int fu = ubin[u[j]], fi = ibin[i[j]];
        const int ub = fu % B, us = fi < giants ? 0 : fu / B, it = fi % B, is = fi / B;
        const int s = (is - us + W) % W;
        key[j] = (unsigned)((((long long)ub * B + it) * W + s) * W + us);
        val[j] = (unsigned)j;
    }
}

// bptr[b] = first position whose key is >= b (keys sorted ascending); bptr[nb] = n
__global__ void __launch_bounds__(256) bound_kernel(const unsigned* __restrict__ key, const int64_t n, const int64_t nb,
                                                    long long* __restrict__ bptr) {
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b <= nb; b += (int64_t)gridDim.x * 256) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)key[mid] < b) lo = mid + 1;
            else hi = mid;
        }
        bptr[b] = lo;
    }
}

int grid_for(int64_t n) {
    int64_t g = (n + 255) / 256;
    if (g > 256 * 8) g = 256 * 8;  // 2048 workgroups, grid-stride beyond
    return (int)(g < 1 ? 1 : g);
}

int Ingest::degrees(int32_t U, int32_t I, int64_t* degu, int64_t* degi) {
    if (n >= (int64_t)1 << 32) return -1;
    if (!ensure_triples()) return -1;
    std::vector<unsigned> hu((size_t)U), hi((size_t)I);
    {
        DevBuf bu, bi;
        ING_CHK(bu.alloc(sizeof(unsigned) * (size_t)U));
        ING_CHK(bi.alloc(sizeof(unsigned) * (size_t)I));
        unsigned *d_u = bu.as<unsigned>(), *d_i = bi.as<unsigned>();
        const int32_t *d_uu = du.as<int32_t>(), *d_ii = di.as<int32_t>();
        ING_CHK(hipMemset(d_u, 0, sizeof(unsigned) * (size_t)U));
        ING_CHK(hipMemset(d_i, 0, sizeof(unsigned) * (size_t)I));
        if (std::min(U, I) <= kDegLdsRows && n >= (1 << 20)) {
            const bool items_small = I <= U;
            const int n_small = items_small ? I : U;
            const size_t lds = 4 * (size_t)n_small;
            ING_CHK(hipFuncSetAttribute((const void*)degree_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(degree_lds_kernel, dim3(256), dim3(1024), lds, 0, items_small ? d_uu : d_ii, items_small ? d_ii : d_uu, n,
                               items_small ? d_u : d_i, items_small ? d_i : d_u, n_small);
        } else {
            hipLaunchKernelGGL(degree_kernel, dim3(grid_for(n)), dim3(256), 0, 0, d_uu, d_ii, n, d_u, d_i);
        }
        ING_CHK(hipGetLastError());
        ING_CHK(hipMemcpy(hu.data(), d_u, sizeof(unsigned) * (size_t)U, hipMemcpyDeviceToHost));
        ING_CHK(hipMemcpy(hi.data(), d_i, sizeof(unsigned) * (size_t)I, hipMemcpyDeviceToHost));
    }
    for (int32_t x = 0; x < U; ++x) degu[x] = hu[(size_t)x];
    for (int32_t x = 0; x < I; ++x) degi[x] = hi[(size_t)x];
    return 0;
}

// Keys, one stable LSD radix sort of (key, index) pairs, bucket starts.  Leaves the sorted indices and
// the bucket starts on the device (pk.sorted, pk.bptr).
int Ingest::bucket_on_device(const int32_t* ubin, const int32_t* ibin, int32_t U, int32_t I, int B, int W, int giants) {
    const int64_t nb = (int64_t)B * B * W * W;
    if (n >= (int64_t)1 << 32 || nb >= (int64_t)1 << 32) return -1;
    if (!ensure_triples()) return -1;
    pk = PackState{};
    DevBuf d_ubin, d_ibin, k0, k1, v0, v1, d_bptr, temp;  // all but v1 and d_bptr go when this returns
    size_t temp_bytes = 0;
    const size_t nn = (size_t)(n > 0 ? n : 1);
    unsigned bits = 1;
    while (((int64_t)1 << bits) < nb) ++bits;
    ING_CHK(d_ubin.alloc(sizeof(int32_t) * (size_t)U));
    ING_CHK(d_ibin.alloc(sizeof(int32_t) * (size_t)I));
    ING_CHK(hipMemcpy(d_ubin.get(), ubin, sizeof(int32_t) * (size_t)U, hipMemcpyHostToDevice));
    ING_CHK(hipMemcpy(d_ibin.get(), ibin, sizeof(int32_t) * (size_t)I, hipMemcpyHostToDevice));
    ING_CHK(k0.alloc(4 * nn));
    ING_CHK(k1.alloc(4 * nn));
    ING_CHK(v0.alloc(4 * nn));
    ING_CHK(v1.alloc(4 * nn));
    ING_CHK(d_bptr.alloc(sizeof(long long) * (size_t)(nb + 1)));
    unsigned *key_in = k0.as<unsigned>(), *key_out = k1.as<unsigned>(), *val_in = v0.as<unsigned>(), *val_out = v1.as<unsigned>();
    hipLaunchKernelGGL(key_kernel, dim3(grid_for(n)), dim3(256), 0, 0, du.as<int32_t>(), di.as<int32_t>(), n,
                       d_ubin.as<int32_t>(), d_ibin.as<int32_t>(), B, W, giants, key_in, val_in);
    ING_CHK(hipGetLastError());
    // LSD radix sort: stable, so equal keys keep their input order -- the host counting sort's order
    ING_CHK(rocprim::radix_sort_pairs(nullptr, temp_bytes, key_in, key_out, val_in, val_out, (size_t)n, 0u, bits, (hipStream_t)0));
    ING_CHK(temp.alloc(temp_bytes));
    ING_CHK(rocprim::radix_sort_pairs(temp.get(), temp_bytes, key_in, key_out, val_in, val_out, (size_t)n, 0u, bits, (hipStream_t)0));
    hipLaunchKernelGGL(bound_kernel, dim3(grid_for(nb + 1)), dim3(256), 0, 0, key_out, n, nb, d_bptr.as<long long>());
    ING_CHK(hipGetLastError());
    ING_CHK(hipDeviceSynchronize());
    pk.sorted = std::move(v1);
    pk.bptr = std::move(d_bptr);
    pk.nb = nb;
    return 0;
}

int Ingest::fetch_bptr(int64_t* bptr) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the bucket starts come down as they are");
    if (hipMemcpy(bptr, pk.bptr.get(), sizeof(long long) * (size_t)(pk.nb + 1), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return 0;
}

int Ingest::fetch_sorted(int64_t* sorted) {
    if (!pk.sorted) return -1;
    std::vector<unsigned> hv((size_t)(n > 0 ? n : 1));
    if (hipMemcpy(hv.data(), pk.sorted.get(), 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    for (int64_t j = 0; j < n; ++j) sorted[j] = (int64_t)hv[(size_t)j];
    return 0;
}

int Ingest::fetch_sorted32(uint32_t* sorted) {
    if (!pk.sorted) return -1;
    if (n > 0 && hipMemcpy(sorted, pk.sorted.get(), 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return 0;
}

// out[dst[x] + y] = sorted[lo[x] + y], y < len[x]: one workgroup per range
__global__ void __launch_bounds__(256) gather_ranges_kernel(const unsigned* __restrict__ sorted, const long long* __restrict__ lo,
                                                            const long long* __restrict__ len, const long long* __restrict__ dst,
                                                            unsigned* __restrict__ out) {
    const long long a = lo[blockIdx.x], n = len[blockIdx.x], d = dst[blockIdx.x];
    for (long long y = threadIdx.x; y < n; y += 256) out[d + y] = sorted[a + y];
}

int Ingest::fetch_sorted_ranges(int64_t n_ranges, const int64_t* lo, const int64_t* len, uint32_t* out) {
    if (!pk.sorted || n_ranges < 0) return -1;
    if (n_ranges == 0) return 0;
    std::vector<long long> dst((size_t)n_ranges);
    long long total = 0;
    for (int64_t x = 0; x < n_ranges; ++x) {
        if (lo[x] < 0 || len[x] < 0 || lo[x] + len[x] > n) return -1;
        dst[(size_t)x] = total;
        total += len[x];
    }
    if (total == 0) return 0;
    DevBuf d_lo, d_len, d_dst, d_out;
    static_assert(sizeof(long long) == sizeof(int64_t), "ranges are uploaded as they are");
    ING_CHK(d_lo.alloc(8 * (size_t)n_ranges));
    ING_CHK(d_len.alloc(8 * (size_t)n_ranges));
    ING_CHK(d_dst.alloc(8 * (size_t)n_ranges));
    ING_CHK(d_out.alloc(4 * (size_t)total));
    ING_CHK(hipMemcpy(d_lo.get(), lo, 8 * (size_t)n_ranges, hipMemcpyHostToDevice));
    ING_CHK(hipMemcpy(d_len.get(), len, 8 * (size_t)n_ranges, hipMemcpyHostToDevice));
    ING_CHK(hipMemcpy(d_dst.get(), dst.data(), 8 * (size_t)n_ranges, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(gather_ranges_kernel, dim3((unsigned)n_ranges), dim3(256), 0, 0, pk.sorted.as<unsigned>(),
                       d_lo.as<long long>(), d_len.as<long long>(), d_dst.as<long long>(), d_out.as<unsigned>());
    ING_CHK(hipGetLastError());
    ING_CHK(hipMemcpy(out, d_out.get(), 4 * (size_t)total, hipMemcpyDeviceToHost));
    return 0;
}

int Ingest::bucket_dev(const int32_t* ubin, const int32_t* ibin, int32_t U, int32_t I, int B, int W, int giants,
                       int64_t* bptr) {
    if (bucket_on_device(ubin, ibin, U, I, B, W, giants) != 0) return -1;
    return fetch_bptr(bptr);
}

int Ingest::bucket(const int32_t* ubin, const int32_t* ibin, int32_t U, int32_t I, int B, int W, int giants, int64_t* bptr,
                   int64_t* sorted) {
    if (bucket_on_device(ubin, ibin, U, I, B, W, giants) != 0) return -1;
    const int rc = fetch_bptr(bptr) == 0 && fetch_sorted(sorted) == 0 ? 0 : -1;
    pk = PackState{};
    return rc;
}

// ---- the device packer (pack.hip) -------------------------------------------------------------------
// rank of every row among the rows of its block (block = bin % B), ascending row index
void block_ranks(const int32_t* bin, int32_t n, int B, std::vector<int32_t>& rank, int32_t& max_rank) {
    std::vector<int32_t> next((size_t)B, 0);
    rank.resize((size_t)n);
    for (int32_t x = 0; x < n; ++x) rank[(size_t)x] = next[(size_t)(bin[x] % B)]++;
    max_rank = 0;
    for (int b = 0; b < B; ++b) max_rank = std::max(max_rank, next[(size_t)b]);
}

int Ingest::pack_count(const PackRequest& q, std::vector<PackCellInfo>& info) {
    if (!pk.sorted || !pk.bptr) return -1;
    const int64_t n_cells = (int64_t)q.B * q.B, WW = (int64_t)q.W * q.W;
    if (n_cells >= (int64_t)1 << 31 || q.G > 64) return 1;
    std::vector<int32_t> ur, ir;
    int32_t mu = 0, mi = 0;
    block_ranks(q.ubin, q.U, q.B, ur, mu);
    block_ranks(q.ibin, q.I, q.B, ir, mi);
    PackArgs a{};
    a.max_m = (int)((std::max<int64_t>(q.max_cell_nnz, 64) + 63) / 64 * 64);
    if (mu > 65535 || mi > 65535 || a.max_m > 2048) return 1;  // 16-bit ranks, 32 candidates per lane
    a.u_words = (mu + 31) / 32 + 1;
    a.i_words = (mi + 31) / 32 + 1;
    // rows a cell can touch: at most 2 per rating and at most what the blocks hold; the training kernel's LDS
    // image (160 KiB) cannot hold more than 10240 16-byte units of rows anyway.  Most cells touch far fewer, and
    // the kernel's occupancy hangs on this number (its per-wave state arrays), so a first launch provides for
    // 512 and only a set with fuller cells pays for a second launch with the full bound.
    int rows_full = std::max(8, (int)std::min<int64_t>(std::min<int64_t>(2 * (int64_t)a.max_m, (int64_t)mu + mi), 32767 / std::max(1, q.L)));
    if (q.fit_rows > 0) rows_full = std::max(8, std::min(rows_full, q.fit_rows));  // (more rows than fit: cut anyway)
    a.max_rows = std::min(rows_full, 512);
    a.B = q.B;
    a.W = q.W;
    a.G = q.G;
    a.L = q.L;
    a.lr = q.lr;
    a.c = q.c;
    a.solo_ok = q.solo_ok ? 1 : 0;
    {
        PackArgs worst = a;
        worst.max_rows = rows_full;
        if (pack_lds_bytes(worst) > 160 * 1024 - 256) return 1;
    }
    const size_t nn = (size_t)std::max<int64_t>(n, 1);
    ING_CHK(pk.r.alloc(sizeof(float) * nn));
    ING_CHK(hipMemcpy(pk.r.get(), q.r, sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
    if (q.orig) {
        ING_CHK(pk.orig.alloc(sizeof(long long) * nn));
        ING_CHK(hipMemcpy(pk.orig.get(), q.orig, sizeof(long long) * (size_t)n, hipMemcpyHostToDevice));
    }
    ING_CHK(pk.urank.alloc(sizeof(int32_t) * (size_t)q.U));
    ING_CHK(pk.irank.alloc(sizeof(int32_t) * (size_t)q.I));
    ING_CHK(hipMemcpy(pk.urank.get(), ur.data(), sizeof(int32_t) * (size_t)q.U, hipMemcpyHostToDevice));
    ING_CHK(hipMemcpy(pk.irank.get(), ir.data(), sizeof(int32_t) * (size_t)q.I, hipMemcpyHostToDevice));
    ING_CHK(pk.info.alloc(sizeof(PackCellInfo) * (size_t)n_cells));
    ING_CHK(pk.subs.alloc(sizeof(SubDesc) * (size_t)(n_cells * WW)));
    a.u = du.as<int32_t>();
    a.i = di.as<int32_t>();
    a.r = pk.r.as<float>();
    a.orig = pk.orig.as<long long>();
    a.sorted = pk.sorted.as<unsigned>();
    a.bptr = pk.bptr.as<long long>();
    a.urank = pk.urank.as<int32_t>();
    a.irank = pk.irank.as<int32_t>();
    a.info = pk.info.as<PackCellInfo>();
    a.subs = pk.subs.as<SubDesc>();
    a.emit = 0;
    if (q.ord_off && !std::getenv("MFSGD_PACK_TWICE")) {  // (the variable: A/B measurements)
        // one-pass mode: scratch for rows and entries, the order array itself; if any of it does not fit, count only
        // (nor when the scratch would take more than a third of what is free: the final arrays come after it)
        const size_t steps = pack_scratch_steps(n, n_cells, q.W);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        const size_t need = sizeof(Entry) * steps * (size_t)q.G + 16 * nn;
        if (need <= free_b / 3 && pk.one.srows.alloc(4 * (2 * nn)) == hipSuccess &&
            pk.one.sent.alloc(sizeof(Entry) * steps * (size_t)q.G) == hipSuccess && pk.one.order.alloc(8 * nn) == hipSuccess &&
            pk.one.ord_off.alloc(8 * (size_t)n_cells) == hipSuccess &&
            hipMemcpy(pk.one.ord_off.get(), q.ord_off, 8 * (size_t)n_cells, hipMemcpyHostToDevice) == hipSuccess) {
            a.emit = 2;
            a.rows = pk.one.srows.as<uint32_t>();
            a.entries = pk.one.sent.as<Entry>();
            a.order = pk.one.order.as<long long>();
            a.ord_off = pk.one.ord_off.as<long long>();
        } else {
            (void)hipGetLastError();
            pk.one = PackState::OnePass{};
        }
    }
    reserve_huge(info, (size_t)n_cells);
    info.resize((size_t)n_cells);
    for (;;) {
        ING_CHK(launch_pack(a, n_cells, (hipStream_t)0));
        ING_CHK(hipMemcpy(info.data(), pk.info.get(), sizeof(PackCellInfo) * (size_t)n_cells, hipMemcpyDeviceToHost));
        bool more_rows = false;
        for (const PackCellInfo& ci : info) more_rows = more_rows || ci.status == 2;
        if (!more_rows || a.max_rows >= rows_full) break;
        a.max_rows = rows_full;
    }
    pk.args = a;
    pk.n_cells = n_cells;
    pk.rows_full = rows_full;
    return 0;
}

// A list of parts (chunks) as the packing kernel's cells: uploads it and returns the arguments of a launch over it
// (COUNT outputs allocated), which live as long as `pl`.
bool Ingest::upload_parts(const PartsToEmit& parts, PartList& pl, PackArgs& a) {
    const int64_t n_parts = parts.n_parts, n_sorted = parts.n_sorted;
    const int64_t WW = (int64_t)pk.args.W * pk.args.W;
    static_assert(sizeof(long long) == sizeof(int64_t), "cptr is uploaded as it is");
    if (pl.sorted.alloc(4 * (size_t)std::max<int64_t>(n_sorted, 1)) != hipSuccess ||
        pl.cptr.alloc(8 * (size_t)(n_parts * WW + 1)) != hipSuccess ||
        pl.info.alloc(sizeof(PackCellInfo) * (size_t)n_parts) != hipSuccess ||
        pl.subs.alloc(sizeof(SubDesc) * (size_t)(n_parts * WW)) != hipSuccess ||
        hipMemcpy(pl.sorted.get(), parts.sorted, 4 * (size_t)n_sorted, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(pl.cptr.get(), parts.cptr, 8 * (size_t)(n_parts * WW + 1), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    a = pk.args;
    a.rows = nullptr;  // (a COUNT pass proper: the cells' one-pass scratch is not the parts')
    a.entries = nullptr;
    a.order = nullptr;
    a.ord_off = nullptr;
    a.max_rows = pk.rows_full;  // a part can hold any number of rows a cell can
    a.sorted = pl.sorted.as<unsigned>();
    a.bptr = pl.cptr.as<long long>();
    a.info = pl.info.as<PackCellInfo>();
    a.subs = pl.subs.as<SubDesc>();
    a.emit = 0;
    return true;
}

int Ingest::pack_count_parts(const PartsToEmit& parts, PackCellInfo* info) {
    if (!pk.info || parts.n_parts < 0) return -1;
    if (parts.n_parts == 0) return 0;
    PartList pl;
    PackArgs a{};
    if (!upload_parts(parts, pl, a)) return -1;
    ING_CHK(launch_pack(a, parts.n_parts, (hipStream_t)0));
    ING_CHK(hipMemcpy(info, pl.info.get(), sizeof(PackCellInfo) * (size_t)parts.n_parts, hipMemcpyDeviceToHost));
    return 0;
}

// fin[desc[y] * WW + x] = src[y * WW + x]: the parts' sub-cell tables to their chunk descriptors
__global__ void __launch_bounds__(256) table_scatter_kernel(SubDesc* __restrict__ fin, const SubDesc* __restrict__ src,
                                                            const long long* __restrict__ desc, const long long n_parts, const int WW) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= n_parts * WW) return;
    fin[desc[x / WW] * WW + x % WW] = src[x];
}

int Ingest::emit(const CellOffsets& cells, const PartsToEmit* parts, DevicePacked& out) {
    if (!pk.info) return -1;
    const int64_t n_rows = cells.n_rows, n_steps = cells.n_steps, n_descs = cells.n_descs;
    PackArgs a = pk.args;
    DevBuf ro, eo, oo, pdesc;         // the offsets, for the length of this call
    DevBuf rows, ent, order, fin;     // what `out` gets: fin = the final sub-cell table
    const size_t nc = (size_t)pk.n_cells;
    const bool one_pass = (bool)pk.one.sent;  // the COUNT pass wrote what it packed: move it, do not pack again
    const size_t WWs = (size_t)a.W * a.W;
    std::vector<long long> oo_host(cells.ord_off, cells.ord_off + nc);
    if (n_descs < pk.n_cells) return -1;
    ING_CHK(ro.alloc(4 * nc));
    ING_CHK(eo.alloc(4 * nc));
    ING_CHK(oo.alloc(8 * nc));
    ING_CHK(hipMemcpy(ro.get(), cells.row_off, 4 * nc, hipMemcpyHostToDevice));
    ING_CHK(hipMemcpy(eo.get(), cells.ent_off, 4 * nc, hipMemcpyHostToDevice));
    ING_CHK(hipMemcpy(oo.get(), oo_host.data(), 8 * nc, hipMemcpyHostToDevice));
    ING_CHK(rows.alloc(4 * (size_t)(n_rows + 4)));
    ING_CHK(hipMemset(rows.as<uint32_t>() + n_rows, 0, 16));  // the staging DMA reads whole 16-byte units
    ING_CHK(ent.alloc(sizeof(Entry) * (size_t)std::max<int64_t>(n_steps * a.G, 1)));
    if (one_pass)
        order = std::move(pk.one.order);  // written by the COUNT pass, at its final place
    else
        ING_CHK(order.alloc(8 * (size_t)std::max<int64_t>(n, 1)));
    a.row_off = ro.as<uint32_t>();
    a.ent_off = eo.as<uint32_t>();
    a.ord_off = oo.as<long long>();
    a.rows = rows.as<uint32_t>();
    a.entries = ent.as<Entry>();
    a.order = order.as<long long>();
    // the final sub-cell table: the cells' tables as the COUNT pass left them (a cell that is cut gets its first chunk's
    // below), zeros for the descriptors nothing is written to and for the two padding records
    ING_CHK(fin.alloc(sizeof(SubDesc) * ((size_t)n_descs * WWs + 2)));
    SubDesc* d_fin = fin.as<SubDesc>();
    ING_CHK(hipMemsetAsync(d_fin + nc * WWs, 0, sizeof(SubDesc) * ((size_t)(n_descs - pk.n_cells) * WWs + 2), (hipStream_t)0));
    ING_CHK(hipMemcpyAsync(d_fin, pk.subs.get(), sizeof(SubDesc) * nc * WWs, hipMemcpyDeviceToDevice, (hipStream_t)0));
    if (one_pass) {
        a.emit = 2;
        ING_CHK(launch_compact(a, pk.n_cells, pk.one.srows.as<uint32_t>(), pk.one.sent.as<Entry>(), (hipStream_t)0));
    } else {
        a.emit = 1;
        ING_CHK(launch_pack(a, pk.n_cells, (hipStream_t)0));
    }
    if (parts && parts->n_parts > 0) {
        // the chunks of the cells that were cut: COUNT over the final list (the EMIT pass reads the sub-cell table the
        // COUNT pass of the SAME list left on the device), then EMIT at the caller's offsets into the same arrays.
        // The list and its offsets go at the end of this block, before the arrays are handed on.
        PartList pl;
        PackArgs pa{};
        DevBuf p_ro, p_eo, p_oo;
        const size_t np = (size_t)parts->n_parts;
        if (!upload_parts(*parts, pl, pa)) return -1;
        ING_CHK(launch_pack(pa, parts->n_parts, (hipStream_t)0));
        ING_CHK(p_ro.alloc(4 * np));
        ING_CHK(p_eo.alloc(4 * np));
        ING_CHK(p_oo.alloc(8 * np));
        ING_CHK(hipMemcpy(p_ro.get(), parts->row_off, 4 * np, hipMemcpyHostToDevice));
        ING_CHK(hipMemcpy(p_eo.get(), parts->ent_off, 4 * np, hipMemcpyHostToDevice));
        ING_CHK(hipMemcpy(p_oo.get(), parts->ord_off, 8 * np, hipMemcpyHostToDevice));
        pa.emit = 1;
        pa.row_off = p_ro.as<uint32_t>();
        pa.ent_off = p_eo.as<uint32_t>();
        pa.ord_off = p_oo.as<long long>();
        pa.rows = a.rows;
        pa.entries = a.entries;
        pa.order = a.order;
        ING_CHK(launch_pack(pa, parts->n_parts, (hipStream_t)0));
        // (the EMIT pass does not touch the table the COUNT pass of the same list left in pl.subs)
        if (!parts->desc) return -1;
        ING_CHK(pdesc.alloc(8 * np));
        ING_CHK(hipMemcpy(pdesc.get(), parts->desc, 8 * np, hipMemcpyHostToDevice));
        const long long tot = (long long)np * a.W * a.W;
        hipLaunchKernelGGL(table_scatter_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)0, d_fin,
                           pl.subs.as<SubDesc>(), pdesc.as<long long>(), (long long)np, a.W * a.W);
        ING_CHK(hipGetLastError());
        ING_CHK(hipDeviceSynchronize());
    }
    ING_CHK(hipDeviceSynchronize());
    out.rows = std::move(rows);
    out.entries = std::move(ent);
    out.order = std::move(order);
    out.subs = std::move(fin);
    out.n_subs = n_descs * (int64_t)WWs + 2;
    pk = PackState{};
    return 0;
}

}  // namespace

std::unique_ptr<DeviceIngest> make_device_ingest(int device) { return std::make_unique<Ingest>(device); }

}  // namespace mfsgd
