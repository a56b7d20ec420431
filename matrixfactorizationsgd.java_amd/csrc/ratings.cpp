// ratings.cpp -- from rating triples to schedules on the device: the rating hash, mfsgd_set_ratings, the DSGD item
// map and plan, and the getters that show what was built.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "handle.hpp"
#include "ingest.hpp"
#include "jrandom.hpp"

namespace mfsgd {

void default_item_map(mfsgd_handle* h) {
    const int G = h->n_parts;
    const int32_t I = h->cfg.n_items;
    h->item_part.resize((size_t)I);
    h->item_row.resize((size_t)I);
    h->part_q_rows.assign((size_t)G, 0);
    for (int32_t x = 0; x < I; ++x) {
        h->item_part[(size_t)x] = x % G;
        h->item_row[(size_t)x] = x / G;
    }
    for (int g = 0; g < G; ++g) h->part_q_rows[(size_t)g] = (I - g + G - 1) / G;
    h->custom_item_map = false;
}

static int ensure_part_on_device(mfsgd_handle* h, Part& p) {
    if (p.on_device) return MFSGD_OK;
    int rc;
    if ((rc = upload(h, p.d_cells, p.sched.cells))) return rc;
    DevicePacked& dev = p.sched.dev;
    if (p.sched.device_packed && dev.subs) {
        p.d_subs = std::move(dev.subs);  // (the device assembled the sub-cell tables too)
    } else if ((rc = upload(h, p.d_subs, p.sched.subs))) {
        return rc;
    }
    if (p.sched.device_packed) {
        // the device packer left rows and entries where they are needed: the partition's arrays own them from here on
        p.d_rows = std::move(dev.rows);
        p.d_entries = std::move(dev.entries);
    } else {
        if ((rc = upload(h, p.d_rows, p.sched.rows))) return rc;
        if ((rc = upload(h, p.d_entries, p.sched.entries))) return rc;
    }
    if ((rc = dev_alloc(h, p.d_sse_partial, sizeof(double) * p.sched.cells.size()))) return rc;
    if ((rc = dev_alloc(h, p.d_sse_out, 1))) return rc;
    if ((rc = dev_alloc(h, p.d_sync, sync_bytes(p) / sizeof(unsigned)))) return rc;
    HIPCHK(h, hipMemset(p.d_sync.data(), 0, sync_bytes(p)));
    HIPCHK(h, hipDeviceSynchronize());  // (memset is asynchronous; the first launch may be on another stream)
    p.on_device = true;
    return MFSGD_OK;
}

int prepare_compute(mfsgd_handle* h) {
    if (!h->have_ratings) return fail(h, MFSGD_ERR_STATE, "no ratings: call mfsgd_set_ratings first");
    int rc = factors_to_device(h);
    if (rc) return rc;
    for (Part& p : h->parts)
        if ((rc = ensure_part_on_device(h, p))) return rc;
    return MFSGD_OK;
}

// Host copies of a device-packed schedule's big arrays, made when somebody asks for them
// (mfsgd_get_order, the debug getters): they never existed on the host.
static int host_copies(const mfsgd_handle* h, const Part& cp, bool want_order, bool want_arrays) {
    Part& p = const_cast<Part&>(cp);
    Schedule& s = p.sched;
    if (!s.device_packed) return MFSGD_OK;
    // rows, entries and subs are the schedule's until the first compute call, the partition's after it
    const DevBuf& d_rows = p.on_device ? p.d_rows.buf() : s.dev.rows.buf();
    const DevBuf& d_entries = p.on_device ? p.d_entries.buf() : s.dev.entries.buf();
    const DevBuf& d_subs = p.on_device ? p.d_subs.buf() : s.dev.subs.buf();
    auto download = [](void* host, const DevBuf& dev, size_t bytes) {
        if (bytes == 0) return true;
        if (bytes <= dev.bytes() && hipMemcpy(host, dev.get(), bytes, hipMemcpyDeviceToHost) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    };
    try {
        if (want_order && s.order.empty() && s.nnz > 0) {
            s.order.resize_uninit((size_t)s.nnz);
            if (!download(s.order.data(), s.dev.order.buf(), s.order.size() * sizeof(int64_t)))
                return fail(h, MFSGD_ERR_HIP, "could not copy the canonical order from the device");
        }
        if (want_arrays && s.subs.empty() && s.n_sub_recs > 0 && d_subs) {
            s.subs.resize((size_t)s.n_sub_recs);
            if (!download(s.subs.data(), d_subs, s.subs.size() * sizeof(SubDesc)))
                return fail(h, MFSGD_ERR_HIP, "could not copy the sub-cell tables from the device");
        }
        if (want_arrays && s.entries.empty() && s.n_entry_recs > 0) {
            s.rows.resize_uninit((size_t)s.n_rows_words);
            s.entries.resize_uninit((size_t)s.n_entry_recs);
            if (!download(s.rows.data(), d_rows, s.rows.size() * sizeof(uint32_t)) ||
                !download(s.entries.data(), d_entries, s.entries.size() * sizeof(Entry)))
                return fail(h, MFSGD_ERR_HIP, "could not copy the schedule from the device");
        }
        return MFSGD_OK;
    } catch (const std::bad_alloc&) {
        return fail(h, MFSGD_ERR_OOM, "out of host memory");  // (without the caller's name: the text this failure has)
    }
}

// fn(0) here and fn(1) .. fn(nt - 1) on threads of their own; returns when all have.  A thread that cannot be
// started is an exception for the caller's guard, thrown once those that did start have finished.
template <class F>
static void run_on_threads(int nt, F&& fn) {
    std::vector<std::thread> th;
    th.reserve((size_t)std::max(0, nt - 1));
    try {
        for (int t = 1; t < nt; ++t) th.emplace_back([&fn, t] { fn(t); });
        fn(0);
    } catch (...) {
        for (auto& t : th) t.join();
        throw;
    }
    for (auto& t : th) t.join();
}

// 2 x 64-bit multiply-xorshift hash of the three rating arrays (every byte; the array boundaries and
// the length are mixed in), computed in parallel over fixed 1 MiB pieces so that it does not depend on
// the thread count.  Not cryptographic; 128 bits make an accidental match of two different rating sets
// (the only thing it guards against) a non-event.
static void hash_ratings(const int32_t* u, const int32_t* i, const float* r, int64_t n, int threads, uint64_t out[2]) {
    constexpr uint64_t M1 = 0x9E3779B97F4A7C15ull, M2 = 0xC2B2AE3D27D4EB4Full;
    constexpr int64_t kPiece = 1 << 18;  // elements per piece
    const int64_t pieces = (n + kPiece - 1) / kPiece;
    std::vector<uint64_t> ph((size_t)pieces * 6, 0);
    auto piece_hash = [&](const void* base, int64_t lo, int64_t hi, uint64_t& a, uint64_t& b) {
        const unsigned char* p = static_cast<const unsigned char*>(base) + lo * 4;
        const int64_t bytes = (hi - lo) * 4;
        uint64_t h1 = 0x243F6A8885A308D3ull ^ (uint64_t)bytes, h2 = 0x13198A2E03707344ull + (uint64_t)bytes;
        int64_t x = 0;
        for (; x + 8 <= bytes; x += 8) {
            uint64_t w;
            std::memcpy(&w, p + x, 8);
            h1 = (h1 ^ w) * M1;
            h1 ^= h1 >> 32;
            h2 = (h2 + w) * M2;
            h2 ^= h2 >> 29;
        }
        if (x < bytes) {
            uint64_t w = 0;
            std::memcpy(&w, p + x, (size_t)(bytes - x));
            h1 = (h1 ^ w) * M1;
            h1 ^= h1 >> 32;
            h2 = (h2 + w) * M2;
            h2 ^= h2 >> 29;
        }
        a = h1;
        b = h2;
    };
    std::atomic<int64_t> next{0};
    int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(nt, 64), pieces));
    run_on_threads(nt, [&](int) {
        for (;;) {
            const int64_t c = next.fetch_add(1);
            if (c >= pieces) break;
            const int64_t lo = c * kPiece, hi = std::min(n, lo + kPiece);
            piece_hash(u, lo, hi, ph[(size_t)c * 6 + 0], ph[(size_t)c * 6 + 1]);
            piece_hash(i, lo, hi, ph[(size_t)c * 6 + 2], ph[(size_t)c * 6 + 3]);
            piece_hash(r, lo, hi, ph[(size_t)c * 6 + 4], ph[(size_t)c * 6 + 5]);
        }
    });
    uint64_t h1 = 0x452821E638D01377ull ^ (uint64_t)n, h2 = 0xBE5466CF34E90C6Cull + (uint64_t)n;
    for (size_t x = 0; x < ph.size(); x += 2) {
        h1 = (h1 ^ ph[x]) * M1;
        h1 ^= h1 >> 32;
        h2 = (h2 + ph[x + 1]) * M2;
        h2 ^= h2 >> 29;
    }
    out[0] = h1;
    out[1] = h2;
}

// mfsgd_set_ratings, step by step -------------------------------------------------
// The rating arrays of one call, as every step sees them.
struct Triples {
    const int32_t* u;
    const int32_t* i;
    const float* r;
    int64_t nnz;
};

// MFSGD_SCHED_TRACE: the time each step took, on stderr
struct Lap {
    const bool trace = std::getenv("MFSGD_SCHED_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[set_ratings] %-25s %.3f s\n", what, std::chrono::duration<double>(now - t_last).count());
        t_last = now;
    }
};

// The same triples again (Java / C++ / Python hosts hand train() the same arrays every call): keep
// the schedules and their device copies.  Exact: length + 128-bit hash of every byte.
static bool same_ratings(const mfsgd_handle* h, int64_t nnz, const uint64_t hash[2]) {
    return h->have_ratings && h->nnz_total == nnz && hash[0] == h->ratings_hash[0] && hash[1] == h->ratings_hash[1];
}

// drop what an earlier call built (device copies included)
static void release_schedules(mfsgd_handle* h) {
    if (h->device_ready) {
        (void)hipSetDevice(h->cfg.device);
        (void)hipStreamSynchronize(h->stream);
    }
    h->parts.clear();
    h->have_ratings = false;
}

// range check, on the host threads: first offending rating, if any
static int check_range(const mfsgd_handle* h, const Triples& t) {
    const int32_t *u = t.u, *i = t.i;
    const int64_t nnz = t.nnz;
    int nt = h->cfg.host_threads > 0 ? h->cfg.host_threads : (int)std::thread::hardware_concurrency();
    nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(nt, 64), nnz >> 16));
    std::vector<int64_t> first_bad((size_t)nt, nnz);
    run_on_threads(nt, [&](int th) {
        const int64_t lo = nnz * th / nt, hi = nnz * (th + 1) / nt;
        const int32_t nu = h->cfg.n_users, ni = h->cfg.n_items;
        for (int64_t j = lo; j < hi; ++j)
            if ((uint32_t)u[j] >= (uint32_t)nu || (uint32_t)i[j] >= (uint32_t)ni) {
                first_bad[(size_t)th] = j;
                return;
            }
    });
    const int64_t j = *std::min_element(first_bad.begin(), first_bad.end());
    if (j < nnz)
        return fail(h, MFSGD_ERR_INVALID_ARG, "set_ratings: rating " + std::to_string(j) + " has (u,i) = (" +
                                                  std::to_string(u[j]) + "," + std::to_string(i[j]) + ") out of range");
    return MFSGD_OK;
}

// Ingestion (degree histograms, bucket order) runs on the GPU when there is one and the
// rating set is large enough to pay for the upload; the host loops are the fallback.
struct IngestContext {
    std::unique_ptr<DeviceIngest> ingest;  // null: host loops
    IngestContext(mfsgd_handle* h, int64_t nnz) {
        const bool want_dev = !(h->cfg.flags & MFSGD_FLAG_HOST_INGEST) &&
                              ((h->cfg.flags & MFSGD_FLAG_DEVICE_INGEST) || nnz >= (int64_t)1 << 20);
        if (!want_dev) return;
        if (ensure_device(h) == MFSGD_OK) ingest = make_device_ingest(h->cfg.device);
        else h->err.clear();  // no device: not an error for a host-side call
    }
};

static SchedParams sched_params(const mfsgd_handle* h, DeviceIngest* ingest) {
    SchedParams prm;
    prm.ingest = ingest;
    prm.U = h->cfg.n_users;
    prm.k = h->cfg.k;
    prm.lr = h->cfg.lr;
    prm.lambda = h->cfg.lambda;
    prm.B = h->cfg.blocks;
    prm.W = h->cfg.waves;
    prm.threads = h->cfg.host_threads;
    prm.solo = !(h->cfg.flags & MFSGD_FLAG_NO_SOLO);
    prm.device_pack = !(h->cfg.flags & MFSGD_FLAG_HOST_PACK);
    if (const char* e = std::getenv("MFSGD_LDS_BUDGET")) {  // (A/B measurements: e.g. 81408 = two workgroups per CU)
        const int v = std::atoi(e);
        if (v >= 16 * 1024 && v <= prm.lds_budget) prm.lds_budget = v;
    }
    return prm;
}

static int build_single(mfsgd_handle* h, SchedParams prm, const Triples& t, Lap& lap) {
    const int32_t *u = t.u, *i = t.i;
    const int64_t nnz = t.nnz;
    Part& p = h->parts[0];
    p.q_rows = h->cfg.n_items;
    // rating counts per user and per item: on the device when it ingests, else here; they
    // decide which side carries the longest chain and are handed on to the scheduler
    std::vector<int64_t> du((size_t)h->cfg.n_users, 0), di((size_t)h->cfg.n_items, 0);
    DeviceIngest* const ingest = prm.ingest;
    if (ingest) ingest->load(u, i, nnz);
    if (!(ingest && ingest->degrees(h->cfg.n_users, h->cfg.n_items, du.data(), di.data()) == 0)) {
        std::fill(du.begin(), du.end(), 0);
        std::fill(di.begin(), di.end(), 0);
        for (int64_t j = 0; j < nnz; ++j) {
            du[(size_t)u[j]]++;
            di[(size_t)i[j]]++;
        }
    }
    const int64_t mu = du.empty() ? 0 : *std::max_element(du.begin(), du.end());
    const int64_t mi = di.empty() ? 0 : *std::max_element(di.begin(), di.end());
    prm.validated = true;  // check_range checked every (u, i)
    lap("degrees + role decision");
    p.swapped = mu > mi;
    std::string err;
    int rc;
    prm.degu = p.swapped ? di.data() : du.data();
    prm.degi = p.swapped ? du.data() : di.data();
    if (p.swapped) {
        prm.U = h->cfg.n_items;
        prm.I = h->cfg.n_users;
        if (ingest) ingest->load(i, u, nnz);  // (the roles exchanged: another rating set to the device)
        rc = build_schedule_auto(prm, i, u, t.r, nullptr, nnz, p.sched, err);
    } else {
        prm.I = p.q_rows;
        rc = build_schedule_auto(prm, u, i, t.r, nullptr, nnz, p.sched, err);
    }
    if (ingest) ingest->drop();
    if (rc != 0) return fail(h, MFSGD_ERR_SCHEDULE, err);
    return MFSGD_OK;
}

static int build_partitioned(mfsgd_handle* h, SchedParams prm, const Triples& t, Lap& lap) {
    const int32_t *u = t.u, *i = t.i;
    const float* r = t.r;
    const int64_t nnz = t.nnz;
    const int G = h->n_parts;
    // item i -> partition item_part[i], local row item_row[i]: one counting sort of the rating
    // indices by partition, then one schedule per partition
    std::vector<int64_t> pptr((size_t)G + 1, 0);
    for (int64_t j = 0; j < nnz; ++j) pptr[(size_t)h->item_part[(size_t)i[j]] + 1]++;
    for (int g = 0; g < G; ++g) pptr[(size_t)g + 1] += pptr[(size_t)g];
    std::vector<int64_t> orig((size_t)nnz);
    {
        std::vector<int64_t> cur(pptr.begin(), pptr.end() - 1);
        for (int64_t j = 0; j < nnz; ++j) orig[(size_t)cur[(size_t)h->item_part[(size_t)i[j]]]++] = j;
    }
    lap("partition split");
    for (int g = 0; g < G; ++g) {
        const int64_t lo = pptr[(size_t)g], m = pptr[(size_t)g + 1] - lo;
        std::vector<int32_t> uu((size_t)m), ii((size_t)m);
        std::vector<float> rr((size_t)m);
        for (int64_t x = 0; x < m; ++x) {
            const int64_t j = orig[(size_t)(lo + x)];
            uu[(size_t)x] = u[j];
            ii[(size_t)x] = h->item_row[(size_t)i[j]];
            rr[(size_t)x] = r[j];
        }
        Part& p = h->parts[(size_t)g];
        p.q_rows = h->part_q_rows[(size_t)g];
        // every partition is a rating set of its own to the device ingest (uu / ii of two partitions of equal size sit
        // at the same addresses: the allocator hands the block back)
        if (prm.ingest) prm.ingest->load(uu.data(), ii.data(), m);
        prm.I = std::max<int32_t>(1, p.q_rows);
        prm.validated = true;  // check_range checked; local rows are in range by construction
        // the partition's own rating counts per row: build_schedule_auto compares the longest chain with the
        // partition's work when it picks the wave count (a chain-bound partition runs on two waves, a
        // work-bound one on four), exactly as for a single-partition handle
        std::vector<int64_t> du((size_t)h->cfg.n_users, 0), di((size_t)prm.I, 0);
        for (int64_t x = 0; x < m; ++x) {
            du[(size_t)uu[(size_t)x]]++;
            di[(size_t)ii[(size_t)x]]++;
        }
        prm.degu = du.data();
        prm.degi = di.data();
        std::string err;
        const int rc = build_schedule_auto(prm, uu.data(), ii.data(), rr.data(), orig.data() + lo, m, p.sched, err);
        if (prm.ingest) prm.ingest->drop();  // (uu / ii go with this iteration)
        if (rc != 0)
            return fail(h, MFSGD_ERR_SCHEDULE, "partition " + std::to_string(g) + ": " + err);
    }
    return MFSGD_OK;
}

static void commit_ratings(mfsgd_handle* h, int64_t nnz, const uint64_t hash[2]) {
    h->nnz_total = nnz;
    h->ratings_hash[0] = hash[0];
    h->ratings_hash[1] = hash[1];
    h->n_schedule_builds++;
    h->have_ratings = true;
}

}  // namespace mfsgd

using namespace mfsgd;

extern "C" {

int mfsgd_set_ratings(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, int64_t nnz) {
    return guarded(h, "set_ratings", [&]() -> int {
        if (nnz < 0 || (nnz > 0 && (!u || !i || !r))) return fail(h, MFSGD_ERR_INVALID_ARG, "set_ratings: null array or negative nnz");
        const Triples t{u, i, r, nnz};
        Lap lap;
        int rc;
        uint64_t hash[2];
        hash_ratings(u, i, r, nnz, h->cfg.host_threads, hash);
        if (same_ratings(h, nnz, hash)) {
            h->n_schedule_reuses++;
            return MFSGD_OK;
        }
        lap("hash of the triples");
        release_schedules(h);
        if ((rc = check_range(h, t))) return rc;
        lap("release + range check");
        h->parts.resize((size_t)h->n_parts);
        IngestContext ic(h, nnz);
        lap("device ingest context");
        const SchedParams prm = sched_params(h, ic.ingest.get());
        rc = h->n_parts == 1 ? build_single(h, prm, t, lap) : build_partitioned(h, prm, t, lap);
        if (rc) return rc;
        lap("schedules");
        commit_ratings(h, nnz, hash);
        return MFSGD_OK;
    }, MFSGD_ERR_INVALID_ARG);
}

int mfsgd_dsgd_plan(const int64_t* deg_user, const int64_t* deg_item, int32_t n_users, int32_t n_items, int32_t n_parts,
                    int32_t* user_begin, int32_t* item_part) {
    return guarded_free(nullptr, [&]() -> int {
        if (!deg_user || !deg_item || !user_begin || !item_part || n_users < 1 || n_items < 1 || n_parts < 1)
            return MFSGD_ERR_INVALID_ARG;
        for (int32_t x = 0; x < n_users; ++x)
            if (deg_user[x] < 0) return MFSGD_ERR_INVALID_ARG;
        for (int32_t x = 0; x < n_items; ++x)
            if (deg_item[x] < 0) return MFSGD_ERR_INVALID_ARG;
        dsgd_plan(deg_user, deg_item, n_users, n_items, n_parts, user_begin, item_part);
        return MFSGD_OK;
    });
}

int mfsgd_dsgd_plan_ex(const int64_t* deg_user, const int64_t* deg_item, int32_t n_users, int32_t n_items, int32_t world,
                       int32_t parts_per_rank, int32_t k, float chain_crit, int32_t* user_begin, int32_t* item_part,
                       int64_t* info4) {
    return guarded_free(nullptr, [&]() -> int {
        if (!deg_user || !deg_item || !user_begin || !item_part || n_users < 1 || n_items < 1 || world < 1 || parts_per_rank < 1 ||
            k < 1 || k > MFSGD_MAX_K || (int64_t)world * parts_per_rank > INT32_MAX || !(chain_crit >= 0.f))
            return MFSGD_ERR_INVALID_ARG;
        for (int32_t x = 0; x < n_users; ++x)
            if (deg_user[x] < 0) return MFSGD_ERR_INVALID_ARG;
        for (int32_t x = 0; x < n_items; ++x)
            if (deg_item[x] < 0) return MFSGD_ERR_INVALID_ARG;
        dsgd_plan_users(deg_user, n_users, world, user_begin);
        dsgd_plan_items(deg_item, n_items, world * parts_per_rank, world, k, (double)chain_crit, item_part, info4);
        return MFSGD_OK;
    });
}

int mfsgd_set_item_partition(mfsgd_handle* h, const int32_t* item_part) {
    return guarded(h, "set_item_partition", [&]() -> int {
        if (h->n_parts <= 1) return fail(h, MFSGD_ERR_STATE, "set_item_partition: handle has a single partition");
        if (h->have_ratings) return fail(h, MFSGD_ERR_STATE, "set_item_partition: call it before mfsgd_set_ratings");
        if (!item_part) {
            default_item_map(h);
            return MFSGD_OK;
        }
        const int G = h->n_parts;
        const int32_t I = h->cfg.n_items;
        for (int32_t x = 0; x < I; ++x)
            if (item_part[x] < 0 || item_part[x] >= G)
                return fail(h, MFSGD_ERR_INVALID_ARG, "set_item_partition: item " + std::to_string(x) + " has partition " +
                                                          std::to_string(item_part[x]) + " out of range");
        h->item_part.assign(item_part, item_part + I);
        h->item_row.assign((size_t)I, 0);
        h->part_q_rows.assign((size_t)G, 0);
        for (int32_t x = 0; x < I; ++x) h->item_row[(size_t)x] = h->part_q_rows[(size_t)item_part[x]]++;
        h->custom_item_map = true;
        return MFSGD_OK;
    });
}

int mfsgd_get_item_partition(const mfsgd_handle* h, int32_t* item_part, int32_t* item_row) {
    return guarded(h, "get_item_partition", [&]() -> int {
        if (h->n_parts <= 1) return fail(h, MFSGD_ERR_STATE, "get_item_partition: handle has a single partition");
        if (item_part) std::memcpy(item_part, h->item_part.data(), h->item_part.size() * sizeof(int32_t));
        if (item_row) std::memcpy(item_row, h->item_row.data(), h->item_row.size() * sizeof(int32_t));
        return MFSGD_OK;
    });
}

int mfsgd_part_rows(const mfsgd_handle* h, int32_t part, int32_t* rows) {
    return guarded(h, "part_rows", [&]() -> int {
        if (!rows) return fail(h, MFSGD_ERR_INVALID_ARG, "part_rows: null argument");
        if (int rc = check_part(h, part, "part_rows")) return rc;
        *rows = h->n_parts > 1 ? h->part_q_rows[(size_t)part] : h->cfg.n_items;
        return MFSGD_OK;
    });
}

int mfsgd_part_init_q(const mfsgd_handle* h, int32_t part, int64_t seed, int64_t u_total, float* q_block_host) {
    return guarded(h, "part_init_q", [&]() -> int {
        if (!q_block_host || u_total < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "part_init_q: bad argument");
        if (int rc = check_part(h, part, "part_init_q")) return rc;
        const int k = h->cfg.k, kp = h->geo.kp;
        const float scale = (float)(1.0 / std::sqrt((double)k));
        // items of this partition in ascending id order = ascending row order; the stream position of
        // item i is (u_total + i) * k
        JRandom g(seed);
        int64_t pos = 0;  // floats drawn so far
        for (int32_t x = 0; x < h->cfg.n_items; ++x) {
            if (h->n_parts > 1 && h->item_part[(size_t)x] != part) continue;
            const int64_t want = ((int64_t)u_total + x) * k;
            g.skip((uint64_t)(want - pos));
            float* row = q_block_host + (size_t)(h->n_parts > 1 ? h->item_row[(size_t)x] : x) * kp;
            for (int f = 0; f < k; ++f) row[f] = g.nextFloat() * scale;
            for (int f = k; f < kp; ++f) row[f] = 0.0f;
            pos = want + k;
        }
        return MFSGD_OK;
    });
}

int mfsgd_get_schedule_info(const mfsgd_handle* h, int32_t part, mfsgd_schedule_info* out) {
    return guarded(h, "get_schedule_info", [&]() -> int {
        if (!out) return fail(h, MFSGD_ERR_INVALID_ARG, "get_schedule_info: null argument");
        if (!h->have_ratings) return fail(h, MFSGD_ERR_STATE, "get_schedule_info: no ratings");
        if (int rc = check_part(h, part, "get_schedule_info")) return rc;
        const Schedule& s = h->parts[(size_t)part].sched;
        std::memset(out, 0, sizeof *out);
        out->nnz = s.nnz;
        out->part = part;
        out->blocks = s.B;
        out->waves = s.W;
        out->group_lanes = s.geo.L;
        out->slots = s.geo.G;
        out->kp = s.geo.kp;
        out->rounds = s.B;
        out->lds_bytes = s.lds_bytes;
        out->total_steps = s.total_steps;
        out->total_rows = s.total_rows;
        out->max_cell_nnz = s.max_cell_nnz;
        out->max_cell_rows = s.max_cell_rows;
        out->max_cell_steps = s.max_cell_steps;
        out->sum_round_steps = s.sum_round_steps;
        out->build_seconds = s.build_seconds;
        out->swapped = h->parts[(size_t)part].swapped ? 1 : 0;
        out->device_ingest = s.device_packed ? 2 : s.device_ingest ? 1 : 0;
        out->chunks = (int64_t)s.cells.size();
        out->split_cells = s.split_cells;
        return MFSGD_OK;
    });
}

int mfsgd_get_order(const mfsgd_handle* h, int32_t part, int64_t* order, int64_t* cell_ptr) {
    return guarded(h, "get_order", [&]() -> int {
        if (!h->have_ratings) return fail(h, MFSGD_ERR_STATE, "get_order: no ratings");
        if (int rc = check_part(h, part, "get_order")) return rc;
        if (order) {
            const int rc = host_copies(h, h->parts[(size_t)part], true, false);
            if (rc) return rc;
        }
        const Schedule& s = h->parts[(size_t)part].sched;
        if (order && !s.order.empty()) std::memcpy(order, s.order.data(), s.order.size() * sizeof(int64_t));
        if (cell_ptr) std::memcpy(cell_ptr, s.cell_ptr.data(), s.cell_ptr.size() * sizeof(int64_t));
        return MFSGD_OK;
    });
}

int mfsgd_debug_schedule_sizes(const mfsgd_handle* h, int32_t part, int64_t* n_cells, int64_t* n_rows,
                               int64_t* n_subs, int64_t* n_entries) {
    return guarded(h, "debug_schedule_sizes", [&]() -> int {
        if (!n_cells || !n_rows || !n_subs || !n_entries) return fail(h, MFSGD_ERR_INVALID_ARG, "debug_schedule_sizes: null argument");
        if (!h->have_ratings) return fail(h, MFSGD_ERR_STATE, "debug_schedule_sizes: no ratings");
        if (int rc = check_part(h, part, "debug_schedule_sizes")) return rc;
        const Schedule& s = h->parts[(size_t)part].sched;
        *n_cells = (int64_t)s.cells.size();
        *n_rows = s.n_rows_words;
        *n_subs = s.subs.empty() ? s.n_sub_recs : (int64_t)s.subs.size();
        *n_entries = s.n_entry_recs;
        return MFSGD_OK;
    });
}

int mfsgd_debug_get_schedule(const mfsgd_handle* h, int32_t part, uint32_t* cells, uint32_t* rows, uint32_t* subs,
                             uint32_t* entries) {
    return guarded(h, "debug_get_schedule", [&]() -> int {
        if (!h->have_ratings) return fail(h, MFSGD_ERR_STATE, "debug_get_schedule: no ratings");
        if (int rc = check_part(h, part, "debug_get_schedule")) return rc;
        if (rows || entries || subs) {
            const int rc = host_copies(h, h->parts[(size_t)part], false, true);
            if (rc) return rc;
        }
        const Schedule& s = h->parts[(size_t)part].sched;
        if (cells && !s.cells.empty()) std::memcpy(cells, s.cells.data(), s.cells.size() * sizeof(CellDesc));
        if (rows && !s.rows.empty()) std::memcpy(rows, s.rows.data(), s.rows.size() * sizeof(uint32_t));
        if (subs && !s.subs.empty()) std::memcpy(subs, s.subs.data(), s.subs.size() * sizeof(SubDesc));
        if (entries && !s.entries.empty()) std::memcpy(entries, s.entries.data(), s.entries.size() * sizeof(Entry));
        return MFSGD_OK;
    });
}

}  // extern "C"
