// handle.cpp -- the handle of the C-ABI (include/mfsgd.h): its life cycle, the error channel, device bring-up, and
// the factors (seed, set, get, upload, and growing them: rows appended in place, capacity).
//
// No reference counterpart exists; the surface follows SURVEY.md section 8b.  There is no CPU
// compute path in this library: every compute entry point needs a gfx950
// device and fails with MFSGD_ERR_NO_DEVICE otherwise.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>

#include "handle.hpp"
#include "jrandom.hpp"

namespace mfsgd {

thread_local std::string g_create_error;

int fail(const mfsgd_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

int hip_fail(const mfsgd_handle* h, const std::string& what, hipError_t e) {
    return fail(h, e == hipErrorOutOfMemory ? MFSGD_ERR_OOM : MFSGD_ERR_HIP, what + hipGetErrorString(e));
}

int serve_fail(const mfsgd_handle* h, const char* prefix, hipError_t e) {
    (void)hipGetLastError();
    return hip_fail(h, prefix, e);
}

int check_part(const mfsgd_handle* h, int32_t part, const char* name) {
    if (part < 0 || part >= h->n_parts) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(name) + ": bad partition");
    return MFSGD_OK;
}

int check_has_q(const mfsgd_handle* h, const char* call) {
    if (h->n_parts == 1 && h->where != mfsgd_handle::Where::None && !h->have_q)
        return fail(h, MFSGD_ERR_STATE,
                    std::string(call) + ": Q is not initialised: call mfsgd_init_factors or mfsgd_set_factors, or drive the "
                                        "handle with mfsgd_part_* and a caller-owned block");
    return MFSGD_OK;
}

int check_reads_factors(const mfsgd_handle* h, const char* call, bool reads_q) {
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, std::string(call) + ": single-partition handles only");
    if (h->where == mfsgd_handle::Where::None) return fail(h, MFSGD_ERR_STATE, std::string(call) + ": factors not initialised");
    return reads_q ? check_has_q(h, call) : MFSGD_OK;
}

static int usable_devices(int* count, std::string* why) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        *count = 0;
        if (why) *why = std::string("no HIP device visible (") + hipGetErrorString(e) + ")";
        return 0;
    }
    *count = n;
    return 0;
}

int ensure_device(mfsgd_handle* h) {
    if (h->device_ready) {
        HIPCHK(h, hipSetDevice(h->cfg.device));
        return MFSGD_OK;
    }
    int n = 0;
    std::string why;
    usable_devices(&n, &why);
    if (n <= 0) return fail(h, MFSGD_ERR_NO_DEVICE, "libmfsgd has no CPU fallback: " + why);
    if (h->cfg.device < 0 || h->cfg.device >= n)
        return fail(h, MFSGD_ERR_NO_DEVICE, "device ordinal " + std::to_string(h->cfg.device) +
                                                " out of range (" + std::to_string(n) + " visible)");
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, h->cfg.device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(h, MFSGD_ERR_NO_DEVICE,
                    std::string("device is ") + prop.gcnArchName + "; libmfsgd is built for gfx950 only");
    h->n_cu = prop.multiProcessorCount;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreate(&h->ev0));
    HIPCHK(h, hipEventCreate(&h->ev1));
    h->device_ready = true;
    return MFSGD_OK;
}

int dev_alloc(mfsgd_handle* h, DevBuf& b, size_t bytes) {
    const hipError_t e = b.alloc(bytes);
    if (e != hipSuccess) return hip_fail(h, "hipMalloc(&b.p, bytes): ", e);  // (the text this failure has always had)
    return MFSGD_OK;
}

// The device copies of the factors go away (re-seed, set_factors, load): nothing captured with the
// old pointers may be replayed, and nothing may still be running on them.
static void release_device_factors(mfsgd_handle* h) {
    if (h->where != mfsgd_handle::Where::Device) return;
    if (h->device_ready) {
        (void)hipSetDevice(h->cfg.device);
        (void)hipDeviceSynchronize();
    }
    for (Part& p : h->parts) p.drop_graphs();
    h->dP.reset();
    h->dQ.reset();
}

// factors host <-> device -------------------------------------------------------
// The staged rows of one side into a buffer of `capacity` rows (mfsgd_reserve_rows; the count where nothing is reserved,
// and then this is upload()).
static int upload_with_capacity(mfsgd_handle* h, DevArray<float>& b, const std::vector<float>& v, int32_t capacity) {
    int rc = dev_alloc(h, b, std::max(v.size(), (size_t)capacity * (size_t)h->geo.kp));
    if (rc) return rc;
    if (!v.empty()) HIPCHK(h, hipMemcpy(b.data(), v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return MFSGD_OK;
}

int factors_to_device(mfsgd_handle* h) {
    int rc = ensure_device(h);
    if (rc) return rc;
    if (h->where == mfsgd_handle::Where::Device) return MFSGD_OK;
    if (h->where == mfsgd_handle::Where::None)
        return fail(h, MFSGD_ERR_STATE, "factors not initialised: call mfsgd_init_factors or mfsgd_set_factors");
    if ((rc = upload_with_capacity(h, h->dP, h->hP, h->user_capacity()))) return rc;
    if (h->n_parts == 1 && (rc = upload_with_capacity(h, h->dQ, h->hQ, h->item_capacity()))) return rc;
    h->where = mfsgd_handle::Where::Device;
    std::vector<float>().swap(h->hP);
    std::vector<float>().swap(h->hQ);
    return MFSGD_OK;
}

static void fill_rows(JRandom& g, float* dst, int64_t rows, int k, int kp, float scale) {
    for (int64_t x = 0; x < rows; ++x) {
        float* row = dst + x * kp;
        for (int f = 0; f < k; ++f) row[f] = g.nextFloat() * scale;
        for (int f = k; f < kp; ++f) row[f] = 0.0f;
    }
}

// Seeds P (stream position of row u: (u_offset + u) * k) and, for single-partition handles with with_q, Q
// (row i: (n_users + i) * k).  On the device when there is one (a kernel per matrix; nothing crosses PCIe);
// on the host otherwise (host-only callers: the factors are uploaded when the first compute call comes).
static int seed_factors(mfsgd_handle* h, int64_t seed, int64_t u_offset, bool with_q) {
    const int k = h->cfg.k, kp = h->geo.kp;
    const float scale = (float)(1.0 / std::sqrt((double)k));
    release_device_factors(h);
    h->where = mfsgd_handle::Where::None;
    h->have_q = with_q;
    if (ensure_device(h) == MFSGD_OK) {
        int rc;
        if ((rc = dev_alloc(h, h->dP, (size_t)h->user_capacity() * kp))) return rc;
        HIPCHK(h, launch_init_rows(h->dP.data(), h->cfg.n_users, k, kp, seed, (unsigned long long)u_offset * (unsigned long long)k,
                                   scale, h->stream));
        if (with_q) {
            if ((rc = dev_alloc(h, h->dQ, (size_t)h->item_capacity() * kp))) return rc;
            HIPCHK(h, launch_init_rows(h->dQ.data(), h->cfg.n_items, k, kp, seed,
                                       (unsigned long long)h->cfg.n_users * (unsigned long long)k, scale, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<float>().swap(h->hP);
        std::vector<float>().swap(h->hQ);
        h->where = mfsgd_handle::Where::Device;
        return MFSGD_OK;
    }
    h->err.clear();  // no device: not an error for this call
    h->hP.assign((size_t)h->cfg.n_users * kp, 0.0f);
    JRandom g(seed);
    g.skip((uint64_t)u_offset * (uint64_t)k);
    fill_rows(g, h->hP.data(), h->cfg.n_users, k, kp, scale);
    h->hQ.clear();
    if (with_q) {
        h->hQ.assign((size_t)h->cfg.n_items * kp, 0.0f);
        JRandom gq(seed);
        gq.skip((uint64_t)h->cfg.n_users * (uint64_t)k);
        fill_rows(gq, h->hQ.data(), h->cfg.n_items, k, kp, scale);
    }
    h->where = mfsgd_handle::Where::Host;
    return MFSGD_OK;
}

// Growing a live model ("Growing a live model") -----------------------------------------------------------
// A buffer of new_rows rows that starts with the `rows` rows `old` holds: after a wait for the handle's stream, copied
// device to device on it (asynchronous: the caller synchronises before it lets go of `old`).  Allocated before anything
// is released, so a failure leaves the model as it was.
static int grown_copy(mfsgd_handle* h, const char* prefix, const DevArray<float>& old, int64_t rows, int64_t new_rows,
                      DevArray<float>& grown) {
    auto bad = [h, prefix](hipError_t e) { return serve_fail(h, prefix, e); };
    const size_t kp = (size_t)h->geo.kp;
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    if (const int rc = dev_alloc(h, grown, (size_t)new_rows * kp)) return rc;
    HIPCHK_OR(bad, hipMemcpyAsync(grown.data(), old.data(), sizeof(float) * (size_t)rows * kp, hipMemcpyDeviceToDevice, h->stream));
    return MFSGD_OK;
}

// The grown buffer takes the place of the old one: nothing runs on either (the caller has synchronised), and the
// training graphs, which hold the old pointer, go first.
static void adopt(mfsgd_handle* h, DevArray<float>& buf, DevArray<float>& grown) {
    for (Part& p : h->parts) p.drop_graphs();
    buf = std::move(grown);
}

// Dense rows of the caller's per staging buffer of an append: 32 MB
constexpr int64_t kAppendStageFloats = (int64_t)1 << 23;

// n_new rows (rows: n_new x k dense, or null: seeded) behind the `count` rows at dst_base, on the handle's stream; the
// caller's rows go up in pieces through a staging buffer that is gone when this returns.
static int write_new_rows(mfsgd_handle* h, const char* prefix, float* dst_base, int64_t count, int32_t n_new, const float* rows,
                          int64_t seed) {
    auto bad = [h, prefix](hipError_t e) { return serve_fail(h, prefix, e); };
    const int k = h->cfg.k, kp = h->geo.kp;
    float* dst = dst_base + (size_t)count * kp;
    if (!rows) {
        HIPCHK_OR(bad, launch_init_rows(dst, n_new, k, kp, seed, 0, (float)(1.0 / std::sqrt((double)k)), h->stream));
        return MFSGD_OK;
    }
    const int64_t piece = std::min<int64_t>(n_new, std::max<int64_t>(1, kAppendStageFloats / k));
    DevArray<float> stage;
    if (const int rc = dev_alloc(h, stage, (size_t)piece * k)) return rc;
    for (int64_t x0 = 0; x0 < n_new; x0 += piece) {
        const int64_t nb = std::min<int64_t>(piece, n_new - x0);
        HIPCHK_OR(bad, copy_up(stage, rows + x0 * k, (size_t)nb * k, h->stream));
        HIPCHK_OR(bad, launch_place_rows(dst + (size_t)x0 * kp, stage.data(), nb, k, kp, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // the staging buffer is reused, and freed on return
    }
    return MFSGD_OK;
}

// Body of mfsgd_append_users / mfsgd_append_items.
static int append_rows(mfsgd_handle* h, bool items, const char* name, int32_t n_new, const float* rows, int64_t seed,
                       int32_t* first) {
    const std::string call = std::string(name) + ": ";
    int32_t& count = items ? h->cfg.n_items : h->cfg.n_users;
    if (n_new < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_new is negative");
    if ((int64_t)count + n_new > (int64_t)INT32_MAX)
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "the number of " + (items ? "items" : "users") + " would exceed INT32_MAX");
    if (const int rc = check_reads_factors(h, name)) return rc;
    if (first) *first = count;
    if (n_new == 0) return MFSGD_OK;
    const int k = h->cfg.k, kp = h->geo.kp;
    const int64_t need = (int64_t)count + n_new;
    std::vector<int32_t>& last = items ? h->online_last_i : h->online_last_u;
    if (!last.empty()) last.reserve((size_t)need);  // (what can fail comes before anything changes)
    // users beyond the capacity: the per-user tables of the seen-item index grow with it, new before old as the rows do
    DevArray<long long> seen_off;
    DevArray<int32_t> seen_slot;
    if (!items && need > h->user_capacity()) {
        if (const int rc = seen_grown_tables(h, call.c_str(), (int32_t)need, seen_off, seen_slot)) return rc;
    }
    if (h->where == mfsgd_handle::Where::Host) {
        std::vector<float>& v = items ? h->hQ : h->hP;
        const size_t old = v.size();
        v.resize(old + (size_t)n_new * kp, 0.0f);
        if (rows) {
            for (int64_t x = 0; x < n_new; ++x)
                for (int f = 0; f < k; ++f) v[old + (size_t)x * kp + f] = canon_nan(rows[x * k + f]);
        } else {
            JRandom g(seed);
            fill_rows(g, v.data() + old, n_new, k, kp, (float)(1.0 / std::sqrt((double)k)));
        }
    } else {
        int rc = ensure_device(h);
        if (rc) return rc;
        auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
        DevArray<float>& buf = items ? h->dQ : h->dP;
        DevArray<float> grown;  // beyond the capacity: to exactly what is needed (the capacity is at least the reserve)
        if (need > (items ? h->item_capacity() : h->user_capacity()) && (rc = grown_copy(h, call.c_str(), buf, count, need, grown)))
            return rc;
        if ((rc = write_new_rows(h, call.c_str(), grown ? grown.data() : buf.data(), count, n_new, rows, seed))) return rc;
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
        if (grown) adopt(h, buf, grown);
    }
    if (seen_off) {
        (void)hipStreamSynchronize(h->stream);
        seen_adopt_tables(h, (int32_t)need, seen_off, seen_slot);
    }
    count = (int32_t)need;
    if (items && !h->parts.empty()) h->parts[0].q_rows = count;
    if (!last.empty()) last.resize((size_t)need, 0);
    return MFSGD_OK;
}

}  // namespace mfsgd

using namespace mfsgd;

// =============================================================================
extern "C" {

int mfsgd_abi_version(void) { return MFSGD_ABI_VERSION; }

int mfsgd_device_count(int32_t* out) {
    if (!out) return MFSGD_ERR_INVALID_ARG;
    return guarded_free(nullptr, [&]() -> int {
        int n = 0;
        usable_devices(&n, nullptr);
        int ok = 0;
        for (int d = 0; d < n; ++d) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
        }
        *out = ok;
        return MFSGD_OK;
    });
}

int mfsgd_create(const mfsgd_config* cfg, mfsgd_handle** out) {
    if (out) *out = nullptr;
    return guarded_free("mfsgd_create", [&]() -> int {
        auto bad = [&](const char* m, int code = MFSGD_ERR_INVALID_ARG) {
            g_create_error = std::string("mfsgd_create: ") + m;
            return code;
        };
        if (!cfg || !out) return bad("null argument");
        if (cfg->n_users < 1 || cfg->n_items < 1) return bad("n_users and n_items must be >= 1");
        if (cfg->k < 1) return bad("k must be >= 1");
        if (cfg->k > MFSGD_MAX_K) return bad("k exceeds MFSGD_MAX_K (256)", MFSGD_ERR_UNSUPPORTED);
        if (!(cfg->lr == cfg->lr) || !(cfg->lambda == cfg->lambda)) return bad("lr / lambda is NaN");
        if (cfg->blocks < 0 || cfg->waves < 0 || cfg->n_parts < 0 || cfg->device < 0 || cfg->host_threads < 0)
            return bad("negative geometry field");
        if (cfg->waves != 0 && cfg->waves != 1 && cfg->waves != 2 && cfg->waves != 4 && cfg->waves != 8)
            return bad("waves must be 0 (auto), 1, 2, 4 or 8");
        for (int x = 0; x < 5; ++x)
            if (cfg->reserved[x] != 0) return bad("reserved fields must be zero");
        auto h = std::make_unique<mfsgd_handle>();
        h->cfg = *cfg;
        h->geo = geometry_for_k(cfg->k);
        h->n_parts = cfg->n_parts > 1 ? cfg->n_parts : 1;
        if (h->n_parts > cfg->n_items) return bad("n_parts exceeds n_items");
        if (h->n_parts > 1) default_item_map(h.get());
        *out = h.release();
        return MFSGD_OK;
    });
}

void mfsgd_destroy(mfsgd_handle* h) {
    if (!h) return;
    if (h->device_ready) {
        (void)hipSetDevice(h->cfg.device);
        (void)hipStreamSynchronize(h->stream);
    }
    h->parts.clear();
    h->dP.reset();
    h->dQ.reset();
    h->val = Validation{};
    h->seen = Seen{};
    h->weights = ItemWeights{};
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->side_stream) {
        (void)hipStreamSynchronize(h->side_stream);
        if (h->occupy_started) (void)hipHostFree(h->occupy_started);
        h->occupy_started = nullptr;
        (void)hipStreamDestroy(h->side_stream);
    }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

const char* mfsgd_last_error(const mfsgd_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int mfsgd_get_dims(const mfsgd_handle* h, int32_t* n_users, int32_t* n_items, int32_t* k) {
    if (!h) return MFSGD_ERR_INVALID_ARG;
    if (n_users) *n_users = h->cfg.n_users;
    if (n_items) *n_items = h->cfg.n_items;
    if (k) *k = h->cfg.k;
    return MFSGD_OK;
}

int mfsgd_get_parts(const mfsgd_handle* h, int32_t* n_parts, int32_t* kp, int32_t* device) {
    if (!h) return MFSGD_ERR_INVALID_ARG;
    if (n_parts) *n_parts = h->n_parts;
    if (kp) *kp = h->geo.kp;
    if (device) *device = h->cfg.device;
    return MFSGD_OK;
}

int mfsgd_init_p_offset(mfsgd_handle* h, int64_t seed, int64_t u_offset) {
    return guarded(h, "init_p_offset", [&]() -> int {
        if (u_offset < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "init_p_offset: bad argument");
        return seed_factors(h, seed, u_offset, false);
    });
}

int mfsgd_init_factors(mfsgd_handle* h, int64_t seed) {
    return guarded(h, "init_factors", [&]() -> int {
        return seed_factors(h, seed, 0, h->n_parts == 1);  // n_parts > 1: Q lives in caller-owned blocks
    });
}

int mfsgd_set_factors(mfsgd_handle* h, const float* P, const float* Q) {
    return guarded(h, "set_factors", [&]() -> int {
        if (!P) return fail(h, MFSGD_ERR_INVALID_ARG, "set_factors: P is null");
        if (h->n_parts == 1 && !Q) return fail(h, MFSGD_ERR_INVALID_ARG, "set_factors: Q is null");
        const int k = h->cfg.k, kp = h->geo.kp;
        release_device_factors(h);
        h->hP.assign((size_t)h->cfg.n_users * kp, 0.0f);
        for (int64_t x = 0; x < h->cfg.n_users; ++x) std::memcpy(&h->hP[(size_t)x * kp], P + x * k, sizeof(float) * (size_t)k);
        h->hQ.clear();
        if (h->n_parts == 1) {
            h->hQ.assign((size_t)h->cfg.n_items * kp, 0.0f);
            for (int64_t x = 0; x < h->cfg.n_items; ++x) std::memcpy(&h->hQ[(size_t)x * kp], Q + x * k, sizeof(float) * (size_t)k);
        }
        for (float& x : h->hP) x = canon_nan(x);  // (records.hpp: no NaN keeps a payload of the caller's)
        for (float& x : h->hQ) x = canon_nan(x);
        h->have_q = h->n_parts == 1;
        h->where = mfsgd_handle::Where::Host;
        return MFSGD_OK;
    });
}

int mfsgd_get_factors(mfsgd_handle* h, float* P, float* Q) {
    return guarded(h, "get_factors", [&]() -> int {
        if (h->where == mfsgd_handle::Where::None) return fail(h, MFSGD_ERR_STATE, "get_factors: factors not initialised");
        if (Q)
            if (const int rc = check_has_q(h, "get_factors")) return rc;  // (before P is touched: an error writes nothing)
        const int k = h->cfg.k, kp = h->geo.kp;
        const std::vector<float>*sp = &h->hP, *sq = &h->hQ;
        std::vector<float> tp, tq;
        if (h->where == mfsgd_handle::Where::Device) {
            HIPCHK(h, hipSetDevice(h->cfg.device));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if (P) {
                tp.resize((size_t)h->cfg.n_users * kp);
                HIPCHK(h, hipMemcpy(tp.data(), h->dP.data(), tp.size() * sizeof(float), hipMemcpyDeviceToHost));
            }
            if (Q && h->n_parts == 1) {
                tq.resize((size_t)h->cfg.n_items * kp);
                HIPCHK(h, hipMemcpy(tq.data(), h->dQ.data(), tq.size() * sizeof(float), hipMemcpyDeviceToHost));
            }
            sp = &tp;
            sq = &tq;
        }
        if (P)
            for (int64_t x = 0; x < h->cfg.n_users; ++x) std::memcpy(P + x * k, &(*sp)[(size_t)x * kp], sizeof(float) * (size_t)k);
        if (Q) {
            if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "get_factors: Q lives in caller-owned blocks when n_parts > 1");
            for (int64_t x = 0; x < h->cfg.n_items; ++x) std::memcpy(Q + x * k, &(*sq)[(size_t)x * kp], sizeof(float) * (size_t)k);
        }
        return MFSGD_OK;
    });
}

int mfsgd_append_users(mfsgd_handle* h, int32_t n_new, const float* rows, int64_t seed, int32_t* first) {
    return guarded(h, "append_users", [&]() -> int { return append_rows(h, false, "append_users", n_new, rows, seed, first); });
}

int mfsgd_append_items(mfsgd_handle* h, int32_t n_new, const float* rows, int64_t seed, int32_t* first) {
    return guarded(h, "append_items", [&]() -> int { return append_rows(h, true, "append_items", n_new, rows, seed, first); });
}

int mfsgd_reserve_rows(mfsgd_handle* h, int32_t user_capacity, int32_t item_capacity) {
    return guarded(h, "reserve_rows", [&]() -> int {
        if (user_capacity < 0 || item_capacity < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "reserve_rows: a capacity is negative");
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "reserve_rows: single-partition handles only");
        // with the factors on the device a larger capacity is a larger buffer now; before that it is a number
        // factors_to_device and seed_factors read
        struct Side {
            DevArray<float>& buf;
            int32_t count, capacity, want;
            int32_t& reserved;
        } sides[2] = {{h->dP, h->cfg.n_users, h->user_capacity(), user_capacity, h->reserved_users},
                      {h->dQ, h->cfg.n_items, h->item_capacity(), item_capacity, h->reserved_items}};
        for (Side& s : sides) {
            if (s.want <= s.capacity) continue;
            DevArray<long long> seen_off;  // the users' side: the tables of the seen-item index grow too
            DevArray<int32_t> seen_slot;
            if (&s == &sides[0]) {
                if (const int rc = seen_grown_tables(h, "reserve_rows: ", s.want, seen_off, seen_slot)) return rc;
                if (seen_off) {
                    const hipError_t e = hipStreamSynchronize(h->stream);
                    if (e != hipSuccess) return serve_fail(h, "reserve_rows: ", e);
                }
            }
            if (h->where == mfsgd_handle::Where::Device && s.buf) {
                int rc = ensure_device(h);
                if (rc) return rc;
                DevArray<float> grown;
                if ((rc = grown_copy(h, "reserve_rows: ", s.buf, s.count, s.want, grown))) return rc;
                const hipError_t e = hipStreamSynchronize(h->stream);
                if (e != hipSuccess) return serve_fail(h, "reserve_rows: ", e);
                adopt(h, s.buf, grown);
            }
            seen_adopt_tables(h, s.want, seen_off, seen_slot);
            s.reserved = s.want;
        }
        return MFSGD_OK;
    });
}

int mfsgd_get_capacity(const mfsgd_handle* h, int32_t* users, int32_t* items) {
    return guarded(h, "get_capacity", [&]() -> int {
        if (users) *users = h->user_capacity();
        if (items) *items = h->item_capacity();
        return MFSGD_OK;
    });
}

// ---- the seen-item index (seen_index.cpp) ----
int mfsgd_set_seen(mfsgd_handle* h, const int32_t* u, const int32_t* i, int64_t n) {
    return guarded(h, "set_seen", [&]() -> int { return seen_update(h, "set_seen", false, u, i, n); });
}

int mfsgd_mark_seen(mfsgd_handle* h, const int32_t* u, const int32_t* i, int64_t n) {
    return guarded(h, "mark_seen", [&]() -> int { return seen_update(h, "mark_seen", true, u, i, n); });
}

int mfsgd_clear_seen(mfsgd_handle* h) {
    return guarded(h, "clear_seen", [&]() -> int {
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "clear_seen: single-partition handles only");
        if (h->device_ready) {
            (void)hipSetDevice(h->cfg.device);
            (void)hipStreamSynchronize(h->stream);
        }
        h->seen = Seen{};
        return MFSGD_OK;
    });
}

int mfsgd_seen_size(const mfsgd_handle* h, int64_t* pairs) {
    return guarded(h, "seen_size", [&]() -> int {
        if (!pairs) return fail(h, MFSGD_ERR_INVALID_ARG, "seen_size: pairs is null");
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "seen_size: single-partition handles only");
        *pairs = h->seen.present ? h->seen.n : -1;
        return MFSGD_OK;
    });
}

int mfsgd_get_seen(mfsgd_handle* h, const int32_t* users, int32_t n_users, int64_t* row_ptr, int32_t* items,
                   int64_t items_capacity) {
    return guarded(h, "get_seen", [&]() -> int { return seen_get(h, users, n_users, row_ptr, items, items_capacity); });
}

int mfsgd_sample_unseen(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                        int32_t* out_items) {
    return guarded(h, "sample_unseen", [&]() -> int { return seen_sample(h, users, n, m, seed, first, out_items); });
}

// ---- item weights and the weighted draw (seen_index.cpp) ----
int mfsgd_set_item_weights(mfsgd_handle* h, const uint32_t* w, int32_t n) {
    return guarded(h, "set_item_weights", [&]() -> int { return weights_set(h, w, n); });
}

int mfsgd_get_item_weights(mfsgd_handle* h, uint32_t* w, int32_t* n) {
    return guarded(h, "get_item_weights", [&]() -> int { return weights_get(h, w, n); });
}

int mfsgd_clear_item_weights(mfsgd_handle* h) {
    return guarded(h, "clear_item_weights", [&]() -> int { return weights_clear(h); });
}

int mfsgd_seen_item_counts(mfsgd_handle* h, int64_t* counts) {
    return guarded(h, "seen_item_counts", [&]() -> int { return seen_item_histogram(h, counts); });
}

int mfsgd_sample_unseen_weighted(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                                 int32_t* out_items, int64_t* out_mass) {
    return guarded(h, "sample_unseen_weighted", [&]() -> int {
        return seen_sample_weighted(h, users, n, m, seed, first, out_items, out_mass);
    });
}

int mfsgd_sample_unseen_hard(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                             int32_t* out_items, float* out_scores, int32_t* out_draw) {
    return guarded(h, "sample_unseen_hard", [&]() -> int {
        return seen_sample_hard(h, users, n, m, seed, first, out_items, out_scores, out_draw);
    });
}

int mfsgd_sample_unseen_violating(mfsgd_handle* h, const int32_t* users, const int32_t* pos_items, int64_t n, int32_t m,
                                  float margin, int64_t seed, int64_t first, int32_t* out_items, int32_t* out_draw,
                                  float* out_margin, int32_t* out_rank) {
    return guarded(h, "sample_unseen_violating", [&]() -> int {
        return seen_sample_violating(h, users, pos_items, n, m, margin, seed, first, out_items, out_draw, out_margin, out_rank);
    });
}

int mfsgd_sample_unseen_hard_weighted(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                                      int32_t* out_items, float* out_scores, int32_t* out_draw, int64_t* out_mass) {
    return guarded(h, "sample_unseen_hard_weighted", [&]() -> int {
        return seen_sample_hard_weighted(h, users, n, m, seed, first, out_items, out_scores, out_draw, out_mass);
    });
}

int mfsgd_sample_unseen_violating_weighted(mfsgd_handle* h, const int32_t* users, const int32_t* pos_items, int64_t n, int32_t m,
                                           float margin, int64_t seed, int64_t first, int32_t* out_items, int32_t* out_draw,
                                           float* out_margin, int32_t* out_rank, int64_t* out_mass) {
    return guarded(h, "sample_unseen_violating_weighted", [&]() -> int {
        return seen_sample_violating_weighted(h, users, pos_items, n, m, margin, seed, first, out_items, out_draw, out_margin,
                                              out_rank, out_mass);
    });
}

int mfsgd_debug_device_bytes(int64_t* live) {
    if (!live) return MFSGD_ERR_INVALID_ARG;
    *live = g_dev_live_bytes.load();
    return MFSGD_OK;
}

}  // extern "C"
