// online_update.cpp -- online updates of the live factors ("Online updates"): the dependency levels of a list
// of fresh ratings, the launch policy over them, and the two calls, mfsgd_online_levels and mfsgd_apply_ratings.  The
// kernel is online.hip's.  The pairwise (BPR) update of a list of triples ("Pairwise ranking (BPR)") is the
// same code with a third row per step: mfsgd_triple_levels, mfsgd_apply_triples (kernel: pairwise.hip) and the host's
// view of its logistic weight, mfsgd_bpr_weights.  mfsgd_apply_triples_weighted is mfsgd_apply_triples with the step size
// of every triple given by the caller, and mfsgd_warp_weights the host's table of the WARP weight ("WARP").
#include <algorithm>

#include "canon.hpp"
#include "handle.hpp"
#include "serve_util.hpp"

namespace mfsgd {

// Ratings of one piece: the pieces of a list are consecutive and applied one after the other, so the levels are those of
// a piece, and the device buffers of a call are sized by one.  (include/mfsgd.h states the size.)
constexpr int64_t kOnlinePiece = (int64_t)1 << 20;
// Consecutive narrow levels one workgroup walks in one launch: bounds the time a single launch runs.
constexpr int32_t kOnlineRun = 1 << 16;

static int check_online_pairs(const mfsgd_handle* h, const char* call, const int32_t* u, const int32_t* i, int64_t n) {
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": n is negative");
    if (n > 0 && (!u || !i)) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": u or i is null");
    const int64_t j = first_outside(u, h->cfg.n_users, i, h->cfg.n_items, n);
    if (j >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": rating " + std::to_string(j) + " out of range");
    return MFSGD_OK;
}

// The same for triples (u, i, i2), i2 being the negative item; i[x] == i2[x] is refused on top (the message names the triple).
// With weights (mfsgd_apply_triples_weighted), w is one of the arrays that must be there.
static int check_online_triples(const mfsgd_handle* h, const char* call, const int32_t* u, const int32_t* i, const int32_t* i2,
                                int64_t n, bool weighted = false, const float* w = nullptr) {
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": n is negative");
    if (n > 0 && (!u || !i || !i2 || (weighted && !w)))
        return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + (weighted ? ": u, i, j or w is null" : ": u, i or j is null"));
    const uint32_t U = (uint32_t)h->cfg.n_users, I = (uint32_t)h->cfg.n_items;
    int64_t x = first_where(n, [=](int64_t t) {
        return (uint32_t)((uint32_t)u[t] >= U) | (uint32_t)((uint32_t)i[t] >= I) | (uint32_t)((uint32_t)i2[t] >= I);
    });
    if (x >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": triple " + std::to_string(x) + " out of range");
    x = first_where(n, [=](int64_t t) { return (uint32_t)(i[t] == i2[t]); });
    if (x >= 0)
        return fail(h, MFSGD_ERR_INVALID_ARG, std::string(call) + ": triple " + std::to_string(x) + " has the same positive and negative item");
    return MFSGD_OK;
}

// level[j] of the n ratings of one piece (every index in range), and how many levels there are: one pass, and a second
// one that puts the handle's two "last level" arrays back to zero -- O(n), whatever n_users and n_items are.
// i2 (nullable): a second item per step, for triples -- a row of Q like the first, so both go through the item array.
static int32_t online_levels_of(mfsgd_handle* h, const int32_t* u, const int32_t* i, int64_t n, int32_t* level,
                                const int32_t* i2 = nullptr) {
    if (h->online_last_u.empty()) h->online_last_u.assign((size_t)h->cfg.n_users, 0);
    if (h->online_last_i.empty()) h->online_last_i.assign((size_t)h->cfg.n_items, 0);
    int32_t* lu = h->online_last_u.data();
    int32_t* li = h->online_last_i.data();
    int32_t n_levels = 0;
    for (int64_t j = 0; j < n; ++j) {
        int32_t l = std::max(lu[u[j]], li[i[j]]);
        if (i2) l = std::max(l, li[i2[j]]);
        level[j] = l;
        lu[u[j]] = li[i[j]] = l + 1;
        if (i2) li[i2[j]] = l + 1;
        n_levels = std::max(n_levels, l + 1);
    }
    for (int64_t j = 0; j < n; ++j) lu[u[j]] = li[i[j]] = 0;
    if (i2)
        for (int64_t j = 0; j < n; ++j) li[i2[j]] = 0;
    return n_levels;
}

// One piece ready for the device: its ratings in a stable counting sort by level.  A piece of triples has i2, the
// negative items, in the place of r, and with them w, the weights of a weighted call (else empty).
struct OnlinePiece {
    std::vector<int32_t> level, level_ptr, u, i, i2, orig;
    std::vector<float> r, w;
    int32_t n_levels = 0;
};

// Exactly one of r and i2 is given; w (nullable) only with i2.
static void online_sort_piece(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, const int32_t* i2, const float* w,
                              int64_t n, OnlinePiece& pc) {
    pc.level.resize((size_t)n);
    pc.u.resize((size_t)n), pc.i.resize((size_t)n), pc.orig.resize((size_t)n);
    if (r) pc.r.resize((size_t)n);
    else pc.i2.resize((size_t)n);
    pc.w.resize(w ? (size_t)n : 0);
    pc.n_levels = online_levels_of(h, u, i, n, pc.level.data(), i2);
    pc.level_ptr.assign((size_t)pc.n_levels + 1, 0);
    for (int64_t j = 0; j < n; ++j) ++pc.level_ptr[(size_t)pc.level[(size_t)j] + 1];
    for (int32_t l = 0; l < pc.n_levels; ++l) pc.level_ptr[(size_t)l + 1] += pc.level_ptr[(size_t)l];
    std::vector<int32_t> next(pc.level_ptr.begin(), pc.level_ptr.end() - 1);
    for (int64_t j = 0; j < n; ++j) {
        const int32_t at = next[(size_t)pc.level[(size_t)j]]++;
        pc.u[(size_t)at] = u[j];
        pc.i[(size_t)at] = i[j];
        if (r) pc.r[(size_t)at] = canon_nan(r[j]);  // (records.hpp: a payload must not reach P and Q)
        else pc.i2[(size_t)at] = i2[j];
        if (w) pc.w[(size_t)at] = canon_nan(w[j]);  // (the same: lr * w is the step size of three rows)
        pc.orig[(size_t)at] = (int32_t)j;
    }
}

static void online_count(mfsgd_online_info* info, const int32_t* level_ptr, int32_t n_levels) {
    info->pieces += 1;
    info->levels += n_levels;
    for (int32_t l = 0; l < n_levels; ++l) info->max_width = std::max<int64_t>(info->max_width, level_ptr[l + 1] - level_ptr[l]);
}

// The launches of one piece that is on the device.  A wide level (more ratings than one pass of one workgroup holds) is a
// launch of its own, of as many workgroups as it has passes: stream order is the barrier before and behind it.  A run of
// consecutive narrow levels is ONE launch of ONE workgroup, which walks them (online.hip).  (Narrow is one pass, not a few:
// calling levels of up to 4, 8 or 16 passes narrow saved launches and no time on the bench workload, 32 passes cost four
// times the time -- DESIGN.md, "Online updates".)
template <class Launch>
static hipError_t online_launches(const std::vector<int32_t>& level_ptr, int32_t n_levels, int L, int64_t* launches, Launch&& launch) {
    const int32_t gpb = 256 / L;
    for (int32_t l = 0; l < n_levels;) {
        const int32_t width = level_ptr[(size_t)l + 1] - level_ptr[(size_t)l];
        int32_t l1 = l + 1, wgs = 1;
        if (width > gpb) {
            wgs = (width + gpb - 1) / gpb;
        } else {
            while (l1 < n_levels && l1 - l < kOnlineRun && level_ptr[(size_t)l1 + 1] - level_ptr[(size_t)l1] <= gpb) ++l1;
        }
        const hipError_t e = launch(l, l1, wgs);
        if (e != hipSuccess) return e;
        ++*launches;
        l = l1;
    }
    return hipSuccess;
}

// Body of mfsgd_online_levels (i2 == nullptr) and mfsgd_triple_levels behind their checks: the levels piece by piece.
static void levels_of_list(mfsgd_handle* h, const int32_t* u, const int32_t* i, const int32_t* i2, int64_t n, int32_t* level,
                           mfsgd_online_info* info) {
    mfsgd_online_info got{};
    got.n = n;
    std::vector<int32_t> own, count;
    if (!level && n > 0) own.resize((size_t)std::min(n, kOnlinePiece));
    for (int64_t j0 = 0; j0 < n; j0 += kOnlinePiece) {
        const int64_t c = std::min(kOnlinePiece, n - j0);
        int32_t* lv = level ? level + j0 : own.data();
        const int32_t n_levels = online_levels_of(h, u + j0, i + j0, c, lv, i2 ? i2 + j0 : nullptr);
        count.assign((size_t)n_levels + 1, 0);  // (as a level_ptr: entry l + 1 counts level l)
        for (int64_t j = 0; j < c; ++j) ++count[(size_t)lv[j] + 1];
        for (int32_t l = 0; l < n_levels; ++l) count[(size_t)l + 1] += count[(size_t)l];
        online_count(&got, count.data(), n_levels);
    }
    if (info) *info = got;
}

// Body of mfsgd_apply_ratings (r given), mfsgd_apply_triples (i2 given) and mfsgd_apply_triples_weighted (i2 and w given)
// behind their argument checks: piece by piece, the sort, the uploads, the launches of online.hip's or pairwise.hip's
// kernel, and out (nullable, n floats: the errors or the margins) coming down.
static int apply_list(mfsgd_handle* h, const char* call, const int32_t* u, const int32_t* i, const float* r, const int32_t* i2,
                      const float* w, int64_t n, float* out, mfsgd_online_info* info) {
    int rc = check_reads_factors(h, call);
    if (rc) return rc;
    mfsgd_online_info got{};
    got.n = n;
    if (n == 0) {
        if (info) *info = got;
        return MFSGD_OK;
    }
    if ((rc = factors_to_device(h))) return rc;
    const std::string prefix = std::string(call) + ": ";
    auto bad = [&](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    const size_t piece = (size_t)std::min(n, kOnlinePiece);
    DevArray<int32_t> du, di, di2, dorig, dptr;  // sized by the largest piece; gone when this returns, whichever way
    DevArray<float> dr, dw, dout;
    if ((rc = dev_alloc(h, du, piece)) || (rc = dev_alloc(h, di, piece))) return rc;
    if ((rc = r ? dev_alloc(h, dr, piece) : dev_alloc(h, di2, piece)) || (rc = dev_alloc(h, dorig, piece))) return rc;
    if ((rc = dev_alloc(h, dptr, piece + 1))) return rc;
    if (w && (rc = dev_alloc(h, dw, piece))) return rc;
    if (out && (rc = dev_alloc(h, dout, piece))) return rc;
    const float lr = h->cfg.lr, c1 = 1.0f - h->cfg.lr * h->cfg.lambda;
    OnlinePiece pc;
    for (int64_t j0 = 0; j0 < n; j0 += kOnlinePiece) {
        const size_t c = (size_t)std::min(kOnlinePiece, n - j0);
        online_sort_piece(h, u + j0, i + j0, r ? r + j0 : nullptr, i2 ? i2 + j0 : nullptr, w ? w + j0 : nullptr, (int64_t)c, pc);
        online_count(&got, pc.level_ptr.data(), pc.n_levels);
        HIPCHK_OR(bad, copy_up(du, pc.u.data(), c, h->stream));
        HIPCHK_OR(bad, copy_up(di, pc.i.data(), c, h->stream));
        HIPCHK_OR(bad, r ? copy_up(dr, pc.r.data(), c, h->stream) : copy_up(di2, pc.i2.data(), c, h->stream));
        if (w) HIPCHK_OR(bad, copy_up(dw, pc.w.data(), c, h->stream));
        HIPCHK_OR(bad, copy_up(dorig, pc.orig.data(), c, h->stream));
        HIPCHK_OR(bad, copy_up(dptr, pc.level_ptr.data(), (size_t)pc.n_levels + 1, h->stream));
        HIPCHK_OR(bad, online_launches(pc.level_ptr, pc.n_levels, h->geo.L, &got.launches, [&](int32_t l0, int32_t l1, int32_t wgs) {
            if (r)
                return launch_apply_levels(h->geo.L, h->dP.data(), h->dQ.data(), du.data(), di.data(), dr.data(), dorig.data(),
                                           dptr.data(), l0, l1, wgs, h->cfg.k, lr, c1, dout.data(), h->stream);
            return launch_apply_triple_levels(h->geo.L, h->dP.data(), h->dQ.data(), du.data(), di.data(), di2.data(), dw.data(),
                                              dorig.data(), dptr.data(), l0, l1, wgs, h->cfg.k, lr, c1, dout.data(), h->stream);
        }));
        if (out) HIPCHK_OR(bad, copy_down(out + j0, dout, c, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // the staging buffers, the host's and the device's, are reused
    }
    if (info) *info = got;
    return MFSGD_OK;
}

}  // namespace mfsgd

using namespace mfsgd;

extern "C" {

int mfsgd_online_levels(mfsgd_handle* h, const int32_t* u, const int32_t* i, int64_t n, int32_t* level, mfsgd_online_info* info) {
    return guarded(h, "online_levels", [&]() -> int {
        if (const int rc = check_online_pairs(h, "online_levels", u, i, n)) return rc;
        levels_of_list(h, u, i, nullptr, n, level, info);
        return MFSGD_OK;
    });
}

int mfsgd_triple_levels(mfsgd_handle* h, const int32_t* u, const int32_t* i, const int32_t* j, int64_t n, int32_t* level,
                        mfsgd_online_info* info) {
    return guarded(h, "triple_levels", [&]() -> int {
        if (const int rc = check_online_triples(h, "triple_levels", u, i, j, n)) return rc;
        levels_of_list(h, u, i, j, n, level, info);
        return MFSGD_OK;
    });
}

int mfsgd_apply_ratings(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, int64_t n, float* err,
                        mfsgd_online_info* info) {
    return guarded(h, "apply_ratings", [&]() -> int {
        if (const int rc = check_online_pairs(h, "apply_ratings", u, i, n)) return rc;
        if (n > 0 && !r) return fail(h, MFSGD_ERR_INVALID_ARG, "apply_ratings: r is null");
        return apply_list(h, "apply_ratings", u, i, r, nullptr, nullptr, n, err, info);
    });
}

int mfsgd_apply_triples(mfsgd_handle* h, const int32_t* u, const int32_t* i, const int32_t* j, int64_t n, float* margin,
                        mfsgd_online_info* info) {
    return guarded(h, "apply_triples", [&]() -> int {
        if (const int rc = check_online_triples(h, "apply_triples", u, i, j, n)) return rc;
        return apply_list(h, "apply_triples", u, i, nullptr, j, nullptr, n, margin, info);
    });
}

int mfsgd_apply_triples_weighted(mfsgd_handle* h, const int32_t* u, const int32_t* i, const int32_t* j, const float* w, int64_t n,
                                 float* margin, mfsgd_online_info* info) {
    return guarded(h, "apply_triples_weighted", [&]() -> int {
        if (const int rc = check_online_triples(h, "apply_triples_weighted", u, i, j, n, true, w)) return rc;
        return apply_list(h, "apply_triples_weighted", u, i, nullptr, j, w, n, margin, info);
    });
}

int mfsgd_bpr_weights(const float* x, float* g, int64_t n) {
    return guarded_free("bpr_weights", [&]() -> int {
        if (n < 0 || (n > 0 && (!x || !g))) {
            g_create_error = n < 0 ? "bpr_weights: n is negative" : "bpr_weights: x or g is null";
            return MFSGD_ERR_INVALID_ARG;
        }
        for (int64_t a = 0; a < n; ++a) g[a] = lsig(x[a]);
        return MFSGD_OK;
    });
}

int mfsgd_warp_weights(const int32_t* rank, float* w, int64_t n) {
    return guarded_free("warp_weights", [&]() -> int {
        if (n < 0 || (n > 0 && (!rank || !w))) {
            g_create_error = n < 0 ? "warp_weights: n is negative" : "warp_weights: rank or w is null";
            return MFSGD_ERR_INVALID_ARG;
        }
        int32_t top = 0;
        for (int64_t a = 0; a < n; ++a) {
            if (rank[a] < 0) {
                g_create_error = "warp_weights: rank " + std::to_string(a) + " is negative";
                return MFSGD_ERR_INVALID_ARG;
            }
            top = std::max(top, rank[a]);
        }
        // L(r) for r = 0 .. top, once: the fp64 sum 1/1 + 1/2 + ... + 1/r in ascending order, rounded to fp32 once
        std::vector<float> table((size_t)top + 1);
        double sum = 0.0;
        table[0] = 0.0f;
        for (int64_t r = 1; r <= top; ++r) {
            sum += 1.0 / (double)r;
            table[(size_t)r] = (float)sum;
        }
        for (int64_t a = 0; a < n; ++a) w[a] = table[(size_t)rank[a]];
        return MFSGD_OK;
    });
}

}  // extern "C"
