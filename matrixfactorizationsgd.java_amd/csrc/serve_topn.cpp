// serve_topn.cpp -- predictions and the top-N side of what a trained model answers: recommendations for users and for
// items, among all rows or among candidates, and the cosine neighbours of items and users.  Every call batches its work
// through bounded staging buffers.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>

#include "serve_lists.hpp"

namespace mfsgd {

constexpr ServeName kRecommend{"recommend", "the requested users"};
constexpr ServeName kAmong{"recommend_among", "the requested users"}, kRowsAmong{"recommend_rows_among", "the rows"};
// ... and the calls that exclude what the handle's seen-item index holds instead of a pair list
constexpr ServeName kUnseen{"recommend_unseen", "the requested users"}, kUnseenAmong{"recommend_unseen_among", "the requested users"};
// ... and the item-side calls: the request rows are items (or item rows of the caller's), the users are scanned
constexpr ServeName kUsers{"recommend_users", "the requested items", "item", "users"};
constexpr ServeName kUsersAmong{"recommend_users_among", "the requested items", "item", "users"};
constexpr ServeName kUsersUnseen{"recommend_users_unseen", "the requested items", "item", "users"};
constexpr ServeName kUsersUnseenAmong{"recommend_users_unseen_among", "the requested items", "item", "users"};
constexpr ServeName kUsersRows{"recommend_users_rows", "the rows", "item", "users"};
constexpr ServeName kUsersRowsAmong{"recommend_users_rows_among", "the rows", "item", "users"};

// The candidates of a recommend_among call as the caller gave them (checked by recommend_core): ptr == nullptr, one
// list for every request row; otherwise CSR over the request rows.
struct Candidates {
    const int64_t* ptr;
    const int32_t* items;
    int64_t n;
};

// The two sides of a top-N call (recommend_core): `own` is the model's matrix the request rows index where the caller
// brings no rows, `scanned` the one whose rows are scored and returned, all cfg.*n_scanned of them.
struct TopnSides {
    const DevArray<float> mfsgd_handle::*own;
    const DevArray<float> mfsgd_handle::*scanned;
    int32_t mfsgd_config::*n_scanned;
};
// P's users against Q's items; and the item-side calls (recommend_users): Q's items against P's users
constexpr TopnSides kItemsOfUsers{&mfsgd_handle::dP, &mfsgd_handle::dQ, &mfsgd_config::n_items};
constexpr TopnSides kUsersOfItems{&mfsgd_handle::dQ, &mfsgd_handle::dP, &mfsgd_config::n_users};

// A top-N call: "user j" is row j of a matrix of n_rows rows -- the model's P (host_rows == nullptr), or host_rows
// (n_rows x k, dense) -- and `users` names the n_users rows asked for.  cand != nullptr: among the candidates only.
struct TopnRequest {
    const float* host_rows = nullptr;
    int32_t n_rows = 0;
    const int32_t* users = nullptr;
    int32_t n_users = 0, topn = 0;
    const Candidates* cand = nullptr;
    Exclusions excl;
    int32_t* out_items = nullptr;
    float* out_scores = nullptr;
    TopnSides sides = kItemsOfUsers;  // (recommend_core; kUsersOfItems: everything above reads with the two words exchanged)
    bool for_items() const { return sides.scanned == &mfsgd_handle::dP; }
};

// The candidates as the kernels read them: sorted, distinct lists on the device (d_off, d_items: dev points into them),
// with their offsets on the host as well (one list: off = {0, its length}), which say how long each row's list came
// out, so what a batch holds and which path it takes.
struct CandLists {
    DevArray<long long> d_off;
    DevArray<int32_t> d_items;
    RecommendAmong dev;
    std::vector<long long> off;
    long long length(int32_t b) const { return dev.per_row ? off[(size_t)b + 1] - off[(size_t)b] : off[1]; }
};

// Candidate lists of one recommend_among call on the device, the way exclusions_to_device builds its lists: the items go
// up in chunks of bounded size, each becomes the key row << 32 | item (the row found in cand.ptr on the device), and the
// keys are sorted and made distinct into one ascending list per request row, or into one list (KeyLists).  Scratch lives
// as long as this function; `out` is the caller's.  cand.n > 0.
static int candidates_to_device(mfsgd_handle* h, const ServeName& what, const Candidates& cand, int32_t n_rows, DevBuf& temp,
                                CandLists& out) {
    const std::string prefix = std::string(what.call) + ": candidate lists: ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    DevArray<long long> d_ptr;
    DevArray<int32_t> ci;
    KeyLists k;
    const int64_t chunk = std::min(cand.n, kExclChunk);
    const int32_t n_slots = cand.ptr ? n_rows : 1;
    int rc;
    if (cand.ptr) {
        if ((rc = dev_alloc(h, d_ptr, (size_t)n_rows + 1))) return rc;
        HIPCHK_OR(bad, copy_up(d_ptr, cand.ptr, (size_t)n_rows + 1, h->stream));
    }
    if ((rc = dev_alloc(h, ci, (size_t)chunk)) || (rc = k.alloc(h, cand.n, n_slots))) return rc;
    for (int64_t x0 = 0; x0 < cand.n; x0 += chunk) {
        const int64_t c = std::min(chunk, cand.n - x0);
        HIPCHK_OR(bad, copy_up(ci, cand.items + x0, (size_t)c, h->stream));
        HIPCHK_OR(bad, recommend_cand_keys(cand.ptr ? d_ptr.data() : nullptr, n_rows, ci.data(), x0, c, k.keys.data(), h->stream));
    }
    HIPCHK_OR(bad, k.finish(cand.n, n_slots, temp, h->stream));
    out.off.resize((size_t)n_slots + 1);
    HIPCHK_OR(bad, copy_down(out.off.data(), k.off, (size_t)n_slots + 1, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    out.d_off = std::move(k.off);
    out.d_items = std::move(k.items);
    out.dev = RecommendAmong{out.d_off.data(), out.d_items.data(), cand.ptr ? 1 : 0};
    return MFSGD_OK;
}

// The device half of a top-N call, shared by recommend_core and similar_core: for each of the rows req.users[...] of
// job.P the job.topn rows of job.Q with the largest score (job.cs: the dot, or the cosine), exclusions as job.ex has
// them -- among all job.n_items rows of Q, or (cl, the dot only) among the candidates of request row b.  Fused where
// recommend_is_fused() holds for the longest row; otherwise in batches of rows through the sort path, about 64 M scores
// at a time (it materialises them): cells of rows x n_items, or of the lists' lengths added up.  `temp` is the sorts'
// scratch, the caller's (the lists may have grown it already).  `prefix` starts the message of a HIP failure.
constexpr int64_t kSortCells = (int64_t)64 << 20;
constexpr int64_t kLaunchRows = 65535;  // the launch's grid bounds a batch too

static int topn_batches(mfsgd_handle* h, const char* prefix, TopnJob job, const TopnRequest& req, const CandLists* cl, DevBuf& temp) {
    const int32_t I = job.n_items, topn = job.topn;
    auto length = [cl, I](int32_t b) -> int64_t { return cl ? cl->length(b) : I; };
    int64_t longest = cl ? 0 : I;
    for (int32_t b = 0; cl && b < req.n_users; ++b) longest = std::max(longest, length(b));
    const bool fused = recommend_is_fused(longest, topn);  // score + select in one kernel, no score buffers
    // whole rows per batch: as many as the cells allow (one at least)
    const Batches bt = cut_batches(req.n_users, length, fused ? INT64_MAX : kSortCells, kLaunchRows);
    auto bad = [h, prefix](hipError_t e) { return serve_fail(h, prefix, e); };
    DevArray<int32_t> d_users, id_in, id_out, o_i;
    DevArray<long long> d_off;
    DevArray<float> o_s;
    DevBuf s_in, s_out;  // read under two types: the scores as floats or, with exclusions, the unsigned keys the sort orders
    int rc;
    const size_t cells = (size_t)bt.max_weight, batch = (size_t)bt.max_rows;
    if ((rc = dev_alloc(h, d_users, batch))) return rc;
    if (!fused) {
        if ((rc = dev_alloc(h, s_in, sizeof(float) * cells)) || (rc = dev_alloc(h, s_out, sizeof(float) * cells))) return rc;
        if ((rc = dev_alloc(h, id_in, cells)) || (rc = dev_alloc(h, id_out, cells))) return rc;
        if ((rc = dev_alloc(h, d_off, batch + 1))) return rc;
    }
    if ((rc = dev_alloc(h, o_s, batch * (size_t)topn)) || (rc = dev_alloc(h, o_i, batch * (size_t)topn))) return rc;
    const TopnScratch scratch{s_in.as<float>(), s_out.as<float>(), id_in.data(), id_out.data(), d_off.data(), &temp};
    RecommendAmong am;
    job.L = h->geo.L, job.d_users = d_users.data();
    job.out_s = o_s.data(), job.out_i = o_i.data();
    for (size_t c = 0; c < bt.count(); ++c) {
        const int32_t done = bt.cut[c];
        job.nb = bt.cut[c + 1] - done;
        job.total = job.longest = 0;
        for (int32_t b = done; b < bt.cut[c + 1]; ++b) {
            job.total += length(b);
            job.longest = std::max(job.longest, length(b));
        }
        if (cl) {
            am = cl->dev;
            if (am.per_row) am.off += done;
            job.among = &am;
        }
        const size_t won = (size_t)job.nb * (size_t)topn;
        HIPCHK_OR(bad, copy_up(d_users, req.users + done, (size_t)job.nb, h->stream));
        HIPCHK_OR(bad, recommend_topn(job, fused ? nullptr : &scratch, h->stream));
        HIPCHK_OR(bad, copy_down(req.out_scores + (size_t)done * topn, o_s, won, h->stream));
        HIPCHK_OR(bad, copy_down(req.out_items + (size_t)done * topn, o_i, won, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    }
    return MFSGD_OK;
}

// Body of the recommend calls.  `what` is how the messages of the argument checks name the call (both recommend calls
// say "recommend"), `own` the call's own name, which its state errors carry.  The candidates (the among calls) are
// checked after the users and before the exclusion pairs.
// The same body serves the item-side calls (recommend_users): req names the two matrices and `what` the words, so
// "users" below are the request rows of either side and "items" the rows that are scanned.
static int recommend_core(mfsgd_handle* h, const ServeName& what, const char* own, const TopnRequest& req) {
    const std::string call = std::string(what.call) + ": ";
    const Exclusions& excl = req.excl;
    const Candidates* cand = req.cand;
    const int32_t n_users = req.n_users, topn = req.topn;
    if (n_users < 0 || topn < 1 || (n_users > 0 && (!req.users || !req.out_items || !req.out_scores)) || excl.n < 0 ||
        (excl.n > 0 && (!excl.u || !excl.i)))
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "bad argument");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    if (excl.from == Exclusions::kSeen && !h->seen.present) return fail(h, MFSGD_ERR_STATE, call + "no seen set");
    const int32_t n_scanned = h->cfg.*req.sides.n_scanned;
    if (topn > n_scanned) return fail(h, MFSGD_ERR_INVALID_ARG, call + "topn exceeds the number of " + what.scanned);
    int64_t x = first_outside(req.users, n_users, req.n_rows);
    if (x >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + what.row + " " + std::to_string(x) + " out of range");
    if (cand) {
        if (cand->n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_cand is negative");
        if (cand->n > 0 && !cand->items) return fail(h, MFSGD_ERR_INVALID_ARG, call + "cand_" + what.scanned + " is null");
        if (cand->ptr) {
            if (cand->ptr[0] != 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "cand_ptr[0] is not 0");
            for (int32_t b = 0; b < n_users; ++b)
                if (cand->ptr[b + 1] < cand->ptr[b])
                    return fail(h, MFSGD_ERR_INVALID_ARG, call + "cand_ptr decreases at row " + std::to_string(b));
            if (cand->ptr[n_users] != cand->n)
                return fail(h, MFSGD_ERR_INVALID_ARG, call + "cand_ptr ends at " + std::to_string(cand->ptr[n_users]) + ", not at n_cand");
        }
        if ((x = first_outside(cand->items, cand->n, n_scanned)) >= 0)
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "candidate " + std::to_string(x) + " out of range");
        if (cand->n > (int64_t)UINT32_MAX) return fail(h, MFSGD_ERR_INVALID_ARG, call + "more than 2^32 - 1 candidates");
    }
    // a slot per distinct requested user, and how many pairs are theirs (no table where there are no pairs)
    Slots slots;
    int64_t kept = 0;
    int rc;
    if (excl.n > 0) {
        slots = slots_of(req.users, n_users, req.n_rows);
        if ((rc = count_exclusions(h, what, slots.slot_of_row, req.n_rows, n_scanned, excl, &kept))) return rc;
    }
    if (n_users == 0) return MFSGD_OK;
    if (req.host_rows && h->where == mfsgd_handle::Where::None)  // (asked here: factors_to_device wants a device first)
        return fail(h, MFSGD_ERR_STATE, std::string(own) + ": factors not initialised");
    if ((rc = check_has_q(h, own)) || (rc = factors_to_device(h))) return rc;
    if (cand && cand->n == 0) {  // nothing is a candidate: every place is padding
        std::fill(req.out_items, req.out_items + (size_t)n_users * topn, -1);
        std::fill(req.out_scores, req.out_scores + (size_t)n_users * topn, std::nanf(""));
        return MFSGD_OK;
    }
    DevArray<float> d_rows;
    ExclLists lists;
    DevBuf temp;  // the rocPRIM scratch, bytes of no type: one for the lists and every batch, grown when one needs more
    TopnJob job;
    if ((rc = upload_rows(h, req.host_rows, req.n_rows, d_rows, &job.P, req.sides.own))) return rc;
    job.Q = (h->*req.sides.scanned).data();
    job.n_items = n_scanned;
    job.topn = topn;
    const auto t0 = std::chrono::steady_clock::now();
    CandLists cl;  // built once for all batches
    if (cand && (rc = candidates_to_device(h, what, *cand, n_users, temp, cl))) return rc;
    // the exclusion lists: built once for all batches; none when no pair belongs to a requested user, or the index is empty
    // (an item-side call cannot read the index where it lies: the lists of its items are made of it, like a caller's)
    const bool unseen = excl.from == Exclusions::kSeen;
    const Seen* by_item = unseen && req.for_items() && h->seen.n > 0 ? &h->seen : nullptr;
    if (unseen && !req.for_items()) job.ex = h->seen.excl();
    if (by_item) slots = slots_of(req.users, n_users, req.n_rows);
    if (by_item && (rc = audience_to_device(h, what, slots, *by_item, lists, temp, job.ex))) return rc;
    if (kept > 0 && (rc = exclusions_to_device(h, what, slots, excl, kept, lists, temp, job.ex))) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    rc = topn_batches(h, call.c_str(), job, req, cand ? &cl : nullptr, temp);
    // (both halves end in a synchronise: mfsgd_debug_serve_seconds)
    h->serve_lists_s = std::chrono::duration<double>(t1 - t0).count();
    h->serve_topn_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return rc;
}

// Body of the similar calls: the neighbours of the query rows among the rows of one side's matrix M (Q for
// MFSGD_SIDE_ITEMS, P for MFSGD_SIDE_USERS) under the cosine of DESIGN.md section 3.  req.host_rows == nullptr: the
// queries are the rows req.users[...] of M itself, and with self_excl each leaves out its own index: a one-item
// exclusion list per distinct query, so the EXCL variants of recommend.hip do it.  Otherwise the queries are
// req.host_rows (n_rows x k, dense), uploaded for the length of the call, req.users[...] index them, and nothing is
// excluded.  The inverse norms are computed here, per call; nothing stays in the handle.  `name` is the call's, without
// the colon.
static int similar_core(mfsgd_handle* h, const char* name, int32_t side, bool self_excl, const TopnRequest& req) {
    const std::string call = std::string(name) + ": ";
    const int32_t n = req.n_users;
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n is negative");
    if (req.topn < 1) return fail(h, MFSGD_ERR_INVALID_ARG, call + "topn is below 1");
    if (n > 0 && (!req.users || !req.out_items || !req.out_scores))
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "the queries or an output array is null");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    const bool of_items = side == MFSGD_SIDE_ITEMS;
    const int32_t size = of_items ? h->cfg.n_items : h->cfg.n_users;
    if (req.topn > size) return fail(h, MFSGD_ERR_INVALID_ARG, call + "topn exceeds the number of " + (of_items ? "items" : "users"));
    const int64_t x = first_outside(req.users, n, req.n_rows);
    if (x >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "query " + std::to_string(x) + " out of range");
    if (n == 0) return MFSGD_OK;
    int rc;  // (the users' side reads P alone; one partition is known by now, and asked about again)
    if ((rc = check_reads_factors(h, name, of_items)) || (rc = factors_to_device(h))) return rc;
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    DevArray<float> d_rows, d_ra, d_rb;
    ExclLists lists;
    DevBuf temp;  // the rocPRIM scratch, bytes of no type
    TopnJob job;
    job.Q = job.P = of_items ? h->dQ.data() : h->dP.data();
    if (req.host_rows && (rc = upload_rows(h, req.host_rows, req.n_rows, d_rows, &job.P))) return rc;
    job.n_items = size;
    job.topn = req.topn;
    if ((rc = dev_alloc(h, d_rb, (size_t)size))) return rc;
    HIPCHK_OR(bad, launch_row_inv_norms(h->geo.L, job.Q, size, d_rb.data(), h->stream));
    job.cs.ra = job.cs.rb = d_rb.data();
    if (req.host_rows) {
        if ((rc = dev_alloc(h, d_ra, (size_t)req.n_rows))) return rc;
        HIPCHK_OR(bad, launch_row_inv_norms(h->geo.L, job.P, req.n_rows, d_ra.data(), h->stream));
        job.cs.ra = d_ra.data();
    }
    if (self_excl) {
        // a slot per distinct query; the list of slot s is the query itself
        const Slots slots = slots_of(req.users, n, req.n_rows);
        std::vector<long long> off((size_t)slots.n() + 1);
        std::iota(off.begin(), off.end(), 0LL);
        if ((rc = upload(h, lists.slot, slots.slot_of_row))) return rc;
        if ((rc = upload(h, lists.off, off))) return rc;
        if ((rc = upload(h, lists.items, slots.row_of_slot))) return rc;
        job.ex = RecommendExcl{lists.slot.data(), lists.off.data(), lists.items.data()};
    }
    return topn_batches(h, call.c_str(), job, req, nullptr, temp);
}

}  // namespace mfsgd

using namespace mfsgd;

extern "C" {

int mfsgd_predict(mfsgd_handle* h, const int32_t* u, const int32_t* i, float* out, int64_t n) {
    return guarded(h, "predict", [&]() -> int {
        if (n < 0 || (n > 0 && (!u || !i || !out))) return fail(h, MFSGD_ERR_INVALID_ARG, "predict: bad argument");
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "predict: single-partition handles only");
        const int64_t j = first_outside(u, h->cfg.n_users, i, h->cfg.n_items, n);
        if (j >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, "predict: pair " + std::to_string(j) + " out of range");
        if (n == 0) return MFSGD_OK;
        int rc = check_has_q(h, "predict");
        if (rc || (rc = factors_to_device(h))) return rc;
        DevArray<int32_t> du, di;
        DevArray<float> dout;
        if ((rc = dev_alloc(h, du, (size_t)n)) || (rc = dev_alloc(h, di, (size_t)n))) return rc;
        if ((rc = dev_alloc(h, dout, (size_t)n))) return rc;
        // (this call has always reported every HIP failure as MFSGD_ERR_HIP and left the runtime's error word alone)
        auto bad = [h](hipError_t e) { return fail(h, MFSGD_ERR_HIP, std::string("predict: ") + hipGetErrorString(e)); };
        HIPCHK_OR(bad, copy_up(du, u, (size_t)n, h->stream));
        HIPCHK_OR(bad, copy_up(di, i, (size_t)n, h->stream));
        HIPCHK_OR(bad, launch_predict(h->geo.L, h->dP.data(), h->dQ.data(), du.data(), di.data(), dout.data(), n, h->stream));
        HIPCHK_OR(bad, copy_down(out, dout, (size_t)n, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
        return MFSGD_OK;
    });
}

int mfsgd_recommend(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, int32_t* out_items,
                    float* out_scores) {
    return guarded(h, "recommend", [&]() -> int {
        return recommend_core(h, kRecommend, "recommend", {nullptr, h->cfg.n_users, users, n_users, topn, nullptr, {},
                              out_items, out_scores});
    });
}

int mfsgd_recommend_excluding(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, const int32_t* excl_u,
                              const int32_t* excl_i, int64_t n_excl, int32_t* out_items, float* out_scores) {
    return guarded(h, "recommend", [&]() -> int {
        return recommend_core(h, kRecommend, "recommend", {nullptr, h->cfg.n_users, users, n_users, topn, nullptr,
                              Exclusions::pairs(excl_u, excl_i, n_excl), out_items, out_scores});
    });
}

int mfsgd_recommend_rows(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn, const int32_t* excl_row,
                         const int32_t* excl_item, int64_t n_excl, int32_t* out_items, float* out_scores) {
    return guarded(h, "recommend_rows", [&]() -> int {
        if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(h, MFSGD_ERR_INVALID_ARG, "recommend_rows: bad argument");
        const std::vector<int32_t> all = all_rows(n_rows);
        return recommend_core(h, kRecommend, "recommend_rows", {rows, n_rows, all.data(), n_rows, topn, nullptr,
                              Exclusions::pairs(excl_row, excl_item, n_excl), out_items, out_scores});
    });
}

int mfsgd_recommend_among(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, const int64_t* cand_ptr,
                          const int32_t* cand_items, int64_t n_cand, const int32_t* excl_u, const int32_t* excl_i,
                          int64_t n_excl, int32_t* out_items, float* out_scores) {
    return guarded(h, "recommend_among", [&]() -> int {
        const Candidates cand{cand_ptr, cand_items, n_cand};
        return recommend_core(h, kAmong, kAmong.call, {nullptr, h->cfg.n_users, users, n_users, topn, &cand,
                              Exclusions::pairs(excl_u, excl_i, n_excl), out_items, out_scores});
    });
}

int mfsgd_recommend_rows_among(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn, const int64_t* cand_ptr,
                               const int32_t* cand_items, int64_t n_cand, const int32_t* excl_row, const int32_t* excl_item,
                               int64_t n_excl, int32_t* out_items, float* out_scores) {
    return guarded(h, "recommend_rows_among", [&]() -> int {
        if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(h, MFSGD_ERR_INVALID_ARG, "recommend_rows_among: bad argument");
        const std::vector<int32_t> all = all_rows(n_rows);
        const Candidates cand{cand_ptr, cand_items, n_cand};
        return recommend_core(h, kRowsAmong, kRowsAmong.call, {rows, n_rows, all.data(), n_rows, topn, &cand,
                              Exclusions::pairs(excl_row, excl_item, n_excl), out_items, out_scores});
    });
}

int mfsgd_debug_serve_seconds(mfsgd_handle* h, double* out2) {
    return guarded(h, "debug_serve_seconds", [&]() -> int {
        if (!out2) return fail(h, MFSGD_ERR_INVALID_ARG, "debug_serve_seconds: out2 is null");
        out2[0] = h->serve_lists_s;
        out2[1] = h->serve_topn_s;
        return MFSGD_OK;
    });
}

int mfsgd_row_inv_norms(mfsgd_handle* h, int32_t side, float* out) {
    return guarded(h, "row_inv_norms", [&]() -> int {
        if (side != MFSGD_SIDE_USERS && side != MFSGD_SIDE_ITEMS)
            return fail(h, MFSGD_ERR_INVALID_ARG, "row_inv_norms: side is neither MFSGD_SIDE_USERS nor MFSGD_SIDE_ITEMS");
        if (!out) return fail(h, MFSGD_ERR_INVALID_ARG, "row_inv_norms: out is null");
        const bool of_items = side == MFSGD_SIDE_ITEMS;  // (the users' side reads P alone)
        int rc = check_reads_factors(h, "row_inv_norms", of_items);
        if (rc || (rc = factors_to_device(h))) return rc;
        const int32_t size = of_items ? h->cfg.n_items : h->cfg.n_users;
        auto bad = [h](hipError_t e) { return serve_fail(h, "row_inv_norms: ", e); };
        DevArray<float> d_rn;
        if ((rc = dev_alloc(h, d_rn, (size_t)size))) return rc;
        HIPCHK_OR(bad, launch_row_inv_norms(h->geo.L, of_items ? h->dQ.data() : h->dP.data(), size, d_rn.data(), h->stream));
        HIPCHK_OR(bad, copy_down(out, d_rn, (size_t)size, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
        return MFSGD_OK;
    });
}

int mfsgd_similar_items(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn, int32_t* out_items,
                        float* out_scores) {
    return guarded(h, "similar_items", [&]() -> int {
        return similar_core(h, "similar_items", MFSGD_SIDE_ITEMS, true, {nullptr, h->cfg.n_items, items, n, topn, nullptr, {},
                            out_items, out_scores});
    });
}

int mfsgd_similar_users(mfsgd_handle* h, const int32_t* users, int32_t n, int32_t topn, int32_t* out_users,
                        float* out_scores) {
    return guarded(h, "similar_users", [&]() -> int {
        return similar_core(h, "similar_users", MFSGD_SIDE_USERS, true, {nullptr, h->cfg.n_users, users, n, topn, nullptr, {},
                            out_users, out_scores});
    });
}

int mfsgd_similar_rows(mfsgd_handle* h, int32_t side, const float* rows, int32_t n_rows, int32_t topn, int32_t* out_index,
                       float* out_scores) {
    return guarded(h, "similar_rows", [&]() -> int {
        if (side != MFSGD_SIDE_USERS && side != MFSGD_SIDE_ITEMS)
            return fail(h, MFSGD_ERR_INVALID_ARG, "similar_rows: side is neither MFSGD_SIDE_USERS nor MFSGD_SIDE_ITEMS");
        if (n_rows < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "similar_rows: n_rows is negative");
        if (n_rows > 0 && !rows) return fail(h, MFSGD_ERR_INVALID_ARG, "similar_rows: rows is null");
        const std::vector<int32_t> all = all_rows(n_rows);
        return similar_core(h, "similar_rows", side, false, {rows, n_rows, all.data(), n_rows, topn, nullptr, {}, out_index,
                            out_scores});
    });
}

int mfsgd_recommend_unseen(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, int32_t* out_items,
                           float* out_scores) {
    return guarded(h, kUnseen.call, [&]() -> int {
        return recommend_core(h, kUnseen, kUnseen.call, {nullptr, h->cfg.n_users, users, n_users, topn, nullptr,
                              Exclusions::seen(), out_items, out_scores});
    });
}

int mfsgd_recommend_unseen_among(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, const int64_t* cand_ptr,
                                 const int32_t* cand_items, int64_t n_cand, int32_t* out_items, float* out_scores) {
    return guarded(h, kUnseenAmong.call, [&]() -> int {
        const Candidates cand{cand_ptr, cand_items, n_cand};
        return recommend_core(h, kUnseenAmong, kUnseenAmong.call, {nullptr, h->cfg.n_users, users, n_users, topn, &cand,
                              Exclusions::seen(), out_items, out_scores});
    });
}

// The item-side family: Q's rows (or item rows of the caller's) against P.  The exclusion pairs keep the library's
// (user, item) orientation at the surface and reach the core exchanged, request side first.
int mfsgd_recommend_users(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn, const int32_t* excl_u,
                          const int32_t* excl_i, int64_t n_excl, int32_t* out_users, float* out_scores) {
    return guarded(h, kUsers.call, [&]() -> int {
        return recommend_core(h, kUsers, kUsers.call, {nullptr, h->cfg.n_items, items, n, topn, nullptr,
                              Exclusions::pairs(excl_i, excl_u, n_excl), out_users, out_scores, kUsersOfItems});
    });
}

int mfsgd_recommend_users_among(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn, const int64_t* cand_ptr,
                                const int32_t* cand_users, int64_t n_cand, const int32_t* excl_u, const int32_t* excl_i,
                                int64_t n_excl, int32_t* out_users, float* out_scores) {
    return guarded(h, kUsersAmong.call, [&]() -> int {
        const Candidates cand{cand_ptr, cand_users, n_cand};
        return recommend_core(h, kUsersAmong, kUsersAmong.call, {nullptr, h->cfg.n_items, items, n, topn, &cand,
                              Exclusions::pairs(excl_i, excl_u, n_excl), out_users, out_scores, kUsersOfItems});
    });
}

int mfsgd_recommend_users_unseen(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn, int32_t* out_users,
                                 float* out_scores) {
    return guarded(h, kUsersUnseen.call, [&]() -> int {
        return recommend_core(h, kUsersUnseen, kUsersUnseen.call, {nullptr, h->cfg.n_items, items, n, topn, nullptr,
                              Exclusions::seen(), out_users, out_scores, kUsersOfItems});
    });
}

int mfsgd_recommend_users_unseen_among(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn, const int64_t* cand_ptr,
                                       const int32_t* cand_users, int64_t n_cand, int32_t* out_users, float* out_scores) {
    return guarded(h, kUsersUnseenAmong.call, [&]() -> int {
        const Candidates cand{cand_ptr, cand_users, n_cand};
        return recommend_core(h, kUsersUnseenAmong, kUsersUnseenAmong.call, {nullptr, h->cfg.n_items, items, n, topn, &cand,
                              Exclusions::seen(), out_users, out_scores, kUsersOfItems});
    });
}

int mfsgd_recommend_users_rows(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn, const int32_t* excl_row,
                               const int32_t* excl_user, int64_t n_excl, int32_t* out_users, float* out_scores) {
    return guarded(h, kUsersRows.call, [&]() -> int {
        if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(h, MFSGD_ERR_INVALID_ARG, "recommend_users_rows: bad argument");
        const std::vector<int32_t> all = all_rows(n_rows);
        return recommend_core(h, kUsersRows, kUsersRows.call, {rows, n_rows, all.data(), n_rows, topn, nullptr,
                              Exclusions::pairs(excl_row, excl_user, n_excl), out_users, out_scores, kUsersOfItems});
    });
}

int mfsgd_recommend_users_rows_among(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn, const int64_t* cand_ptr,
                                     const int32_t* cand_users, int64_t n_cand, const int32_t* excl_row,
                                     const int32_t* excl_user, int64_t n_excl, int32_t* out_users, float* out_scores) {
    return guarded(h, kUsersRowsAmong.call, [&]() -> int {
        if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(h, MFSGD_ERR_INVALID_ARG, "recommend_users_rows_among: bad argument");
        const std::vector<int32_t> all = all_rows(n_rows);
        const Candidates cand{cand_ptr, cand_users, n_cand};
        return recommend_core(h, kUsersRowsAmong, kUsersRowsAmong.call, {rows, n_rows, all.data(), n_rows, topn, &cand,
                              Exclusions::pairs(excl_row, excl_user, n_excl), out_users, out_scores, kUsersOfItems});
    });
}

}  // extern "C"
