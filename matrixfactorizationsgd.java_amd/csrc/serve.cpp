// serve.cpp -- what a trained model answers: predictions, top-N recommendations, cosine neighbours of items and users,
// ranks of held-out items and their metrics, and the fold-in of new users and new items.  Every call batches its work
// through bounded staging buffers.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "handle.hpp"

namespace mfsgd {

// How a serving call speaks of itself and of the users it was given, in the messages the two cores share.
struct ServeName {
    const char* call;
    const char* whose;
};
constexpr ServeName kRecommend{"recommend", "the requested users"}, kRank{"rank_items", "the users asked about"};
constexpr ServeName kAmong{"recommend_among", "the requested users"}, kRowsAmong{"recommend_rows_among", "the rows"};
// ... and the calls that exclude what the handle's seen-item index holds instead of a pair list
constexpr ServeName kUnseen{"recommend_unseen", "the requested users"}, kUnseenAmong{"recommend_unseen_among", "the requested users"};
constexpr ServeName kRankUnseen{"rank_items_unseen", "the users asked about"};
constexpr ServeName kEvaluateUnseen{"evaluate_ranking_unseen", "the users asked about"};

// The row matrix of a serving call on the device: the model's P, or host_rows (n_rows x k, dense), which goes up into
// a kp-padded temporary (`buf`) for the length of the call.
static int upload_rows(mfsgd_handle* h, const float* host_rows, int32_t n_rows, DevBuf& buf, const float** rows) {
    *rows = h->dP.as<const float>();
    if (!host_rows) return MFSGD_OK;
    const int k = h->cfg.k, kp = h->geo.kp;
    std::vector<float> padded((size_t)n_rows * kp, 0.0f);
    for (int64_t x = 0; x < n_rows; ++x) std::memcpy(&padded[(size_t)x * kp], host_rows + x * k, sizeof(float) * (size_t)k);
    const int rc = upload(h, buf, padded);
    *rows = buf.as<const float>();
    return rc;
}

// Range check of the exclusion pairs, and *kept = how many of them belong to a user that has a slot.
static int count_exclusions(const mfsgd_handle* h, const ServeName& what, const std::vector<int32_t>& slot_of_user, int32_t n_rows,
                            const int32_t* excl_u, const int32_t* excl_i, int64_t n_excl, int64_t* kept) {
    *kept = 0;
    for (int64_t x = 0; x < n_excl; ++x) {
        if (excl_u[x] < 0 || excl_u[x] >= n_rows || excl_i[x] < 0 || excl_i[x] >= h->cfg.n_items)
            return fail(h, MFSGD_ERR_INVALID_ARG, std::string(what.call) + ": excluded pair " + std::to_string(x) + " out of range");
        *kept += slot_of_user[(size_t)excl_u[x]] >= 0 ? 1 : 0;
    }
    if (*kept > (int64_t)UINT32_MAX)
        return fail(h, MFSGD_ERR_INVALID_ARG, std::string(what.call) + ": more than 2^32 - 1 excluded pairs of " + what.whose);
    return MFSGD_OK;
}

// Exclusion lists of one recommend call on the device: the pairs go up in chunks of bounded size, those of requested
// users are kept (slot << 32 | item), then sorted and made distinct into one list per slot (recommend.hip).
// Scratch lives as long as this function; `ex` points into `slot`, `off` and `items`, which are the caller's.
// `what` starts the message of a HIP failure: the call the lists are built for.
// (kExclChunk pairs per upload, handle.hpp)
static int exclusions_to_device(mfsgd_handle* h, const ServeName& what, const std::vector<int32_t>& slot_of_user, int32_t n_slots,
                                const int32_t* excl_u, const int32_t* excl_i, int64_t n_excl, int64_t kept, DevBuf& slot,
                                DevBuf& off, DevBuf& items, DevBuf& temp, RecommendExcl& ex) {
    const std::string prefix = std::string(what.call) + ": exclusion lists: ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    DevBuf cu, ci, keys, keys_tmp, count;
    const int64_t chunk = std::min(n_excl, kExclChunk);
    int rc;
    if ((rc = upload(h, slot, slot_of_user))) return rc;
    if ((rc = dev_alloc(h, cu, sizeof(int32_t) * (size_t)chunk))) return rc;
    if ((rc = dev_alloc(h, ci, sizeof(int32_t) * (size_t)chunk))) return rc;
    if ((rc = dev_alloc(h, keys, 8 * (size_t)kept))) return rc;
    if ((rc = dev_alloc(h, keys_tmp, 8 * (size_t)kept))) return rc;
    if ((rc = dev_alloc(h, count, 16))) return rc;  // [0] appended pairs (u64), [2] distinct ones (u32)
    if ((rc = dev_alloc(h, off, sizeof(long long) * ((size_t)n_slots + 1)))) return rc;
    if ((rc = dev_alloc(h, items, sizeof(int32_t) * (size_t)kept))) return rc;
    auto* cnt = count.as<unsigned long long>();
    HIPCHK_OR(bad, hipMemsetAsync(cnt, 0, 16, h->stream));
    for (int64_t x0 = 0; x0 < n_excl; x0 += chunk) {
        const int64_t c = std::min(chunk, n_excl - x0);
        HIPCHK_OR(bad, hipMemcpyAsync(cu.get(), excl_u + x0, sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, hipMemcpyAsync(ci.get(), excl_i + x0, sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, recommend_excl_filter(slot.as<const int32_t>(), cu.as<const int32_t>(), ci.as<const int32_t>(), c,
                                             keys.as<unsigned long long>(), cnt, kept, h->stream));
    }
    HIPCHK_OR(bad, recommend_excl_lists(keys.as<unsigned long long>(), keys_tmp.as<unsigned long long>(), kept, n_slots,
                                        reinterpret_cast<unsigned*>(cnt + 1), off.as<long long>(), items.as<int32_t>(),
                                        temp, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    ex.slot = slot.as<const int32_t>();
    ex.off = off.as<const long long>();
    ex.items = items.as<const int32_t>();
    return MFSGD_OK;
}

// The candidates of a recommend_among call as the caller gave them (checked by recommend_core): ptr == nullptr, one
// list for every request row; otherwise CSR over the request rows.
struct Candidates {
    const int64_t* ptr;
    const int32_t* items;
    int64_t n;
};

// ... and as the kernels read them: sorted, distinct lists on the device, with their offsets on the host as well (one
// list: off = {0, its length}), which say how long each row's list came out, so what a batch holds and which path it takes.
struct CandLists {
    RecommendAmong dev;
    std::vector<long long> off;
    long long length(int32_t b) const { return dev.per_row ? off[(size_t)b + 1] - off[(size_t)b] : off[1]; }
};

// Candidate lists of one recommend_among call on the device, the way exclusions_to_device builds its lists: the items go
// up in chunks of bounded size, each becomes the key row << 32 | item (the row found in cand.ptr on the device), and the
// keys are sorted and made distinct into one ascending list per request row, or into one list.  Scratch lives as long
// as this function; `out` points into `off` and `items`, which are the caller's.  cand.n > 0.
static int candidates_to_device(mfsgd_handle* h, const ServeName& what, const Candidates& cand, int32_t n_rows, DevBuf& off,
                                DevBuf& items, DevBuf& temp, CandLists& out) {
    const std::string prefix = std::string(what.call) + ": candidate lists: ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    DevBuf d_ptr, ci, keys, keys_tmp, count;
    const int64_t chunk = std::min(cand.n, kExclChunk);
    const int32_t n_slots = cand.ptr ? n_rows : 1;
    int rc;
    if (cand.ptr) {
        if ((rc = dev_alloc(h, d_ptr, sizeof(int64_t) * ((size_t)n_rows + 1)))) return rc;
        HIPCHK_OR(bad, hipMemcpyAsync(d_ptr.get(), cand.ptr, sizeof(int64_t) * ((size_t)n_rows + 1), hipMemcpyHostToDevice, h->stream));
    }
    if ((rc = dev_alloc(h, ci, sizeof(int32_t) * (size_t)chunk))) return rc;
    if ((rc = dev_alloc(h, keys, 8 * (size_t)cand.n))) return rc;
    if ((rc = dev_alloc(h, keys_tmp, 8 * (size_t)cand.n))) return rc;
    if ((rc = dev_alloc(h, count, 16))) return rc;  // [0] distinct keys (u32)
    if ((rc = dev_alloc(h, off, sizeof(long long) * ((size_t)n_slots + 1)))) return rc;
    if ((rc = dev_alloc(h, items, sizeof(int32_t) * (size_t)cand.n))) return rc;
    for (int64_t x0 = 0; x0 < cand.n; x0 += chunk) {
        const int64_t c = std::min(chunk, cand.n - x0);
        HIPCHK_OR(bad, hipMemcpyAsync(ci.get(), cand.items + x0, sizeof(int32_t) * (size_t)c, hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, recommend_cand_keys(cand.ptr ? d_ptr.as<const long long>() : nullptr, n_rows, ci.as<const int32_t>(), x0, c,
                                           keys.as<unsigned long long>(), h->stream));
    }
    HIPCHK_OR(bad, recommend_excl_lists(keys.as<unsigned long long>(), keys_tmp.as<unsigned long long>(), cand.n, n_slots,
                                        count.as<unsigned>(), off.as<long long>(), items.as<int32_t>(), temp, h->stream));
    out.off.resize((size_t)n_slots + 1);
    HIPCHK_OR(bad, hipMemcpyAsync(out.off.data(), off.get(), sizeof(long long) * ((size_t)n_slots + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    out.dev.off = off.as<const long long>();
    out.dev.items = items.as<const int32_t>();
    out.dev.per_row = cand.ptr ? 1 : 0;
    return MFSGD_OK;
}

// The device half of a top-N call, shared by recommend_core and similar_core: for each of the n rows users[...] of P the
// topn rows of Q with the largest score (cs: the dot, or the cosine), exclusions as `ex` has them -- among all n_items
// rows of Q, or (cl, the dot only) among the candidates of request row b.  Fused where recommend_is_fused() /
// recommend_among_is_fused() holds; otherwise in batches of rows through the sort path, about 64 M scores at a time
// (it materialises them): cells of rows x n_items, or of the lists' lengths added up.  `temp` is the sorts' scratch, the
// caller's (the lists may have grown it already).  `prefix` starts the message of a HIP failure.
constexpr int64_t kSortCells = (int64_t)64 << 20;

static int topn_batches(mfsgd_handle* h, const char* prefix, const float* P, const float* Q, int32_t I, const int32_t* users,
                        int32_t n_users, int32_t topn, const RecommendExcl& ex, const CosineScale& cs, DevBuf& temp,
                        int32_t* out_items, float* out_scores, const CandLists* cl = nullptr) {
    auto length = [cl, I](int32_t b) -> int64_t { return cl ? cl->length(b) : I; };
    int64_t longest = cl ? 0 : I;
    for (int32_t b = 0; cl && b < n_users; ++b) longest = std::max(longest, length(b));
    // score + select in one kernel, no score buffers
    const bool fused = cl ? recommend_among_is_fused(longest, topn) : recommend_is_fused(I, topn);
    // whole rows per batch: as many as the cells allow (one at least), the launch's grid bounding them too
    std::vector<int32_t> cut{0};
    std::vector<int64_t> batch_cells, batch_longest;
    int64_t max_cells = 0;
    int32_t batch = 0;
    for (int32_t b0 = 0; b0 < n_users;) {
        int32_t b1 = b0;
        int64_t cells = 0, lng = 0;
        while (b1 < n_users && b1 - b0 < 65535 && (fused || b1 == b0 || cells + length(b1) <= kSortCells)) {
            cells += length(b1);
            lng = std::max(lng, length(b1));
            ++b1;
        }
        cut.push_back(b1);
        batch_cells.push_back(cells);
        batch_longest.push_back(lng);
        max_cells = std::max(max_cells, cells);
        batch = std::max(batch, b1 - b0);
        b0 = b1;
    }
    auto bad = [h, prefix](hipError_t e) { return serve_fail(h, prefix, e); };
    DevBuf d_users, s_in, s_out, id_in, id_out, d_off, o_s, o_i;
    int rc;
    const size_t cells = (size_t)max_cells;
    if ((rc = dev_alloc(h, d_users, sizeof(int32_t) * (size_t)batch))) return rc;
    if (!fused) {
        if ((rc = dev_alloc(h, s_in, 4 * cells))) return rc;
        if ((rc = dev_alloc(h, s_out, 4 * cells))) return rc;
        if ((rc = dev_alloc(h, id_in, 4 * cells))) return rc;
        if ((rc = dev_alloc(h, id_out, 4 * cells))) return rc;
        if ((rc = dev_alloc(h, d_off, sizeof(long long) * ((size_t)batch + 1)))) return rc;
    }
    if ((rc = dev_alloc(h, o_s, 4 * (size_t)batch * topn))) return rc;
    if ((rc = dev_alloc(h, o_i, 4 * (size_t)batch * topn))) return rc;
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const int32_t done = cut[c];
        const int nb = cut[c + 1] - done;
        const int32_t* du = d_users.as<const int32_t>();
        HIPCHK_OR(bad, hipMemcpyAsync(d_users.get(), users + done, sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, h->stream));
        if (cl) {
            RecommendAmong am = cl->dev;
            if (am.per_row) am.off += done;
            if (fused)
                HIPCHK_OR(bad, recommend_among_fused(h->geo.L, P, Q, du, nb, am, topn, ex, o_s.as<float>(), o_i.as<int32_t>(),
                                                     h->stream));
            else
                HIPCHK_OR(bad, recommend_among_batch(h->geo.L, P, Q, du, nb, am, batch_cells[c], batch_longest[c], topn, ex,
                                                     s_in.as<float>(), s_out.as<float>(), id_in.as<int32_t>(),
                                                     id_out.as<int32_t>(), d_off.as<long long>(), temp, o_s.as<float>(),
                                                     o_i.as<int32_t>(), h->stream));
        } else if (fused) {
            HIPCHK_OR(bad, recommend_fused(h->geo.L, P, Q, du, nb, I, topn, ex, cs, o_s.as<float>(), o_i.as<int32_t>(), h->stream));
        } else {
            HIPCHK_OR(bad, recommend_batch(h->geo.L, P, Q, du, nb, I, topn, ex, cs, s_in.as<float>(), s_out.as<float>(),
                                           id_in.as<int32_t>(), id_out.as<int32_t>(), d_off.as<long long>(), temp,
                                           o_s.as<float>(), o_i.as<int32_t>(), h->stream));
        }
        HIPCHK_OR(bad, hipMemcpyAsync(out_scores + (size_t)done * topn, o_s.get(), 4 * (size_t)nb * topn, hipMemcpyDeviceToHost, h->stream));
        HIPCHK_OR(bad, hipMemcpyAsync(out_items + (size_t)done * topn, o_i.get(), 4 * (size_t)nb * topn, hipMemcpyDeviceToHost, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    }
    return MFSGD_OK;
}

// Body of the recommend calls: "user j" is row j of a matrix of n_rows rows, and `users` names the rows asked for.
// host_rows == nullptr: the matrix is the model's P.  Otherwise it is host_rows (n_rows x k, dense).
// `what` is how the messages of the argument checks name the call (both recommend calls say "recommend"), `own` the
// call's own name, which its state errors carry.  cand != nullptr: among the candidates only (the among calls), which
// are checked after the users and before the exclusion pairs.  unseen: the exclusion lists are those of the handle's
// seen-item index, read where they lie through its identity slot table (the _unseen calls: no pairs, the model's P) --
// nothing is built, uploaded or looped over for them, on the host or on the device.
static int recommend_core(mfsgd_handle* h, const ServeName& what, const char* own, const float* host_rows, int32_t n_rows,
                          const int32_t* users, int32_t n_users, int32_t topn, const Candidates* cand, const int32_t* excl_u,
                          const int32_t* excl_i, int64_t n_excl, int32_t* out_items, float* out_scores, bool unseen = false) {
    const std::string call = std::string(what.call) + ": ";
    if (n_users < 0 || topn < 1 || (n_users > 0 && (!users || !out_items || !out_scores)) || n_excl < 0 ||
        (n_excl > 0 && (!excl_u || !excl_i)))
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "bad argument");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    if (unseen && !h->seen.present) return fail(h, MFSGD_ERR_STATE, call + "no seen set");
    if (topn > h->cfg.n_items) return fail(h, MFSGD_ERR_INVALID_ARG, call + "topn exceeds the number of items");
    for (int32_t j = 0; j < n_users; ++j)
        if (users[j] < 0 || users[j] >= n_rows)
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "user " + std::to_string(j) + " out of range");
    if (cand) {
        if (cand->n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_cand is negative");
        if (cand->n > 0 && !cand->items) return fail(h, MFSGD_ERR_INVALID_ARG, call + "cand_items is null");
        if (cand->ptr) {
            if (cand->ptr[0] != 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "cand_ptr[0] is not 0");
            for (int32_t b = 0; b < n_users; ++b)
                if (cand->ptr[b + 1] < cand->ptr[b])
                    return fail(h, MFSGD_ERR_INVALID_ARG, call + "cand_ptr decreases at row " + std::to_string(b));
            if (cand->ptr[n_users] != cand->n)
                return fail(h, MFSGD_ERR_INVALID_ARG, call + "cand_ptr ends at " + std::to_string(cand->ptr[n_users]) + ", not at n_cand");
        }
        // (in blocks without a branch, so that the compiler vectorises it: the candidates are the most the host reads)
        const uint32_t I = (uint32_t)h->cfg.n_items;
        for (int64_t x0 = 0; x0 < cand->n; x0 += 4096) {
            const int64_t x1 = std::min(cand->n, x0 + 4096);
            uint32_t outside = 0;
            for (int64_t x = x0; x < x1; ++x) outside |= (uint32_t)((uint32_t)cand->items[x] >= I);
            for (int64_t x = x0; outside && x < x1; ++x)
                if ((uint32_t)cand->items[x] >= I)
                    return fail(h, MFSGD_ERR_INVALID_ARG, call + "candidate " + std::to_string(x) + " out of range");
        }
        if (cand->n > (int64_t)UINT32_MAX) return fail(h, MFSGD_ERR_INVALID_ARG, call + "more than 2^32 - 1 candidates");
    }
    // a slot per distinct requested user (one user asked for twice shares it), and how many pairs are theirs
    std::vector<int32_t> slot_of_user;
    int32_t n_slots = 0;
    int64_t kept = 0;
    int rc;
    if (n_excl > 0) {
        slot_of_user.assign((size_t)n_rows, -1);
        for (int32_t j = 0; j < n_users; ++j)
            if (slot_of_user[(size_t)users[j]] < 0) slot_of_user[(size_t)users[j]] = n_slots++;
        if ((rc = count_exclusions(h, what, slot_of_user, n_rows, excl_u, excl_i, n_excl, &kept))) return rc;
    }
    if (n_users == 0) return MFSGD_OK;
    if (host_rows && h->where == mfsgd_handle::Where::None)  // (asked here: factors_to_device wants a device first)
        return fail(h, MFSGD_ERR_STATE, std::string(own) + ": factors not initialised");
    if ((rc = check_has_q(h, own)) || (rc = factors_to_device(h))) return rc;
    if (cand && cand->n == 0) {  // nothing is a candidate: every place is padding
        std::fill(out_items, out_items + (size_t)n_users * topn, -1);
        std::fill(out_scores, out_scores + (size_t)n_users * topn, std::nanf(""));
        return MFSGD_OK;
    }
    DevBuf d_rows, ex_slot, ex_off, ex_items, cand_off, cand_items;
    DevBuf temp;  // of the sorts: one for the lists and every batch, grown when one needs more
    const float* P;
    if ((rc = upload_rows(h, host_rows, n_rows, d_rows, &P))) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    CandLists cl;  // built once for all batches
    if (cand && (rc = candidates_to_device(h, what, *cand, n_users, cand_off, cand_items, temp, cl))) return rc;
    RecommendExcl ex;  // built once for all batches; none when no pair belongs to a requested user
    if (unseen) ex = h->seen.excl();  // (none when the index is empty)
    if (kept > 0 && (rc = exclusions_to_device(h, what, slot_of_user, n_slots, excl_u, excl_i, n_excl, kept, ex_slot,
                                               ex_off, ex_items, temp, ex)))
        return rc;
    const auto t1 = std::chrono::steady_clock::now();
    rc = topn_batches(h, call.c_str(), P, h->dQ.as<const float>(), h->cfg.n_items, users, n_users, topn, ex, CosineScale{},
                      temp, out_items, out_scores, cand ? &cl : nullptr);
    // (both halves end in a synchronise: mfsgd_debug_serve_seconds)
    h->serve_lists_s = std::chrono::duration<double>(t1 - t0).count();
    h->serve_topn_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return rc;
}

// Body of the similar calls: the neighbours of n query rows among the rows of one side's matrix M (Q for
// MFSGD_SIDE_ITEMS, P for MFSGD_SIDE_USERS) under the cosine of DESIGN.md section 3.  host_rows == nullptr: the queries
// are the rows queries[...] of M itself, and with self_excl each leaves out its own index: a one-item exclusion list per
// distinct query, so the EXCL variants of recommend.hip do it.  Otherwise the queries are host_rows (n_rows x k, dense),
// uploaded for the length of the call, queries[...] index them, and nothing is excluded.  The inverse norms are
// computed here, per call; nothing stays in the handle.  `name` is the call's, without the colon.
static int similar_core(mfsgd_handle* h, const char* name, int32_t side, const float* host_rows, int32_t n_rows,
                        const int32_t* queries, int32_t n, int32_t topn, bool self_excl, int32_t* out_index,
                        float* out_scores) {
    const std::string call = std::string(name) + ": ";
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n is negative");
    if (topn < 1) return fail(h, MFSGD_ERR_INVALID_ARG, call + "topn is below 1");
    if (n > 0 && (!queries || !out_index || !out_scores))
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "the queries or an output array is null");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    const int32_t size = side == MFSGD_SIDE_ITEMS ? h->cfg.n_items : h->cfg.n_users;
    if (topn > size)
        return fail(h, MFSGD_ERR_INVALID_ARG,
                    call + "topn exceeds the number of " + (side == MFSGD_SIDE_ITEMS ? "items" : "users"));
    for (int32_t j = 0; j < n; ++j)
        if (queries[j] < 0 || queries[j] >= n_rows)
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "query " + std::to_string(j) + " out of range");
    if (n == 0) return MFSGD_OK;
    if (h->where == mfsgd_handle::Where::None)  // (asked here: factors_to_device wants a device first)
        return fail(h, MFSGD_ERR_STATE, call + "factors not initialised");
    int rc;
    if (side == MFSGD_SIDE_ITEMS && (rc = check_has_q(h, name))) return rc;  // (the users' side reads P alone)
    if ((rc = factors_to_device(h))) return rc;
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    DevBuf d_rows, d_ra, d_rb, ex_slot, ex_off, ex_items, temp;
    const float* M = side == MFSGD_SIDE_ITEMS ? h->dQ.as<const float>() : h->dP.as<const float>();
    const float* A = M;
    if (host_rows && (rc = upload_rows(h, host_rows, n_rows, d_rows, &A))) return rc;
    CosineScale cs;
    if ((rc = dev_alloc(h, d_rb, sizeof(float) * (size_t)size))) return rc;
    HIPCHK_OR(bad, launch_row_inv_norms(h->geo.L, M, size, d_rb.as<float>(), h->stream));
    cs.ra = cs.rb = d_rb.as<const float>();
    if (host_rows) {
        if ((rc = dev_alloc(h, d_ra, sizeof(float) * (size_t)n_rows))) return rc;
        HIPCHK_OR(bad, launch_row_inv_norms(h->geo.L, A, n_rows, d_ra.as<float>(), h->stream));
        cs.ra = d_ra.as<const float>();
    }
    RecommendExcl ex;
    if (self_excl) {
        // a slot per distinct query (one asked for twice shares it); the list of slot s is the query itself
        std::vector<int32_t> slot_of_row((size_t)n_rows, -1), self;
        for (int32_t j = 0; j < n; ++j)
            if (slot_of_row[(size_t)queries[j]] < 0) {
                slot_of_row[(size_t)queries[j]] = (int32_t)self.size();
                self.push_back(queries[j]);
            }
        std::vector<long long> off(self.size() + 1);
        for (size_t x = 0; x < off.size(); ++x) off[x] = (long long)x;
        if ((rc = upload(h, ex_slot, slot_of_row))) return rc;
        if ((rc = upload(h, ex_off, off))) return rc;
        if ((rc = upload(h, ex_items, self))) return rc;
        ex.slot = ex_slot.as<const int32_t>();
        ex.off = ex_off.as<const long long>();
        ex.items = ex_items.as<const int32_t>();
    }
    return topn_batches(h, call.c_str(), A, M, size, queries, n, topn, ex, cs, temp, out_index, out_scores);
}

// Pairs of one rank launch (whole users; a single user with more is a launch of its own): 16 MB of items up, as much
// of ranks down
constexpr int64_t kRankChunk = (int64_t)1 << 22;

// Body of the rank calls, generic over the row matrix as recommend_core is: "user j" is row j of a matrix of n_rows
// rows, the model's P (host_rows == nullptr) or host_rows (n_rows x k, dense).  The pairs are grouped by distinct
// user on the host (counting sort; one slot per user, the slot numbering the exclusion lists use too), go up in
// bounded pieces of whole users, and the ranks come back to the places of the pairs as given.
// `what` is how the call speaks of itself (kRank for every call with a pair list).  unseen: the exclusion lists are those
// of the handle's seen-item index, which the kernel reaches through each slot's user (the _unseen calls: no pairs, the
// model's P).
static int rank_core(mfsgd_handle* h, const ServeName& what, const float* host_rows, int32_t n_rows, const int32_t* users,
                     const int32_t* items, int64_t n, const int32_t* excl_u, const int32_t* excl_i, int64_t n_excl,
                     int32_t* out_rank, bool unseen = false) {
    const std::string call = std::string(what.call) + ": ";
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n is negative");
    if (n_excl < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_excl is negative");
    if (n > 0 && (!users || !items || !out_rank))
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "users, items or out_rank is null");
    if (n_excl > 0 && (!excl_u || !excl_i)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "an exclusion array is null");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    if (unseen && !h->seen.present) return fail(h, MFSGD_ERR_STATE, call + "no seen set");
    const int32_t I = h->cfg.n_items;
    for (int64_t x = 0; x < n; ++x)
        if (users[x] < 0 || users[x] >= n_rows || items[x] < 0 || items[x] >= I)
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "pair " + std::to_string(x) + " out of range");
    // a slot per distinct user, and how many exclusion pairs are theirs
    std::vector<int32_t> slot_of_user((size_t)n_rows, -1), row_of_slot;
    std::vector<long long> off{0};
    for (int64_t x = 0; x < n; ++x) {
        int32_t& s = slot_of_user[(size_t)users[x]];
        if (s < 0) {
            s = (int32_t)row_of_slot.size();
            row_of_slot.push_back(users[x]);
            off.push_back(0);
        }
        ++off[(size_t)s + 1];
    }
    const int32_t n_slots = (int32_t)row_of_slot.size();
    // The slots in the order of their pair counts, most first: a workgroup takes neighbouring slots and passes over Q
    // once per round of its user with the most pairs, so users with many pairs belong together.
    {
        std::vector<int32_t> order((size_t)n_slots);
        for (int32_t s = 0; s < n_slots; ++s) order[(size_t)s] = s;
        std::stable_sort(order.begin(), order.end(),
                         [&off](int32_t a, int32_t b) { return off[(size_t)a + 1] > off[(size_t)b + 1]; });
        std::vector<int32_t> rows_sorted((size_t)n_slots);
        std::vector<long long> off_sorted((size_t)n_slots + 1, 0);
        for (int32_t s = 0; s < n_slots; ++s) {
            rows_sorted[(size_t)s] = row_of_slot[(size_t)order[(size_t)s]];
            off_sorted[(size_t)s + 1] = off[(size_t)order[(size_t)s] + 1];
            slot_of_user[(size_t)rows_sorted[(size_t)s]] = s;
        }
        row_of_slot.swap(rows_sorted);
        off.swap(off_sorted);
    }
    int64_t kept = 0;
    int rc = count_exclusions(h, what, slot_of_user, n_rows, excl_u, excl_i, n_excl, &kept);
    if (rc) return rc;
    if (n == 0) return MFSGD_OK;
    if (h->where == mfsgd_handle::Where::None)  // (asked here: factors_to_device wants a device first)
        return fail(h, MFSGD_ERR_STATE, call + "factors not initialised");
    if ((rc = check_has_q(h, what.call)) || (rc = factors_to_device(h))) return rc;
    // counting sort: the pairs of slot s at off[s] .. off[s + 1], in the order given; place[x] = where pair x went
    for (int32_t s = 0; s < n_slots; ++s) off[(size_t)s + 1] += off[(size_t)s];
    std::vector<int32_t> grouped((size_t)n), ranks((size_t)n);
    std::vector<int64_t> place((size_t)n);
    {
        std::vector<long long> next(off.begin(), off.end() - 1);
        for (int64_t x = 0; x < n; ++x) {
            place[(size_t)x] = next[(size_t)slot_of_user[(size_t)users[x]]]++;
            grouped[(size_t)place[(size_t)x]] = items[x];
        }
    }
    std::vector<int32_t> cut{0};
    int64_t max_pairs = 0;
    for (int32_t s = 0; s < n_slots;) {
        int32_t s1 = s + 1;
        while (s1 < n_slots && off[(size_t)s1 + 1] - off[(size_t)s] <= kRankChunk) ++s1;
        max_pairs = std::max<int64_t>(max_pairs, off[(size_t)s1] - off[(size_t)s]);
        cut.push_back(s1);
        s = s1;
    }
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    DevBuf d_rows, d_slot_rows, d_off, d_items, d_out, ex_slot, ex_off, ex_items, temp;
    const float* P;
    if ((rc = upload_rows(h, host_rows, n_rows, d_rows, &P))) return rc;
    RecommendExcl ex;  // built once for all launches; none when no pair belongs to a user asked about
    if (unseen) ex = h->seen.excl();  // (none when the index is empty)
    if (kept > 0 && (rc = exclusions_to_device(h, what, slot_of_user, n_slots, excl_u, excl_i, n_excl, kept, ex_slot, ex_off,
                                               ex_items, temp, ex)))
        return rc;
    if ((rc = upload(h, d_slot_rows, row_of_slot))) return rc;
    if ((rc = upload(h, d_off, off))) return rc;
    if ((rc = dev_alloc(h, d_items, sizeof(int32_t) * (size_t)max_pairs))) return rc;
    if ((rc = dev_alloc(h, d_out, sizeof(int32_t) * (size_t)max_pairs))) return rc;
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
        const int32_t b0 = cut[b], nb = cut[b + 1] - b0;
        const long long base = off[(size_t)b0];
        const size_t bytes = sizeof(int32_t) * (size_t)(off[(size_t)(b0 + nb)] - base);
        RecommendExcl exb = ex;
        if (exb.off && !unseen) exb.off += b0;  // (the index is reached by user, not by slot)
        HIPCHK_OR(bad, hipMemcpyAsync(d_items.get(), grouped.data() + base, bytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, launch_rank_items(h->geo.L, P, h->dQ.as<const float>(), d_slot_rows.as<const int32_t>() + b0, nb,
                                         d_off.as<const long long>() + b0, base, d_items.as<const int32_t>(), I, exb,
                                         d_out.as<int32_t>(), h->stream, unseen));
        HIPCHK_OR(bad, hipMemcpyAsync(ranks.data() + base, d_out.get(), bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // the staging buffers are reused
    }
    for (int64_t x = 0; x < n; ++x) out_rank[x] = ranks[(size_t)place[(size_t)x]];
    return MFSGD_OK;
}

static int metrics_fail(int code, const std::string& msg) {
    g_create_error = "ranking_metrics: " + msg;
    return code;
}

// Ratings of one fold-in batch (whole lists; a single list longer than this is a batch of its own): 32 MB of staging
constexpr int64_t kFoldChunk = (int64_t)1 << 22;
constexpr int64_t kFoldRows = (int64_t)1 << 20;  // ... and its new rows, so that a run of empty lists is bounded too

// Body of the fold-in calls: n_new rows of one side against the fixed factors of the other.  `fixed` says where those
// are once the factors are on the device (asked then, not before: the upload creates them), n_fixed is their row
// count, and `what` how the call speaks of itself, of a new row and of an id.
struct FoldName {
    const char* call;   // "fold_in"
    const char* row;    // "user": what a new row is
    const char* id;     // "item": what a rating names on the fixed side
    const char* ids;    // "items"
};
constexpr FoldName kFoldInUsers{"fold_in", "user", "item", "items"}, kFoldInItems{"fold_in_items", "item", "user", "users"};

static int fold_in_core(mfsgd_handle* h, const FoldName& what, const DevBuf mfsgd_handle::*fixed, int32_t n_fixed, int32_t n_new,
                        const int64_t* row_ptr, const int32_t* ids, const float* ratings, int32_t epochs, const float* init_rows,
                        int64_t seed, float* out_rows) {
    const std::string call = std::string(what.call) + ": ";
    if (n_new < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_new is negative");
    if (epochs < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "epochs is negative");
    if (n_new > 0 && (!row_ptr || !out_rows)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr or out_rows is null");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    if (h->where == mfsgd_handle::Where::None)  // (asked here: factors_to_device wants a device first)
        return fail(h, MFSGD_ERR_STATE, call + "factors not initialised");
    if (const int rc = check_has_q(h, what.call)) return rc;
    if (n_new == 0) return MFSGD_OK;
    if (row_ptr[0] != 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr[0] is not 0");
    for (int32_t x = 0; x < n_new; ++x)
        if (row_ptr[x + 1] < row_ptr[x])
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr decreases at " + what.row + " " + std::to_string(x));
    const int64_t total = row_ptr[n_new];
    if (total > 0 && (!ids || !ratings)) return fail(h, MFSGD_ERR_INVALID_ARG, call + what.ids + " or ratings is null");
    for (int64_t j = 0; j < total; ++j)
        if (ids[j] < 0 || ids[j] >= n_fixed)
            return fail(h, MFSGD_ERR_INVALID_ARG, call + what.id + " of rating " + std::to_string(j) + " out of range");
    int rc = factors_to_device(h);
    if (rc) return rc;
    const int k = h->cfg.k;
    // batches of whole lists, in the caller's order, so that each batch is one contiguous piece of ids / ratings
    std::vector<int32_t> cut{0};
    int64_t max_ratings = 0, max_rows = 0;
    for (int32_t x0 = 0; x0 < n_new;) {
        int32_t x1 = x0 + 1;
        while (x1 < n_new && x1 - x0 < kFoldRows && row_ptr[x1 + 1] - row_ptr[x0] <= kFoldChunk) ++x1;
        max_ratings = std::max<int64_t>(max_ratings, row_ptr[x1] - row_ptr[x0]);
        max_rows = std::max<int64_t>(max_rows, x1 - x0);
        cut.push_back(x1);
        x0 = x1;
    }
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    DevBuf d_rows, d_ptr, d_perm, d_ids, d_r;
    const size_t row_bytes = sizeof(float) * (size_t)n_new * (size_t)k;
    if ((rc = dev_alloc(h, d_rows, row_bytes))) return rc;
    if (epochs > 0 && total > 0) {
        if ((rc = dev_alloc(h, d_ptr, sizeof(int64_t) * ((size_t)max_rows + 1)))) return rc;
        if ((rc = dev_alloc(h, d_perm, sizeof(int32_t) * (size_t)max_rows))) return rc;
        if ((rc = dev_alloc(h, d_ids, sizeof(int32_t) * (size_t)max_ratings))) return rc;
        if ((rc = dev_alloc(h, d_r, sizeof(float) * (size_t)max_ratings))) return rc;
    }
    // the start rows, dense: the kernel pads them to kp in its registers
    if (init_rows)
        HIPCHK_OR(bad, hipMemcpyAsync(d_rows.get(), init_rows, row_bytes, hipMemcpyHostToDevice, h->stream));
    else
        HIPCHK_OR(bad, launch_init_rows(d_rows.as<float>(), n_new, k, k, seed, 0, (float)(1.0 / std::sqrt((double)k)), h->stream));
    std::vector<int32_t> perm;
    for (size_t b = 0; b + 1 < cut.size() && epochs > 0; ++b) {
        const int32_t x0 = cut[b], nb = cut[b + 1] - cut[b];
        const int64_t base = row_ptr[x0], nr = row_ptr[x0 + nb] - base;
        if (nr == 0) continue;
        // longest first: a wave runs as long as its longest list
        perm.resize((size_t)nb);
        for (int32_t x = 0; x < nb; ++x) perm[(size_t)x] = x;
        const int64_t* rp = row_ptr + x0;
        std::stable_sort(perm.begin(), perm.end(), [rp](int32_t a, int32_t b2) { return rp[a + 1] - rp[a] > rp[b2 + 1] - rp[b2]; });
        HIPCHK_OR(bad, hipMemcpyAsync(d_ptr.get(), rp, sizeof(int64_t) * ((size_t)nb + 1), hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, hipMemcpyAsync(d_perm.get(), perm.data(), sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, hipMemcpyAsync(d_ids.get(), ids + base, sizeof(int32_t) * (size_t)nr, hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, hipMemcpyAsync(d_r.get(), ratings + base, sizeof(float) * (size_t)nr, hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, launch_fold_in(h->geo.L, (h->*fixed).as<const float>(), d_rows.as<float>() + (size_t)x0 * k, k,
                                      d_ptr.as<const long long>(), base, d_perm.as<const int32_t>(), nb,
                                      d_ids.as<const int32_t>(), d_r.as<const float>(), epochs, h->cfg.lr,
                                      1.0f - h->cfg.lr * h->cfg.lambda, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // perm and the staging buffers are reused
    }
    HIPCHK_OR(bad, hipMemcpyAsync(out_rows, d_rows.get(), row_bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

}  // namespace mfsgd

using namespace mfsgd;

extern "C" {

int mfsgd_predict(mfsgd_handle* h, const int32_t* u, const int32_t* i, float* out, int64_t n) {
    return guarded(h, "predict", [&]() -> int {
        if (n < 0 || (n > 0 && (!u || !i || !out))) return fail(h, MFSGD_ERR_INVALID_ARG, "predict: bad argument");
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "predict: single-partition handles only");
        for (int64_t j = 0; j < n; ++j)
            if (u[j] < 0 || u[j] >= h->cfg.n_users || i[j] < 0 || i[j] >= h->cfg.n_items)
                return fail(h, MFSGD_ERR_INVALID_ARG, "predict: pair " + std::to_string(j) + " out of range");
        if (n == 0) return MFSGD_OK;
        int rc = check_has_q(h, "predict");
        if (rc || (rc = factors_to_device(h))) return rc;
        DevBuf du, di, dout;
        if ((rc = dev_alloc(h, du, sizeof(int32_t) * (size_t)n))) return rc;
        if ((rc = dev_alloc(h, di, sizeof(int32_t) * (size_t)n))) return rc;
        if ((rc = dev_alloc(h, dout, sizeof(float) * (size_t)n))) return rc;
        // (this call has always reported every HIP failure as MFSGD_ERR_HIP and left the runtime's error word alone)
        auto bad = [h](hipError_t e) { return fail(h, MFSGD_ERR_HIP, std::string("predict: ") + hipGetErrorString(e)); };
        HIPCHK_OR(bad, hipMemcpyAsync(du.get(), u, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, hipMemcpyAsync(di.get(), i, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIPCHK_OR(bad, launch_predict(h->geo.L, h->dP.as<const float>(), h->dQ.as<const float>(), du.as<const int32_t>(),
                                      di.as<const int32_t>(), dout.as<float>(), n, h->stream));
        HIPCHK_OR(bad, hipMemcpyAsync(out, dout.get(), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
        return MFSGD_OK;
    });
}

int mfsgd_recommend(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, int32_t* out_items,
                    float* out_scores) {
    return guarded(h, "recommend", [&]() -> int {
        return recommend_core(h, kRecommend, "recommend", nullptr, h->cfg.n_users, users, n_users, topn, nullptr, nullptr, nullptr,
                              0, out_items, out_scores);
    });
}

int mfsgd_recommend_excluding(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, const int32_t* excl_u,
                              const int32_t* excl_i, int64_t n_excl, int32_t* out_items, float* out_scores) {
    return guarded(h, "recommend", [&]() -> int {
        return recommend_core(h, kRecommend, "recommend", nullptr, h->cfg.n_users, users, n_users, topn, nullptr, excl_u, excl_i,
                              n_excl, out_items, out_scores);
    });
}

int mfsgd_recommend_rows(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn, const int32_t* excl_row,
                         const int32_t* excl_item, int64_t n_excl, int32_t* out_items, float* out_scores) {
    return guarded(h, "recommend_rows", [&]() -> int {
        if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(h, MFSGD_ERR_INVALID_ARG, "recommend_rows: bad argument");
        std::vector<int32_t> all((size_t)n_rows);
        for (int32_t j = 0; j < n_rows; ++j) all[(size_t)j] = j;
        return recommend_core(h, kRecommend, "recommend_rows", rows, n_rows, all.data(), n_rows, topn, nullptr, excl_row,
                              excl_item, n_excl, out_items, out_scores);
    });
}

int mfsgd_recommend_among(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, const int64_t* cand_ptr,
                          const int32_t* cand_items, int64_t n_cand, const int32_t* excl_u, const int32_t* excl_i,
                          int64_t n_excl, int32_t* out_items, float* out_scores) {
    return guarded(h, "recommend_among", [&]() -> int {
        const Candidates cand{cand_ptr, cand_items, n_cand};
        return recommend_core(h, kAmong, kAmong.call, nullptr, h->cfg.n_users, users, n_users, topn, &cand, excl_u, excl_i,
                              n_excl, out_items, out_scores);
    });
}

int mfsgd_recommend_rows_among(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn, const int64_t* cand_ptr,
                               const int32_t* cand_items, int64_t n_cand, const int32_t* excl_row, const int32_t* excl_item,
                               int64_t n_excl, int32_t* out_items, float* out_scores) {
    return guarded(h, "recommend_rows_among", [&]() -> int {
        if (n_rows < 0 || (n_rows > 0 && !rows)) return fail(h, MFSGD_ERR_INVALID_ARG, "recommend_rows_among: bad argument");
        std::vector<int32_t> all((size_t)n_rows);
        for (int32_t j = 0; j < n_rows; ++j) all[(size_t)j] = j;
        const Candidates cand{cand_ptr, cand_items, n_cand};
        return recommend_core(h, kRowsAmong, kRowsAmong.call, rows, n_rows, all.data(), n_rows, topn, &cand, excl_row, excl_item,
                              n_excl, out_items, out_scores);
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
        if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "row_inv_norms: single-partition handles only");
        if (h->where == mfsgd_handle::Where::None)  // (asked here: factors_to_device wants a device first)
            return fail(h, MFSGD_ERR_STATE, "row_inv_norms: factors not initialised");
        int rc = side == MFSGD_SIDE_ITEMS ? check_has_q(h, "row_inv_norms") : MFSGD_OK;
        if (rc || (rc = factors_to_device(h))) return rc;
        const int32_t size = side == MFSGD_SIDE_ITEMS ? h->cfg.n_items : h->cfg.n_users;
        const float* M = side == MFSGD_SIDE_ITEMS ? h->dQ.as<const float>() : h->dP.as<const float>();
        auto bad = [h](hipError_t e) { return serve_fail(h, "row_inv_norms: ", e); };
        DevBuf d_rn;
        if ((rc = dev_alloc(h, d_rn, sizeof(float) * (size_t)size))) return rc;
        HIPCHK_OR(bad, launch_row_inv_norms(h->geo.L, M, size, d_rn.as<float>(), h->stream));
        HIPCHK_OR(bad, hipMemcpyAsync(out, d_rn.get(), sizeof(float) * (size_t)size, hipMemcpyDeviceToHost, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
        return MFSGD_OK;
    });
}

int mfsgd_similar_items(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn, int32_t* out_items,
                        float* out_scores) {
    return guarded(h, "similar_items", [&]() -> int {
        return similar_core(h, "similar_items", MFSGD_SIDE_ITEMS, nullptr, h->cfg.n_items, items, n, topn, true, out_items,
                            out_scores);
    });
}

int mfsgd_similar_users(mfsgd_handle* h, const int32_t* users, int32_t n, int32_t topn, int32_t* out_users,
                        float* out_scores) {
    return guarded(h, "similar_users", [&]() -> int {
        return similar_core(h, "similar_users", MFSGD_SIDE_USERS, nullptr, h->cfg.n_users, users, n, topn, true, out_users,
                            out_scores);
    });
}

int mfsgd_similar_rows(mfsgd_handle* h, int32_t side, const float* rows, int32_t n_rows, int32_t topn, int32_t* out_index,
                       float* out_scores) {
    return guarded(h, "similar_rows", [&]() -> int {
        if (side != MFSGD_SIDE_USERS && side != MFSGD_SIDE_ITEMS)
            return fail(h, MFSGD_ERR_INVALID_ARG, "similar_rows: side is neither MFSGD_SIDE_USERS nor MFSGD_SIDE_ITEMS");
        if (n_rows < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "similar_rows: n_rows is negative");
        if (n_rows > 0 && !rows) return fail(h, MFSGD_ERR_INVALID_ARG, "similar_rows: rows is null");
        std::vector<int32_t> all((size_t)n_rows);
        for (int32_t j = 0; j < n_rows; ++j) all[(size_t)j] = j;
        return similar_core(h, "similar_rows", side, rows, n_rows, all.data(), n_rows, topn, false, out_index, out_scores);
    });
}

int mfsgd_rank_items(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, const int32_t* excl_u,
                     const int32_t* excl_i, int64_t n_excl, int32_t* out_rank) {
    return guarded(h, "rank_items", [&]() -> int {
        return rank_core(h, kRank, nullptr, h->cfg.n_users, users, items, n, excl_u, excl_i, n_excl, out_rank);
    });
}

int mfsgd_rank_items_rows(mfsgd_handle* h, const float* rows, int32_t n_rows, const int32_t* row_of_pair,
                          const int32_t* items, int64_t n, const int32_t* excl_row, const int32_t* excl_item,
                          int64_t n_excl, int32_t* out_rank) {
    return guarded(h, "rank_items", [&]() -> int {
        if (n_rows < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "rank_items: n_rows is negative");
        if (n_rows > 0 && !rows) return fail(h, MFSGD_ERR_INVALID_ARG, "rank_items: rows is null");
        return rank_core(h, kRank, rows, n_rows, row_of_pair, items, n, excl_row, excl_item, n_excl, out_rank);
    });
}

int mfsgd_ranking_metrics_from_ranks(const int32_t* users, const int32_t* ranks, int64_t n, int32_t topn,
                                     mfsgd_ranking_metrics* out) {
    return guarded_free("ranking_metrics", [&]() -> int {
        if (!out) return metrics_fail(MFSGD_ERR_INVALID_ARG, "out is null");
        if (n < 0) return metrics_fail(MFSGD_ERR_INVALID_ARG, "n is negative");
        if (topn < 1) return metrics_fail(MFSGD_ERR_INVALID_ARG, "topn is below 1");
        if (n > 0 && (!users || !ranks)) return metrics_fail(MFSGD_ERR_INVALID_ARG, "users or ranks is null");
        for (int64_t x = 0; x < n; ++x)
            if (ranks[x] < 0) return metrics_fail(MFSGD_ERR_INVALID_ARG, "rank " + std::to_string(x) + " is negative");
        *out = mfsgd_ranking_metrics{};
        out->n_pairs = n;
        if (n == 0) return MFSGD_OK;
        // ascending user, and inside a user ascending rank: every sum below has one order whatever the caller's was
        std::vector<std::pair<int32_t, int32_t>> ur((size_t)n);
        for (int64_t x = 0; x < n; ++x) ur[(size_t)x] = {users[x], ranks[x]};
        std::sort(ur.begin(), ur.end());
        std::vector<double> idcg{0.0};  // [m]: the DCG of m hits in the first m places
        double hit = 0, prec = 0, rec = 0, ndcg = 0, mrr = 0;
        int64_t n_users = 0;
        for (size_t a = 0; a < ur.size();) {
            size_t b = a;
            int64_t hits = 0;
            double dcg = 0.0;
            for (; b < ur.size() && ur[b].first == ur[a].first; ++b)
                if (ur[b].second < topn) {
                    ++hits;
                    dcg += 1.0 / std::log2((double)ur[b].second + 2.0);
                }
            const size_t m = std::min<size_t>(b - a, (size_t)topn);
            while (idcg.size() <= m) idcg.push_back(idcg.back() + 1.0 / std::log2((double)idcg.size() + 1.0));
            hit += hits > 0 ? 1.0 : 0.0;
            prec += (double)hits / (double)topn;
            rec += (double)hits / (double)(b - a);
            ndcg += dcg / idcg[m];
            mrr += 1.0 / ((double)ur[a].second + 1.0);  // (the user's lowest rank comes first)
            ++n_users;
            a = b;
        }
        out->n_users = n_users;
        out->hit_rate = hit / (double)n_users;
        out->precision = prec / (double)n_users;
        out->recall = rec / (double)n_users;
        out->ndcg = ndcg / (double)n_users;
        out->mrr = mrr / (double)n_users;
        return MFSGD_OK;
    });
}

// Body of the evaluate calls: rank_core, then the metrics of its ranks.
static int evaluate_core(mfsgd_handle* h, const ServeName& what, const int32_t* users, const int32_t* items, int64_t n,
                         int32_t topn, const int32_t* excl_u, const int32_t* excl_i, int64_t n_excl, mfsgd_ranking_metrics* out,
                         int32_t* out_rank, bool unseen) {
    const std::string call = std::string(what.call) + ": ";
    if (topn < 1) return fail(h, MFSGD_ERR_INVALID_ARG, call + "topn is below 1");
    if (!out) return fail(h, MFSGD_ERR_INVALID_ARG, call + "the metrics struct is null");
    std::vector<int32_t> own;
    if (!out_rank && n > 0) {
        own.resize((size_t)n);
        out_rank = own.data();
    }
    int rc = rank_core(h, what, nullptr, h->cfg.n_users, users, items, n, excl_u, excl_i, n_excl, out_rank, unseen);
    if (rc) return rc;
    rc = mfsgd_ranking_metrics_from_ranks(users, out_rank, n, topn, out);
    if (rc) return fail(h, rc, g_create_error);
    return MFSGD_OK;
}

int mfsgd_evaluate_ranking(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t topn,
                           const int32_t* excl_u, const int32_t* excl_i, int64_t n_excl, mfsgd_ranking_metrics* out,
                           int32_t* out_rank) {
    return guarded(h, "rank_items", [&]() -> int {
        return evaluate_core(h, kRank, users, items, n, topn, excl_u, excl_i, n_excl, out, out_rank, false);
    });
}

int mfsgd_recommend_unseen(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, int32_t* out_items,
                           float* out_scores) {
    return guarded(h, kUnseen.call, [&]() -> int {
        return recommend_core(h, kUnseen, kUnseen.call, nullptr, h->cfg.n_users, users, n_users, topn, nullptr, nullptr, nullptr, 0,
                              out_items, out_scores, true);
    });
}

int mfsgd_recommend_unseen_among(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, const int64_t* cand_ptr,
                                 const int32_t* cand_items, int64_t n_cand, int32_t* out_items, float* out_scores) {
    return guarded(h, kUnseenAmong.call, [&]() -> int {
        const Candidates cand{cand_ptr, cand_items, n_cand};
        return recommend_core(h, kUnseenAmong, kUnseenAmong.call, nullptr, h->cfg.n_users, users, n_users, topn, &cand, nullptr,
                              nullptr, 0, out_items, out_scores, true);
    });
}

int mfsgd_rank_items_unseen(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t* out_rank) {
    return guarded(h, kRankUnseen.call, [&]() -> int {
        return rank_core(h, kRankUnseen, nullptr, h->cfg.n_users, users, items, n, nullptr, nullptr, 0, out_rank, true);
    });
}

int mfsgd_evaluate_ranking_unseen(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t topn,
                                  mfsgd_ranking_metrics* out, int32_t* out_rank) {
    return guarded(h, kEvaluateUnseen.call, [&]() -> int {
        return evaluate_core(h, kEvaluateUnseen, users, items, n, topn, nullptr, nullptr, 0, out, out_rank, true);
    });
}

int mfsgd_fold_in_users(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* items, const float* ratings,
                        int32_t epochs, const float* init_rows, int64_t seed, float* out_rows) {
    return guarded(h, "fold_in", [&]() -> int {
        return fold_in_core(h, kFoldInUsers, &mfsgd_handle::dQ, h->cfg.n_items, n_new, row_ptr, items, ratings, epochs, init_rows, seed,
                            out_rows);
    });
}

int mfsgd_fold_in_items(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* users, const float* ratings,
                        int32_t epochs, const float* init_rows, int64_t seed, float* out_rows) {
    return guarded(h, "fold_in_items", [&]() -> int {
        return fold_in_core(h, kFoldInItems, &mfsgd_handle::dP, h->cfg.n_users, n_new, row_ptr, users, ratings, epochs, init_rows, seed,
                            out_rows);
    });
}

}  // extern "C"
