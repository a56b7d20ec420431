// serve.cpp -- what a trained model answers: predictions, top-N recommendations, cosine neighbours of items and users,
// ranks of held-out items and their metrics, and the fold-in of new users and new items.  Every call batches its work
// through bounded staging buffers.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <numeric>

#include "handle.hpp"
#include "serve_util.hpp"

namespace mfsgd {

// How a serving call speaks of itself and of the users it was given, in the messages the two cores share; and (the
// top-N calls) of one request row and of the side that is scanned, which are the other way round for recommend_users.
struct ServeName {
    const char* call;
    const char* whose;
    const char* row = "user";
    const char* scanned = "items";
};
constexpr ServeName kRecommend{"recommend", "the requested users"}, kRank{"rank_items", "the users asked about"};
constexpr ServeName kAmong{"recommend_among", "the requested users"}, kRowsAmong{"recommend_rows_among", "the rows"};
// ... and the calls that exclude what the handle's seen-item index holds instead of a pair list
constexpr ServeName kUnseen{"recommend_unseen", "the requested users"}, kUnseenAmong{"recommend_unseen_among", "the requested users"};
constexpr ServeName kRankUnseen{"rank_items_unseen", "the users asked about"};
constexpr ServeName kEvaluateUnseen{"evaluate_ranking_unseen", "the users asked about"};
// ... and the item-side calls: the request rows are items (or item rows of the caller's), the users are scanned
constexpr ServeName kUsers{"recommend_users", "the requested items", "item", "users"};
constexpr ServeName kUsersAmong{"recommend_users_among", "the requested items", "item", "users"};
constexpr ServeName kUsersUnseen{"recommend_users_unseen", "the requested items", "item", "users"};
constexpr ServeName kUsersUnseenAmong{"recommend_users_unseen_among", "the requested items", "item", "users"};
constexpr ServeName kUsersRows{"recommend_users_rows", "the rows", "item", "users"};
constexpr ServeName kUsersRowsAmong{"recommend_users_rows_among", "the rows", "item", "users"};

// What a serving call leaves out: nothing, the pairs (u[x], i[x]) of a list of the caller's, or (the _unseen calls) what
// the handle's seen-item index holds, which is read where it lies -- nothing is built, uploaded or looped over for it.
// In the cores u[x] is a row of the request side and i[x] one of the scanned side: an item-side call hands its
// (user, item) arrays over exchanged, and from there on a pair list is a pair list.  The index, CSR by user, cannot
// be read where it lies for an item: the lists of the requested items are made of it per call (audience.hip).
struct Exclusions {
    enum { kNone, kPairs, kSeen } from = kNone;
    const int32_t *u = nullptr, *i = nullptr;
    int64_t n = 0;
    static Exclusions pairs(const int32_t* u, const int32_t* i, int64_t n) { return {kPairs, u, i, n}; }
    static Exclusions seen() { return {kSeen, nullptr, nullptr, 0}; }
};

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

// A rank call over the same kind of row matrix: the n pairs (users[x], items[x]), and where their ranks go.
struct RankRequest {
    const float* host_rows = nullptr;
    int32_t n_rows = 0;
    const int32_t *users = nullptr, *items = nullptr;
    int64_t n = 0;
    Exclusions excl;
    int32_t* out_rank = nullptr;
};

// Rows 0 .. n - 1, all of them: what the _rows calls ask for.
static std::vector<int32_t> all_rows(int32_t n) {
    std::vector<int32_t> all((size_t)n);
    std::iota(all.begin(), all.end(), 0);
    return all;
}

// The row matrix of a serving call on the device: the model's P (`own`: or its Q, for an item-side call), or host_rows
// (n_rows x k, dense), which goes up into a kp-padded temporary (`buf`) for the length of the call.
static int upload_rows(mfsgd_handle* h, const float* host_rows, int32_t n_rows, DevArray<float>& buf, const float** rows,
                       const DevArray<float> mfsgd_handle::*own = &mfsgd_handle::dP) {
    *rows = (h->*own).data();
    if (!host_rows) return MFSGD_OK;
    const int k = h->cfg.k, kp = h->geo.kp;
    std::vector<float> padded((size_t)n_rows * kp, 0.0f);
    for (int64_t x = 0; x < n_rows; ++x) std::memcpy(&padded[(size_t)x * kp], host_rows + x * k, sizeof(float) * (size_t)k);
    const int rc = upload(h, buf, padded);
    *rows = buf.data();
    return rc;
}

// Range check of the exclusion pairs (n_scanned: the rows of the scanned side, the model's items unless the call is an
// item-side one), and *kept = how many of them belong to a user that has a slot.
static int count_exclusions(const mfsgd_handle* h, const ServeName& what, const std::vector<int32_t>& slot_of_user, int32_t n_rows,
                            int32_t n_scanned, const Exclusions& excl, int64_t* kept) {
    *kept = 0;
    for (int64_t x0 = 0; x0 < excl.n; x0 += 4096) {  // (block by block: the pairs are read from memory once)
        const int64_t x1 = std::min(excl.n, x0 + 4096), x = first_outside(excl.u + x0, n_rows, excl.i + x0, n_scanned, x1 - x0);
        if (x >= 0)
            return fail(h, MFSGD_ERR_INVALID_ARG, std::string(what.call) + ": excluded pair " + std::to_string(x0 + x) + " out of range");
        for (int64_t y = x0; y < x1; ++y) *kept += slot_of_user[(size_t)excl.u[y]] >= 0 ? 1 : 0;
    }
    if (*kept > (int64_t)UINT32_MAX)
        return fail(h, MFSGD_ERR_INVALID_ARG, std::string(what.call) + ": more than 2^32 - 1 excluded pairs of " + what.whose);
    return MFSGD_OK;
}

// The exclusion lists of one call on the device, as RecommendExcl reads them.
struct ExclLists {
    DevArray<int32_t> slot, items;
    DevArray<long long> off;
};

// The keys of one call's exclusion lists on their way there: slot << 32 | id of the scanned side, appended in no
// particular order, then sorted through keys_tmp.  count: [0] appended keys (u64), then the distinct ones (u32).
struct ExclKeys {
    DevArray<unsigned long long> keys, keys_tmp, count;
};

// The slot table on the device and the counter (the caller zeroes it before each pass that appends or counts keys).
static int excl_keys_begin(mfsgd_handle* h, const Slots& slots, ExclLists& lists, ExclKeys& k) {
    const int rc = upload(h, lists.slot, slots.slot_of_row);
    return rc ? rc : dev_alloc(h, k.count, 2);
}

// Room for `kept` keys and for the lists they become: 20 bytes per kept pair (two key buffers and the lists' ids), and
// an offset per slot.
static int excl_keys_alloc(mfsgd_handle* h, const Slots& slots, int64_t kept, ExclLists& lists, ExclKeys& k) {
    int rc;
    if ((rc = dev_alloc(h, k.keys, (size_t)kept)) || (rc = dev_alloc(h, k.keys_tmp, (size_t)kept))) return rc;
    if ((rc = dev_alloc(h, lists.off, (size_t)slots.n() + 1)) || (rc = dev_alloc(h, lists.items, (size_t)kept))) return rc;
    return MFSGD_OK;
}

// The `kept` appended keys sorted and made distinct into one list per slot (recommend.hip), and `ex` pointing into
// `lists`, which is the caller's.  Ends in a synchronise.
static hipError_t excl_keys_to_lists(mfsgd_handle* h, const Slots& slots, int64_t kept, ExclKeys& k, ExclLists& lists, DevBuf& temp,
                                     RecommendExcl& ex) {
    hipError_t e = recommend_excl_lists(k.keys.data(), k.keys_tmp.data(), kept, slots.n(), reinterpret_cast<unsigned*>(k.count.data() + 1),
                                        lists.off.data(), lists.items.data(), temp, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) ex = RecommendExcl{lists.slot.data(), lists.off.data(), lists.items.data()};
    return e;
}

// Exclusion lists of one recommend call on the device: the pairs go up in chunks of bounded size, those of requested
// users are kept (slot << 32 | item), then sorted and made distinct into one list per slot (recommend.hip).
// Scratch lives as long as this function; `ex` points into `lists`, which is the caller's.
// `what` starts the message of a HIP failure: the call the lists are built for.
// (kExclChunk pairs per upload, handle.hpp)
static int exclusions_to_device(mfsgd_handle* h, const ServeName& what, const Slots& slots, const Exclusions& excl, int64_t kept,
                                ExclLists& lists, DevBuf& temp, RecommendExcl& ex) {
    const std::string prefix = std::string(what.call) + ": exclusion lists: ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    DevArray<int32_t> cu, ci;
    ExclKeys k;
    const int64_t chunk = std::min(excl.n, kExclChunk);
    int rc;
    if ((rc = excl_keys_begin(h, slots, lists, k)) || (rc = excl_keys_alloc(h, slots, kept, lists, k))) return rc;
    if ((rc = dev_alloc(h, cu, (size_t)chunk)) || (rc = dev_alloc(h, ci, (size_t)chunk))) return rc;
    HIPCHK_OR(bad, hipMemsetAsync(k.count.data(), 0, 16, h->stream));
    for (int64_t x0 = 0; x0 < excl.n; x0 += chunk) {
        const int64_t c = std::min(chunk, excl.n - x0);
        HIPCHK_OR(bad, copy_up(cu, excl.u + x0, (size_t)c, h->stream));
        HIPCHK_OR(bad, copy_up(ci, excl.i + x0, (size_t)c, h->stream));
        HIPCHK_OR(bad, recommend_excl_filter(lists.slot.data(), cu.data(), ci.data(), c, k.keys.data(), k.count.data(), kept, h->stream));
    }
    HIPCHK_OR(bad, excl_keys_to_lists(h, slots, kept, k, lists, temp, ex));
    return MFSGD_OK;
}

// The same lists for an item-side _unseen call (slots: of the requested items), made of the seen-item index, which is
// CSR by user and cannot be read where it lies for an item: one pass over its pairs counts those of requested items
// -- how many are kept is not known before -- and a second writes them as slot << 32 | user (audience.hip); from there
// they are a caller's pairs.  No pair kept: nothing is built and ex stays empty.  The index's lists are read up to the
// user count (the offsets above it hold the total).  mfsgd_mark_seen keeps an index below 2^32 pairs, so the cap of a
// pair list cannot be met here; it is asked all the same, the lists' counters being 32 bits wide.
static int audience_to_device(mfsgd_handle* h, const ServeName& what, const Slots& slots, const Seen& seen, ExclLists& lists,
                              DevBuf& temp, RecommendExcl& ex) {
    const std::string prefix = std::string(what.call) + ": exclusion lists: ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    ExclKeys k;
    auto pass = [&](unsigned long long* to, int64_t cap) {
        return seen_audience_keys(lists.slot.data(), (int32_t)slots.slot_of_row.size(), seen.off.data(), seen.items.data(),
                                  std::min(h->cfg.n_users, seen.capacity), seen.n, to, k.count.data(), cap, h->stream);
    };
    unsigned long long kept = 0;
    int rc;
    if ((rc = excl_keys_begin(h, slots, lists, k))) return rc;
    HIPCHK_OR(bad, hipMemsetAsync(k.count.data(), 0, 16, h->stream));
    HIPCHK_OR(bad, pass(nullptr, 0));
    HIPCHK_OR(bad, copy_down(&kept, k.count, 1, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    if (kept > (unsigned long long)UINT32_MAX)
        return fail(h, MFSGD_ERR_INVALID_ARG, std::string(what.call) + ": more than 2^32 - 1 excluded pairs of " + what.whose);
    if (kept == 0) return MFSGD_OK;
    if ((rc = excl_keys_alloc(h, slots, (int64_t)kept, lists, k))) return rc;
    HIPCHK_OR(bad, hipMemsetAsync(k.count.data(), 0, 16, h->stream));  // (the counter counts again)
    HIPCHK_OR(bad, pass(k.keys.data(), (int64_t)kept));
    HIPCHK_OR(bad, excl_keys_to_lists(h, slots, (int64_t)kept, k, lists, temp, ex));
    return MFSGD_OK;
}

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
// keys are sorted and made distinct into one ascending list per request row, or into one list.  Scratch lives as long
// as this function; `out` is the caller's.  cand.n > 0.
static int candidates_to_device(mfsgd_handle* h, const ServeName& what, const Candidates& cand, int32_t n_rows, DevBuf& temp,
                                CandLists& out) {
    const std::string prefix = std::string(what.call) + ": candidate lists: ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    DevArray<long long> d_ptr;
    DevArray<int32_t> ci;
    DevArray<unsigned long long> keys, keys_tmp;
    DevArray<unsigned> count;
    const int64_t chunk = std::min(cand.n, kExclChunk);
    const int32_t n_slots = cand.ptr ? n_rows : 1;
    int rc;
    if (cand.ptr) {
        if ((rc = dev_alloc(h, d_ptr, (size_t)n_rows + 1))) return rc;
        HIPCHK_OR(bad, copy_up(d_ptr, cand.ptr, (size_t)n_rows + 1, h->stream));
    }
    if ((rc = dev_alloc(h, ci, (size_t)chunk))) return rc;
    if ((rc = dev_alloc(h, keys, (size_t)cand.n)) || (rc = dev_alloc(h, keys_tmp, (size_t)cand.n))) return rc;
    if ((rc = dev_alloc(h, count, 4))) return rc;  // [0] distinct keys
    if ((rc = dev_alloc(h, out.d_off, (size_t)n_slots + 1)) || (rc = dev_alloc(h, out.d_items, (size_t)cand.n))) return rc;
    for (int64_t x0 = 0; x0 < cand.n; x0 += chunk) {
        const int64_t c = std::min(chunk, cand.n - x0);
        HIPCHK_OR(bad, copy_up(ci, cand.items + x0, (size_t)c, h->stream));
        HIPCHK_OR(bad, recommend_cand_keys(cand.ptr ? d_ptr.data() : nullptr, n_rows, ci.data(), x0, c, keys.data(), h->stream));
    }
    HIPCHK_OR(bad, recommend_excl_lists(keys.data(), keys_tmp.data(), cand.n, n_slots, count.data(), out.d_off.data(),
                                        out.d_items.data(), temp, h->stream));
    out.off.resize((size_t)n_slots + 1);
    HIPCHK_OR(bad, copy_down(out.off.data(), out.d_off, (size_t)n_slots + 1, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
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

// Pairs of one rank launch (whole users; a single user with more is a launch of its own): 16 MB of items up, as much
// of ranks down
constexpr int64_t kRankChunk = (int64_t)1 << 22;

// Body of the rank calls, generic over the row matrix as recommend_core is.  The pairs are grouped by distinct user on
// the host (counting sort; one slot per user, the slot numbering the exclusion lists use too), go up in bounded pieces
// of whole users, and the ranks come back to the places of the pairs as given.
// `what` is how the call speaks of itself (kRank for every call with a pair list).  With the seen-item index for
// exclusions the kernel reaches its lists through each slot's user.
static int rank_core(mfsgd_handle* h, const ServeName& what, const RankRequest& req) {
    const std::string call = std::string(what.call) + ": ";
    const Exclusions& excl = req.excl;
    const bool unseen = excl.from == Exclusions::kSeen;
    const int64_t n = req.n;
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n is negative");
    if (excl.n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_excl is negative");
    if (n > 0 && (!req.users || !req.items || !req.out_rank))
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "users, items or out_rank is null");
    if (excl.n > 0 && (!excl.u || !excl.i)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "an exclusion array is null");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    if (unseen && !h->seen.present) return fail(h, MFSGD_ERR_STATE, call + "no seen set");
    const int32_t I = h->cfg.n_items;
    const int64_t x_bad = first_outside(req.users, req.n_rows, req.items, I, n);
    if (x_bad >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "pair " + std::to_string(x_bad) + " out of range");
    // a slot per distinct user with its pair count, and how many exclusion pairs are theirs
    Slots slots = slots_of(req.users, n, req.n_rows, true);
    const int32_t n_slots = slots.n();
    std::vector<long long> off((size_t)n_slots + 1, 0);
    // The slots in the order of their pair counts, most first: a workgroup takes neighbouring slots and passes over Q
    // once per round of its user with the most pairs, so users with many pairs belong together.
    {
        std::vector<int32_t> order((size_t)n_slots), rows_sorted((size_t)n_slots);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(),
                         [&slots](int32_t a, int32_t b) { return slots.count[(size_t)a] > slots.count[(size_t)b]; });
        for (int32_t s = 0; s < n_slots; ++s) {
            rows_sorted[(size_t)s] = slots.row_of_slot[(size_t)order[(size_t)s]];
            off[(size_t)s + 1] = slots.count[(size_t)order[(size_t)s]];
            slots.slot_of_row[(size_t)rows_sorted[(size_t)s]] = s;
        }
        slots.row_of_slot.swap(rows_sorted);
    }
    int64_t kept = 0;
    int rc = count_exclusions(h, what, slots.slot_of_row, req.n_rows, I, excl, &kept);
    if (rc) return rc;
    if (n == 0) return MFSGD_OK;
    // (one partition is known by now, and asked about again)
    if ((rc = check_reads_factors(h, what.call)) || (rc = factors_to_device(h))) return rc;
    // counting sort: the pairs of slot s at off[s] .. off[s + 1], in the order given; place[x] = where pair x went
    for (int32_t s = 0; s < n_slots; ++s) off[(size_t)s + 1] += off[(size_t)s];
    std::vector<int32_t> grouped((size_t)n), ranks((size_t)n);
    std::vector<int64_t> place((size_t)n);
    {
        std::vector<long long> next(off.begin(), off.end() - 1);
        for (int64_t x = 0; x < n; ++x) {
            place[(size_t)x] = next[(size_t)slots.slot_of_row[(size_t)req.users[x]]]++;
            grouped[(size_t)place[(size_t)x]] = req.items[x];
        }
    }
    const Batches bt = cut_batches(n_slots, [&off](int32_t s) { return off[(size_t)s + 1] - off[(size_t)s]; }, kRankChunk, INT32_MAX);
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    DevArray<float> d_rows;
    DevArray<int32_t> d_slot_rows, d_items, d_out;
    DevArray<long long> d_off;
    ExclLists lists;
    DevBuf temp;  // the rocPRIM scratch, bytes of no type
    const float* P;
    if ((rc = upload_rows(h, req.host_rows, req.n_rows, d_rows, &P))) return rc;
    RecommendExcl ex;  // built once for all launches; none when no pair belongs to a user asked about
    if (unseen) ex = h->seen.excl();  // (none when the index is empty)
    if (kept > 0 && (rc = exclusions_to_device(h, what, slots, excl, kept, lists, temp, ex))) return rc;
    if ((rc = upload(h, d_slot_rows, slots.row_of_slot))) return rc;
    if ((rc = upload(h, d_off, off))) return rc;
    if ((rc = dev_alloc(h, d_items, (size_t)bt.max_weight)) || (rc = dev_alloc(h, d_out, (size_t)bt.max_weight))) return rc;
    for (size_t b = 0; b < bt.count(); ++b) {
        const int32_t b0 = bt.cut[b], nb = bt.cut[b + 1] - b0;
        const long long base = off[(size_t)b0];
        const size_t pairs = (size_t)(off[(size_t)(b0 + nb)] - base);
        RecommendExcl exb = ex;
        if (exb.off && !unseen) exb.off += b0;  // (the index is reached by user, not by slot)
        HIPCHK_OR(bad, copy_up(d_items, grouped.data() + base, pairs, h->stream));
        HIPCHK_OR(bad, launch_rank_items(h->geo.L, P, h->dQ.data(), d_slot_rows.data() + b0, nb, d_off.data() + b0, base,
                                         d_items.data(), I, exb, d_out.data(), h->stream, unseen));
        HIPCHK_OR(bad, copy_down(ranks.data() + base, d_out, pairs, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // the staging buffers are reused
    }
    for (int64_t x = 0; x < n; ++x) req.out_rank[x] = ranks[(size_t)place[(size_t)x]];
    return MFSGD_OK;
}

static int metrics_fail(int code, const std::string& msg) {
    g_create_error = "ranking_metrics: " + msg;
    return code;
}

// Ratings of one fold-in batch (whole lists; a single list longer than this is a batch of its own): 32 MB of staging
constexpr int64_t kFoldChunk = (int64_t)1 << 22;
constexpr int64_t kFoldRows = (int64_t)1 << 20;  // ... and its new rows, so that a run of empty lists is bounded too

// How a fold-in call speaks of itself, of a new row and of an id.
struct FoldName {
    const char* call;   // "fold_in"
    const char* row;    // "user": what a new row is
    const char* id;     // "item": what a rating names on the fixed side
    const char* ids;    // "items"
};
constexpr FoldName kFoldInUsers{"fold_in", "user", "item", "items"}, kFoldInItems{"fold_in_items", "item", "user", "users"};

// A fold-in call as the caller gave it: n_new lists in CSR form (row_ptr over ids / ratings), and where the rows go.
struct FoldRequest {
    int32_t n_new;
    const int64_t* row_ptr;
    const int32_t* ids;
    const float* ratings;
    int32_t epochs;
    const float* init_rows;
    int64_t seed;
    float* out_rows;
};

// Body of the fold-in calls: n_new rows of one side against the fixed factors of the other.  `fixed` says where those
// are once the factors are on the device (asked then, not before: the upload creates them), n_fixed is their row count.
static int fold_in_core(mfsgd_handle* h, const FoldName& what, const DevArray<float> mfsgd_handle::*fixed, int32_t n_fixed,
                        const FoldRequest& req) {
    const std::string call = std::string(what.call) + ": ";
    const int32_t n_new = req.n_new, epochs = req.epochs;
    const int64_t* row_ptr = req.row_ptr;
    if (n_new < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_new is negative");
    if (epochs < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "epochs is negative");
    if (n_new > 0 && (!row_ptr || !req.out_rows)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr or out_rows is null");
    if (const int rc = check_reads_factors(h, what.call)) return rc;
    if (n_new == 0) return MFSGD_OK;
    if (row_ptr[0] != 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr[0] is not 0");
    for (int32_t x = 0; x < n_new; ++x)
        if (row_ptr[x + 1] < row_ptr[x])
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr decreases at " + what.row + " " + std::to_string(x));
    const int64_t total = row_ptr[n_new];
    if (total > 0 && (!req.ids || !req.ratings)) return fail(h, MFSGD_ERR_INVALID_ARG, call + what.ids + " or ratings is null");
    const int64_t j = first_outside(req.ids, total, n_fixed);
    if (j >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + what.id + " of rating " + std::to_string(j) + " out of range");
    int rc = factors_to_device(h);
    if (rc) return rc;
    const int k = h->cfg.k;
    // batches of whole lists, in the caller's order, so that each batch is one contiguous piece of ids / ratings
    const Batches bt = cut_batches(n_new, [row_ptr](int32_t x) { return row_ptr[x + 1] - row_ptr[x]; }, kFoldChunk, kFoldRows);
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    DevArray<float> d_rows, d_r;
    DevArray<long long> d_ptr;
    DevArray<int32_t> d_perm, d_ids;
    const size_t row_floats = (size_t)n_new * (size_t)k;
    if ((rc = dev_alloc(h, d_rows, row_floats))) return rc;
    if (epochs > 0 && total > 0) {
        if ((rc = dev_alloc(h, d_ptr, (size_t)bt.max_rows + 1)) || (rc = dev_alloc(h, d_perm, (size_t)bt.max_rows))) return rc;
        if ((rc = dev_alloc(h, d_ids, (size_t)bt.max_weight)) || (rc = dev_alloc(h, d_r, (size_t)bt.max_weight))) return rc;
    }
    // the start rows, dense: the kernel pads them to kp in its registers
    if (req.init_rows)
        HIPCHK_OR(bad, copy_up(d_rows, req.init_rows, row_floats, h->stream));
    else
        HIPCHK_OR(bad, launch_init_rows(d_rows.data(), n_new, k, k, req.seed, 0, (float)(1.0 / std::sqrt((double)k)), h->stream));
    std::vector<int32_t> perm;
    for (size_t b = 0; b < bt.count() && epochs > 0; ++b) {
        const int32_t x0 = bt.cut[b], nb = bt.cut[b + 1] - x0;
        const int64_t base = row_ptr[x0], nr = row_ptr[x0 + nb] - base;
        if (nr == 0) continue;
        // longest first: a wave runs as long as its longest list
        perm.resize((size_t)nb);
        std::iota(perm.begin(), perm.end(), 0);
        const int64_t* rp = row_ptr + x0;
        std::stable_sort(perm.begin(), perm.end(), [rp](int32_t a, int32_t b2) { return rp[a + 1] - rp[a] > rp[b2 + 1] - rp[b2]; });
        HIPCHK_OR(bad, copy_up(d_ptr, rp, (size_t)nb + 1, h->stream));
        HIPCHK_OR(bad, copy_up(d_perm, perm.data(), (size_t)nb, h->stream));
        HIPCHK_OR(bad, copy_up(d_ids, req.ids + base, (size_t)nr, h->stream));
        HIPCHK_OR(bad, copy_up(d_r, req.ratings + base, (size_t)nr, h->stream));
        HIPCHK_OR(bad, launch_fold_in(h->geo.L, (h->*fixed).data(), d_rows.data() + (size_t)x0 * k, k, d_ptr.data(), base,
                                      d_perm.data(), nb, d_ids.data(), d_r.data(), epochs, h->cfg.lr,
                                      1.0f - h->cfg.lr * h->cfg.lambda, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // perm and the staging buffers are reused
    }
    HIPCHK_OR(bad, copy_down(req.out_rows, d_rows, row_floats, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

// A pairwise fold-in call as the caller gave it: n_new lists of positives in CSR form, and where the results go.
struct PairwiseFoldRequest {
    int32_t n_new;
    const int64_t* row_ptr;
    const int32_t* items;
    int32_t epochs, m;
    const float* init_rows;
    int64_t seed, draw_seed, first;
    float* out_rows;
    float* out_margin;
    int32_t* out_neg;
    bool weighted = false;  // mfsgd_fold_in_users_pairwise_weighted: the draws go by the handle's item weights
};

// Body of mfsgd_fold_in_users_pairwise: fold_in_core's batches, perm and staging; per batch the sorted distinct lists S
// are made on the device out of the positives that were just uploaded, the way candidates_to_device makes its per-row
// lists (keys user << 32 | item, sorted and made distinct, one CSR offset array), and the chain kernel runs off them.
// And of mfsgd_fold_in_users_pairwise_weighted: the same, and per batch the unseen-mass table of those lists under the
// handle's weights (seen_unseen_mass, as for the index), which the chain's weighted draws search.
static int fold_in_pairwise_core(mfsgd_handle* h, const PairwiseFoldRequest& req) {
    const char* name = req.weighted ? "fold_in_pairwise_weighted" : "fold_in_pairwise";
    const std::string call = std::string(name) + ": ";
    const int32_t n_new = req.n_new, epochs = req.epochs, m = req.m;
    const int64_t* row_ptr = req.row_ptr;
    if (n_new < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_new is negative");
    if (epochs < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "epochs is negative");
    if (m < 1) return fail(h, MFSGD_ERR_INVALID_ARG, call + "m is below 1");
    if (req.first < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "first is negative");
    // (the counters of T positives; a T that the checks below refuse is not multiplied)
    const int64_t claimed = n_new > 0 && row_ptr ? row_ptr[n_new] : 0;
    if (claimed > 0 && (__int128)req.first + (__int128)claimed * epochs * m > (__int128)INT64_MAX)
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "first + T * epochs * m exceeds 2^63 - 1");
    if (n_new > 0 && (!row_ptr || !req.out_rows)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr or out_rows is null");
    if (n_new > 0 && row_ptr[0] != 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr[0] is not 0");
    for (int32_t x = 0; x < n_new; ++x) {
        if (row_ptr[x + 1] < row_ptr[x])
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr decreases at user " + std::to_string(x));
        if (row_ptr[x + 1] - row_ptr[x] > (int64_t)UINT32_MAX)  // (a batch is whole users, and its keys are counted in 32 bits)
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "more than 2^32 - 1 positives of user " + std::to_string(x));
    }
    const int64_t total = n_new > 0 ? row_ptr[n_new] : 0;
    if (total > 0 && !req.items) return fail(h, MFSGD_ERR_INVALID_ARG, call + "items is null");
    const int64_t j = first_outside(req.items, total, h->cfg.n_items);
    if (j >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "item of positive " + std::to_string(j) + " out of range");
    if (const int rc = check_reads_factors(h, name)) return rc;
    const ItemWeights& iw = h->weights;
    if (req.weighted && !iw.present) return fail(h, MFSGD_ERR_STATE, call + "no item weights");
    if (req.weighted && iw.n != h->cfg.n_items)
        return fail(h, MFSGD_ERR_STATE,
                    call + "item weights cover " + std::to_string(iw.n) + " items, the model has " + std::to_string(h->cfg.n_items));
    if (n_new == 0) return MFSGD_OK;
    int rc = factors_to_device(h);
    if (rc) return rc;
    const int k = h->cfg.k;
    // batches of whole lists, in the caller's order, so that each batch is one contiguous piece of items
    const Batches bt = cut_batches(n_new, [row_ptr](int32_t x) { return row_ptr[x + 1] - row_ptr[x]; }, kFoldChunk, kFoldRows);
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    const bool work = epochs > 0 && total > 0;
    const size_t stage = (size_t)bt.max_weight, steps = stage * (size_t)epochs;
    DevArray<float> d_rows, d_margin;
    DevArray<long long> d_ptr, s_off;
    DevArray<int32_t> d_perm, d_ids, s_items, d_neg;
    DevArray<unsigned long long> keys, keys_tmp, s_mass, scanned;  // (the last two: 16 bytes per distinct positive, weighted)
    DevArray<unsigned> count;
    DevBuf temp;  // the rocPRIM scratch, bytes of no type
    const size_t row_floats = (size_t)n_new * (size_t)k;
    if ((rc = dev_alloc(h, d_rows, row_floats))) return rc;
    if (work) {
        if (req.weighted && ((rc = dev_alloc(h, s_mass, stage)) || (rc = dev_alloc(h, scanned, stage)))) return rc;
        if ((rc = dev_alloc(h, d_ptr, (size_t)bt.max_rows + 1)) || (rc = dev_alloc(h, d_perm, (size_t)bt.max_rows))) return rc;
        if ((rc = dev_alloc(h, d_ids, stage))) return rc;
        if ((rc = dev_alloc(h, keys, stage)) || (rc = dev_alloc(h, keys_tmp, stage)) || (rc = dev_alloc(h, count, 4))) return rc;
        if ((rc = dev_alloc(h, s_off, (size_t)bt.max_rows + 1)) || (rc = dev_alloc(h, s_items, stage))) return rc;
        if (req.out_margin && (rc = dev_alloc(h, d_margin, steps))) return rc;
        if (req.out_neg && (rc = dev_alloc(h, d_neg, steps))) return rc;
    }
    // the start rows, dense: the kernel pads them to kp in its registers
    if (req.init_rows)
        HIPCHK_OR(bad, copy_up(d_rows, req.init_rows, row_floats, h->stream));
    else
        HIPCHK_OR(bad, launch_init_rows(d_rows.data(), n_new, k, k, req.seed, 0, (float)(1.0 / std::sqrt((double)k)), h->stream));
    std::vector<int32_t> perm;
    std::vector<long long> ptr;
    for (size_t b = 0; b < bt.count() && work; ++b) {
        const int32_t x0 = bt.cut[b], nb = bt.cut[b + 1] - x0;
        const int64_t base = row_ptr[x0], nr = row_ptr[x0 + nb] - base;
        if (nr == 0) continue;
        // longest first: a wave runs as long as its longest list
        perm.resize((size_t)nb);
        std::iota(perm.begin(), perm.end(), 0);
        const int64_t* rp = row_ptr + x0;
        std::stable_sort(perm.begin(), perm.end(), [rp](int32_t a, int32_t b2) { return rp[a + 1] - rp[a] > rp[b2 + 1] - rp[b2]; });
        // the offsets count from the batch's first positive: what the key kernel and the chain kernel index the batch by
        ptr.resize((size_t)nb + 1);
        for (int32_t x = 0; x <= nb; ++x) ptr[(size_t)x] = rp[x] - base;
        HIPCHK_OR(bad, copy_up(d_ptr, ptr.data(), (size_t)nb + 1, h->stream));
        HIPCHK_OR(bad, copy_up(d_perm, perm.data(), (size_t)nb, h->stream));
        HIPCHK_OR(bad, copy_up(d_ids, req.items + base, (size_t)nr, h->stream));
        HIPCHK_OR(bad, recommend_cand_keys(d_ptr.data(), nb, d_ids.data(), 0, nr, keys.data(), h->stream));
        HIPCHK_OR(bad, recommend_excl_lists(keys.data(), keys_tmp.data(), nr, nb, count.data(), s_off.data(), s_items.data(), temp,
                                            h->stream));
        PairwiseFold job{h->dQ.data(), d_rows.data() + (size_t)x0 * k, k, d_ptr.data(), base, d_perm.data(), nb,
                         d_ids.data(), s_off.data(), s_items.data(), h->cfg.n_items, epochs, m, h->cfg.lr,
                         1.0f - h->cfg.lr * h->cfg.lambda, (unsigned long long)req.draw_seed, (unsigned long long)req.first,
                         d_margin.data(), d_neg.data()};
        if (req.weighted) {
            // the batch's mass table, over its distinct pairs: their number comes down first
            unsigned distinct = 0;
            HIPCHK_OR(bad, copy_down(&distinct, count, 1, h->stream));
            HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
            HIPCHK_OR(bad, seen_unseen_mass(s_off.data(), s_items.data(), (int64_t)distinct, nb, iw.C.data(), iw.n, scanned.data(),
                                            s_mass.data(), temp, h->stream));
            job.s_mass = s_mass.data();
            job.C = iw.C.data();
        }
        HIPCHK_OR(bad, launch_fold_in_pairwise(h->geo.L, job, h->stream));
        const size_t at = (size_t)base * (size_t)epochs, n_steps = (size_t)nr * (size_t)epochs;
        if (req.out_margin) HIPCHK_OR(bad, copy_down(req.out_margin + at, d_margin, n_steps, h->stream));
        if (req.out_neg) HIPCHK_OR(bad, copy_down(req.out_neg + at, d_neg, n_steps, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // perm, ptr and the staging buffers are reused
    }
    HIPCHK_OR(bad, copy_down(req.out_rows, d_rows, row_floats, h->stream));
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

int mfsgd_rank_items(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, const int32_t* excl_u,
                     const int32_t* excl_i, int64_t n_excl, int32_t* out_rank) {
    return guarded(h, "rank_items", [&]() -> int {
        return rank_core(h, kRank, {nullptr, h->cfg.n_users, users, items, n, Exclusions::pairs(excl_u, excl_i, n_excl), out_rank});
    });
}

int mfsgd_rank_items_rows(mfsgd_handle* h, const float* rows, int32_t n_rows, const int32_t* row_of_pair,
                          const int32_t* items, int64_t n, const int32_t* excl_row, const int32_t* excl_item,
                          int64_t n_excl, int32_t* out_rank) {
    return guarded(h, "rank_items", [&]() -> int {
        if (n_rows < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "rank_items: n_rows is negative");
        if (n_rows > 0 && !rows) return fail(h, MFSGD_ERR_INVALID_ARG, "rank_items: rows is null");
        return rank_core(h, kRank, {rows, n_rows, row_of_pair, items, n, Exclusions::pairs(excl_row, excl_item, n_excl), out_rank});
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

// Body of the evaluate calls: rank_core for the model's own users (a null req.out_rank: into a vector of its own), then
// the metrics of the ranks.
static int evaluate_core(mfsgd_handle* h, const ServeName& what, RankRequest req, int32_t topn, mfsgd_ranking_metrics* out) {
    const std::string call = std::string(what.call) + ": ";
    if (topn < 1) return fail(h, MFSGD_ERR_INVALID_ARG, call + "topn is below 1");
    if (!out) return fail(h, MFSGD_ERR_INVALID_ARG, call + "the metrics struct is null");
    std::vector<int32_t> own;
    if (!req.out_rank && req.n > 0) {
        own.resize((size_t)req.n);
        req.out_rank = own.data();
    }
    int rc = rank_core(h, what, req);
    if (rc) return rc;
    rc = mfsgd_ranking_metrics_from_ranks(req.users, req.out_rank, req.n, topn, out);
    if (rc) return fail(h, rc, g_create_error);
    return MFSGD_OK;
}

int mfsgd_evaluate_ranking(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t topn,
                           const int32_t* excl_u, const int32_t* excl_i, int64_t n_excl, mfsgd_ranking_metrics* out,
                           int32_t* out_rank) {
    return guarded(h, "rank_items", [&]() -> int {
        const RankRequest req{nullptr, h->cfg.n_users, users, items, n, Exclusions::pairs(excl_u, excl_i, n_excl), out_rank};
        return evaluate_core(h, kRank, req, topn, out);
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

int mfsgd_rank_items_unseen(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t* out_rank) {
    return guarded(h, kRankUnseen.call, [&]() -> int {
        return rank_core(h, kRankUnseen, {nullptr, h->cfg.n_users, users, items, n, Exclusions::seen(), out_rank});
    });
}

int mfsgd_evaluate_ranking_unseen(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t topn,
                                  mfsgd_ranking_metrics* out, int32_t* out_rank) {
    return guarded(h, kEvaluateUnseen.call, [&]() -> int {
        return evaluate_core(h, kEvaluateUnseen, {nullptr, h->cfg.n_users, users, items, n, Exclusions::seen(), out_rank}, topn, out);
    });
}

int mfsgd_fold_in_users(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* items, const float* ratings,
                        int32_t epochs, const float* init_rows, int64_t seed, float* out_rows) {
    return guarded(h, "fold_in", [&]() -> int {
        return fold_in_core(h, kFoldInUsers, &mfsgd_handle::dQ, h->cfg.n_items,
                            {n_new, row_ptr, items, ratings, epochs, init_rows, seed, out_rows});
    });
}

int mfsgd_fold_in_users_pairwise_weighted(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* items,
                                          int32_t epochs, int32_t m, const float* init_rows, int64_t seed, int64_t draw_seed,
                                          int64_t first, float* out_rows, float* out_margin, int32_t* out_neg) {
    return guarded(h, "fold_in_pairwise_weighted", [&]() -> int {
        return fold_in_pairwise_core(h, {n_new, row_ptr, items, epochs, m, init_rows, seed, draw_seed, first, out_rows,
                                         out_margin, out_neg, true});
    });
}

int mfsgd_fold_in_users_pairwise(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* items, int32_t epochs,
                                 int32_t m, const float* init_rows, int64_t seed, int64_t draw_seed, int64_t first,
                                 float* out_rows, float* out_margin, int32_t* out_neg) {
    return guarded(h, "fold_in_pairwise", [&]() -> int {
        return fold_in_pairwise_core(h, {n_new, row_ptr, items, epochs, m, init_rows, seed, draw_seed, first, out_rows,
                                         out_margin, out_neg});
    });
}

int mfsgd_fold_in_items(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* users, const float* ratings,
                        int32_t epochs, const float* init_rows, int64_t seed, float* out_rows) {
    return guarded(h, "fold_in_items", [&]() -> int {
        return fold_in_core(h, kFoldInItems, &mfsgd_handle::dP, h->cfg.n_users,
                            {n_new, row_ptr, users, ratings, epochs, init_rows, seed, out_rows});
    });
}

}  // extern "C"
