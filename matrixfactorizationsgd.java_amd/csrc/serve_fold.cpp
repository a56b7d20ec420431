// serve_fold.cpp -- the fold-in side of what a trained model answers: rows for new users or new items against the fixed
// factors of the other side, from their ratings by an SGD chain (fold_in_core) or by least squares (fold_in_solve_core,
// with the Gram matrix of a side beside it) or, for users, from their positives alone (fold_in_pairwise_core).  All run
// on one frame: the check of the CSR offsets, and the batches with their staging.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "serve_lists.hpp"

namespace mfsgd {

// Ratings of one fold-in batch (whole lists; a single list longer than this is a batch of its own): 32 MB of staging
constexpr int64_t kFoldChunk = (int64_t)1 << 22;
constexpr int64_t kFoldRows = (int64_t)1 << 20;  // ... and its new rows, so that a run of empty lists is bounded too

// The shape of a fold-in call's lists: row_ptr starts at 0 and never decreases and (max_32_bits: the pairwise call,
// where a batch is whole users and its keys are counted in 32 bits) no list holds more than 2^32 - 1 entries.  `call`
// ends in ": ", `row` is what a new row is called.
static int check_fold_lists(const mfsgd_handle* h, const std::string& call, const int64_t* row_ptr, int32_t n_new, const char* row,
                            bool max_32_bits) {
    if (n_new > 0 && row_ptr[0] != 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr[0] is not 0");
    for (int32_t x = 0; x < n_new; ++x) {
        if (row_ptr[x + 1] < row_ptr[x])
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr decreases at " + row + " " + std::to_string(x));
        if (max_32_bits && row_ptr[x + 1] - row_ptr[x] > (int64_t)UINT32_MAX)
            return fail(h, MFSGD_ERR_INVALID_ARG, call + "more than 2^32 - 1 positives of " + row + " " + std::to_string(x));
    }
    return MFSGD_OK;
}

// A fold-in call as the caller gave it: n_new lists in CSR form (row_ptr over ids and, the rated calls, ratings), the
// start rows (init_rows, or seeded from `seed`) and where the rows go.  The least-squares call has no start rows
// (start_rows = false: a row starts, and without entries stays, +0.0f) and no epochs: its one pass is epochs = 1.
struct FoldRequest {
    int32_t n_new;
    const int64_t* row_ptr;
    const int32_t* ids;
    const float* ratings;
    int32_t epochs;
    const float* init_rows;
    int64_t seed;
    float* out_rows;
    bool start_rows = true;
};

// One batch on the device: nb new rows from row x0 of the call on (rows: theirs, dense), whose nr ids start at `base` of
// the call's; ptr[nb + 1], perm[nb] (the batch's rows, longest list first) and ids[nr] are the frame's staging.
struct FoldBatch {
    int32_t x0, nb;
    int64_t base, nr;
    float* rows;
    const long long* ptr;
    const int32_t *perm, *ids;
};

// The frame of a checked fold-in call with n_new > 0: the factors on the device, batches of whole lists in the caller's
// order (each one contiguous piece of ids), the start rows (zeros where the call has none), per batch with ids its
// offsets, perm and ids up, `run(batch)` and a synchronise, and the rows down at the end.  rebased: the offsets go up counted from the batch's first id (the
// pairwise kernels index the batch by them); otherwise as they are, and the kernel gets the batch's `base` beside them.
// `extra(bt)` allocates what the core stages beside that, sized by the largest batch; neither it nor a batch is run
// where epochs == 0 or there are no ids: the start rows are the result.  `call` starts the message of a HIP failure.
template <class Extra, class Run>
static int fold_batches(mfsgd_handle* h, const std::string& call, const FoldRequest& f, bool rebased, Extra extra, Run run) {
    int rc = factors_to_device(h);
    if (rc) return rc;
    const int32_t k = h->cfg.k, n_new = f.n_new;
    const int64_t* row_ptr = f.row_ptr;
    const Batches bt = cut_batches(n_new, [row_ptr](int32_t x) { return row_ptr[x + 1] - row_ptr[x]; }, kFoldChunk, kFoldRows);
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    const bool work = f.epochs > 0 && row_ptr[n_new] > 0;
    DevArray<float> d_rows;
    DevArray<long long> d_ptr;
    DevArray<int32_t> d_perm, d_ids;
    const size_t row_floats = (size_t)n_new * (size_t)k;
    if ((rc = dev_alloc(h, d_rows, row_floats))) return rc;
    if (work) {
        if ((rc = dev_alloc(h, d_ptr, (size_t)bt.max_rows + 1)) || (rc = dev_alloc(h, d_perm, (size_t)bt.max_rows))) return rc;
        if ((rc = dev_alloc(h, d_ids, (size_t)bt.max_weight)) || (rc = extra(bt))) return rc;
    }
    // the start rows, dense: the kernel pads them to kp in its registers (no start rows: what a list without ids keeps)
    if (!f.start_rows)
        HIPCHK_OR(bad, hipMemsetAsync(d_rows.data(), 0, row_floats * sizeof(float), h->stream));
    else if (f.init_rows)
        HIPCHK_OR(bad, copy_up(d_rows, f.init_rows, row_floats, h->stream));
    else
        HIPCHK_OR(bad, launch_init_rows(d_rows.data(), n_new, k, k, f.seed, 0, (float)(1.0 / std::sqrt((double)k)), h->stream));
    std::vector<int32_t> perm;
    std::vector<long long> ptr;  // (rebased only)
    for (size_t b = 0; b < bt.count() && work; ++b) {
        const int32_t x0 = bt.cut[b], nb = bt.cut[b + 1] - x0;
        const int64_t base = row_ptr[x0], nr = row_ptr[x0 + nb] - base;
        if (nr == 0) continue;
        // longest first: a wave runs as long as its longest list
        perm.resize((size_t)nb);
        std::iota(perm.begin(), perm.end(), 0);
        const int64_t* rp = row_ptr + x0;
        std::stable_sort(perm.begin(), perm.end(), [rp](int32_t a, int32_t b2) { return rp[a + 1] - rp[a] > rp[b2 + 1] - rp[b2]; });
        if (rebased) {
            ptr.resize((size_t)nb + 1);
            for (int32_t x = 0; x <= nb; ++x) ptr[(size_t)x] = rp[x] - base;
            HIPCHK_OR(bad, copy_up(d_ptr, ptr.data(), (size_t)nb + 1, h->stream));
        } else {
            HIPCHK_OR(bad, copy_up(d_ptr, rp, (size_t)nb + 1, h->stream));
        }
        HIPCHK_OR(bad, copy_up(d_perm, perm.data(), (size_t)nb, h->stream));
        HIPCHK_OR(bad, copy_up(d_ids, f.ids + base, (size_t)nr, h->stream));
        if ((rc = run(FoldBatch{x0, nb, base, nr, d_rows.data() + (size_t)x0 * k, d_ptr.data(), d_perm.data(), d_ids.data()}))) return rc;
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // perm, ptr and the staging buffers are reused
    }
    HIPCHK_OR(bad, copy_down(f.out_rows, d_rows, row_floats, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

// How a fold-in call speaks of itself, of a new row and of an id.
struct FoldName {
    const char* call;   // "fold_in"
    const char* row;    // "user": what a new row is
    const char* id;     // "item": what a rating names on the fixed side
    const char* ids;    // "items"
};
constexpr FoldName kFoldInUsers{"fold_in", "user", "item", "items"}, kFoldInItems{"fold_in_items", "item", "user", "users"};

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
    int rc = check_reads_factors(h, what.call);
    if (rc) return rc;
    if (n_new == 0) return MFSGD_OK;
    if ((rc = check_fold_lists(h, call, row_ptr, n_new, what.row, false))) return rc;
    const int64_t total = row_ptr[n_new];
    if (total > 0 && (!req.ids || !req.ratings)) return fail(h, MFSGD_ERR_INVALID_ARG, call + what.ids + " or ratings is null");
    const int64_t j = first_outside(req.ids, total, n_fixed);
    if (j >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + what.id + " of rating " + std::to_string(j) + " out of range");
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    const int k = h->cfg.k;
    DevArray<float> d_r;  // the batch's ratings, beside its ids
    return fold_batches(
        h, call, req, false, [&](const Batches& bt) { return dev_alloc(h, d_r, (size_t)bt.max_weight); },
        [&](const FoldBatch& b) -> int {
            HIPCHK_OR(bad, copy_up(d_r, req.ratings + b.base, (size_t)b.nr, h->stream));
            HIPCHK_OR(bad, launch_fold_in(h->geo.L, (h->*fixed).data(), b.rows, k, b.ptr, b.base, b.perm, b.nb, b.ids, d_r.data(), epochs,
                                          h->cfg.lr, 1.0f - h->cfg.lr * h->cfg.lambda, h->stream));
            return MFSGD_OK;
        });
}

// A pairwise fold-in call as the caller gave it: n_new lists of positives in CSR form, and where the results go.
struct PairwiseFoldRequest {
    FoldRequest lists;  // (ids: the positives; no ratings)
    int32_t m;
    int64_t draw_seed, first;
    float* out_margin;
    int32_t* out_neg;
    bool weighted = false;  // mfsgd_fold_in_users_pairwise_weighted: the draws go by the handle's item weights
};

// Body of mfsgd_fold_in_users_pairwise: per batch the sorted distinct lists S are made on the device out of the
// positives the frame has just uploaded, the way candidates_to_device makes its per-row lists (keys user << 32 | item,
// then KeyLists), and the chain kernel runs off them.
// And of mfsgd_fold_in_users_pairwise_weighted: the same, and per batch the unseen-mass table of those lists under the
// handle's weights (seen_unseen_mass, as for the index), which the chain's weighted draws search.
static int fold_in_pairwise_core(mfsgd_handle* h, const PairwiseFoldRequest& req) {
    const char* name = req.weighted ? "fold_in_pairwise_weighted" : "fold_in_pairwise";
    const std::string call = std::string(name) + ": ";
    const FoldRequest& lists = req.lists;
    const int32_t n_new = lists.n_new, epochs = lists.epochs, m = req.m;
    const int64_t* row_ptr = lists.row_ptr;
    if (n_new < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_new is negative");
    if (epochs < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "epochs is negative");
    if (m < 1) return fail(h, MFSGD_ERR_INVALID_ARG, call + "m is below 1");
    if (req.first < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "first is negative");
    // (the counters of T positives; a T that the checks below refuse is not multiplied)
    const int64_t claimed = n_new > 0 && row_ptr ? row_ptr[n_new] : 0;
    if (claimed > 0 && (__int128)req.first + (__int128)claimed * epochs * m > (__int128)INT64_MAX)
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "first + T * epochs * m exceeds 2^63 - 1");
    if (n_new > 0 && (!row_ptr || !lists.out_rows)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr or out_rows is null");
    int rc = check_fold_lists(h, call, row_ptr, n_new, "user", true);
    if (rc) return rc;
    const int64_t total = n_new > 0 ? row_ptr[n_new] : 0;
    if (total > 0 && !lists.ids) return fail(h, MFSGD_ERR_INVALID_ARG, call + "items is null");
    const int64_t j = first_outside(lists.ids, total, h->cfg.n_items);
    if (j >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "item of positive " + std::to_string(j) + " out of range");
    if ((rc = check_reads_factors(h, name))) return rc;
    const ItemWeights& iw = h->weights;
    if (req.weighted && !iw.present) return fail(h, MFSGD_ERR_STATE, call + "no item weights");
    if (req.weighted && iw.n != h->cfg.n_items)
        return fail(h, MFSGD_ERR_STATE,
                    call + "item weights cover " + std::to_string(iw.n) + " items, the model has " + std::to_string(h->cfg.n_items));
    if (n_new == 0) return MFSGD_OK;
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    const int k = h->cfg.k;
    KeyLists S;  // the batch's keys and the lists S they become
    DevArray<float> d_margin;
    DevArray<int32_t> d_neg;
    DevArray<unsigned long long> s_mass, scanned;  // (16 bytes per distinct positive, weighted)
    DevBuf temp;  // the rocPRIM scratch, bytes of no type
    return fold_batches(
        h, call, lists, true,
        [&](const Batches& bt) -> int {
            const size_t stage = (size_t)bt.max_weight, steps = stage * (size_t)epochs;
            if (req.weighted && ((rc = dev_alloc(h, s_mass, stage)) || (rc = dev_alloc(h, scanned, stage)))) return rc;
            if ((rc = S.alloc(h, bt.max_weight, bt.max_rows))) return rc;
            if (req.out_margin && (rc = dev_alloc(h, d_margin, steps))) return rc;
            if (req.out_neg && (rc = dev_alloc(h, d_neg, steps))) return rc;
            return MFSGD_OK;
        },
        [&](const FoldBatch& b) -> int {
            HIPCHK_OR(bad, recommend_cand_keys(b.ptr, b.nb, b.ids, 0, b.nr, S.keys.data(), h->stream));
            HIPCHK_OR(bad, S.finish(b.nr, b.nb, temp, h->stream));
            PairwiseFold job{h->dQ.data(), b.rows, k, b.ptr, b.base, b.perm, b.nb,
                             b.ids, S.off.data(), S.items.data(), h->cfg.n_items, epochs, m, h->cfg.lr,
                             1.0f - h->cfg.lr * h->cfg.lambda, (unsigned long long)req.draw_seed, (unsigned long long)req.first,
                             d_margin.data(), d_neg.data()};
            if (req.weighted) {
                // the batch's mass table, over its distinct pairs: their number comes down first
                unsigned distinct = 0;
                HIPCHK_OR(bad, copy_down(&distinct, S.count, 1, h->stream, S.distinct_at()));
                HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
                HIPCHK_OR(bad, seen_unseen_mass(S.off.data(), S.items.data(), (int64_t)distinct, b.nb, iw.C.data(), iw.n, scanned.data(),
                                                s_mass.data(), temp, h->stream));
                job.s_mass = s_mass.data();
                job.C = iw.C.data();
            }
            HIPCHK_OR(bad, launch_fold_in_pairwise(h->geo.L, job, h->stream));
            const size_t at = (size_t)b.base * (size_t)epochs, n_steps = (size_t)b.nr * (size_t)epochs;
            if (req.out_margin) HIPCHK_OR(bad, copy_down(req.out_margin + at, d_margin, n_steps, h->stream));
            if (req.out_neg) HIPCHK_OR(bad, copy_down(req.out_neg + at, d_neg, n_steps, h->stream));
            return MFSGD_OK;
        });
}

// G = gram(F) of the n rows of one side on the device, k x k; the tile partials live as long as this function.
static int gram_to_device(mfsgd_handle* h, const std::string& call, const float* F, int32_t n, DevArray<float>& d_G) {
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    const size_t kk = (size_t)h->cfg.k * (size_t)h->cfg.k;
    DevArray<float> partial;
    int rc = dev_alloc(h, d_G, kk);
    if (rc || (rc = dev_alloc(h, partial, (size_t)gram_tiles(n) * kk))) return rc;
    HIPCHK_OR(bad, launch_gram(h->geo.L, F, n, h->cfg.k, partial.data(), d_G.data(), h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

static bool is_side(int32_t side) { return side == MFSGD_SIDE_USERS || side == MFSGD_SIDE_ITEMS; }

// A least-squares fold-in call as the caller gave it: the lists (ratings: b), the weights a (nullable) and the three
// numbers of the system, and where the status of each row goes (nullable).
struct SolveFoldRequest {
    FoldRequest lists;
    const float* a;
    float alpha, ridge, ridge_per_entry;
    int32_t* out_status;
};

// Body of mfsgd_fold_in_solve: n_new rows of `side` against the fixed factors of the other side, each the solution of
// its own k x k system (solve.hip).  G of the fixed side is made once per call, and only where alpha != 0.
static int fold_in_solve_core(mfsgd_handle* h, int32_t side, const SolveFoldRequest& req) {
    const std::string call = "fold_in_solve: ";
    const FoldRequest& lists = req.lists;
    const int32_t n_new = lists.n_new;
    const int64_t* row_ptr = lists.row_ptr;
    if (!is_side(side)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "side is neither MFSGD_SIDE_USERS nor MFSGD_SIDE_ITEMS");
    if (n_new < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n_new is negative");
    if (n_new > 0 && (!row_ptr || !lists.out_rows)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "row_ptr or out_rows is null");
    int rc = check_fold_lists(h, call, row_ptr, n_new, "row", false);
    if (rc) return rc;
    const bool users = side == MFSGD_SIDE_USERS;  // new users: against Q
    const int32_t n_fixed = users ? h->cfg.n_items : h->cfg.n_users;
    const int64_t total = n_new > 0 ? row_ptr[n_new] : 0;
    if (total > 0 && (!lists.ids || !lists.ratings)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "ids or b is null");
    const int64_t j = first_outside(lists.ids, total, n_fixed);
    if (j >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "id of entry " + std::to_string(j) + " out of range");
    if (!std::isfinite(req.alpha) || !std::isfinite(req.ridge) || !std::isfinite(req.ridge_per_entry))
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "alpha, ridge or ridge_per_entry is not finite");
    if ((rc = check_reads_factors(h, "fold_in_solve"))) return rc;
    if (n_new == 0) return MFSGD_OK;
    if ((rc = factors_to_device(h))) return rc;
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    const float* F = users ? h->dQ.data() : h->dP.data();
    DevArray<float> d_a, d_b, d_G;
    DevArray<int32_t> d_status;  // of the whole call: a list without entries never reaches the kernel, and is status 0
    if (req.out_status) {
        if ((rc = dev_alloc(h, d_status, (size_t)n_new))) return rc;
        HIPCHK_OR(bad, hipMemsetAsync(d_status.data(), 0, (size_t)n_new * sizeof(int32_t), h->stream));
    }
    rc = fold_batches(
        h, call, lists, false,
        [&](const Batches& bt) -> int {
            int rc2 = dev_alloc(h, d_b, (size_t)bt.max_weight);
            if (rc2 || (req.a && (rc2 = dev_alloc(h, d_a, (size_t)bt.max_weight)))) return rc2;
            return req.alpha != 0.0f ? gram_to_device(h, call, F, n_fixed, d_G) : MFSGD_OK;
        },
        [&](const FoldBatch& b) -> int {
            HIPCHK_OR(bad, copy_up(d_b, lists.ratings + b.base, (size_t)b.nr, h->stream));
            if (req.a) HIPCHK_OR(bad, copy_up(d_a, req.a + b.base, (size_t)b.nr, h->stream));
            const SolveRows job{F, b.rows, h->cfg.k, b.ptr, b.base, b.perm, b.nb, b.ids, req.a ? d_a.data() : nullptr, d_b.data(),
                                d_G.data(), req.alpha, req.ridge, req.ridge_per_entry,
                                req.out_status ? d_status.data() + b.x0 : nullptr};
            HIPCHK_OR(bad, launch_solve_rows(h->geo.L, job, h->stream));
            return MFSGD_OK;
        });
    if (rc || !req.out_status) return rc;
    HIPCHK_OR(bad, copy_down(req.out_status, d_status, (size_t)n_new, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

}  // namespace mfsgd

using namespace mfsgd;

extern "C" {

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
        return fold_in_pairwise_core(h, {{n_new, row_ptr, items, nullptr, epochs, init_rows, seed, out_rows}, m, draw_seed, first,
                                         out_margin, out_neg, true});
    });
}

int mfsgd_fold_in_users_pairwise(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* items, int32_t epochs,
                                 int32_t m, const float* init_rows, int64_t seed, int64_t draw_seed, int64_t first,
                                 float* out_rows, float* out_margin, int32_t* out_neg) {
    return guarded(h, "fold_in_pairwise", [&]() -> int {
        return fold_in_pairwise_core(h, {{n_new, row_ptr, items, nullptr, epochs, init_rows, seed, out_rows}, m, draw_seed, first,
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

int mfsgd_gram(mfsgd_handle* h, int32_t side, float* out) {
    return guarded(h, "gram", [&]() -> int {
        if (!is_side(side)) return fail(h, MFSGD_ERR_INVALID_ARG, "gram: side is neither MFSGD_SIDE_USERS nor MFSGD_SIDE_ITEMS");
        if (!out) return fail(h, MFSGD_ERR_INVALID_ARG, "gram: out is null");
        const bool of_items = side == MFSGD_SIDE_ITEMS;  // (the users' side reads P alone)
        int rc = check_reads_factors(h, "gram", of_items);
        if (rc || (rc = factors_to_device(h))) return rc;
        auto bad = [h](hipError_t e) { return serve_fail(h, "gram: ", e); };
        DevArray<float> d_G;
        if ((rc = gram_to_device(h, "gram: ", of_items ? h->dQ.data() : h->dP.data(), of_items ? h->cfg.n_items : h->cfg.n_users, d_G)))
            return rc;
        HIPCHK_OR(bad, copy_down(out, d_G, d_G.size(), h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
        return MFSGD_OK;
    });
}

int mfsgd_fold_in_solve(mfsgd_handle* h, int32_t side, int32_t n_new, const int64_t* row_ptr, const int32_t* ids, const float* a,
                        const float* b, float alpha, float ridge, float ridge_per_entry, float* out_rows, int32_t* out_status) {
    return guarded(h, "fold_in_solve", [&]() -> int {
        return fold_in_solve_core(h, side, {{n_new, row_ptr, ids, b, 1, nullptr, 0, out_rows, false}, a, alpha, ridge,
                                            ridge_per_entry, out_status});
    });
}

}  // extern "C"
