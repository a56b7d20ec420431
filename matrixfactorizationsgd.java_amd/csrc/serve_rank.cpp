// serve_rank.cpp -- the rank side of what a trained model answers: where held-out items land in a user's
// recommendation order, and the metrics of those ranks (host).  The pairs go through bounded staging buffers.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "serve_lists.hpp"

namespace mfsgd {

constexpr ServeName kRank{"rank_items", "the users asked about"};
// ... and the calls that exclude what the handle's seen-item index holds instead of a pair list
constexpr ServeName kRankUnseen{"rank_items_unseen", "the users asked about"};
constexpr ServeName kEvaluateUnseen{"evaluate_ranking_unseen", "the users asked about"};

// A rank call over the kind of row matrix a top-N call has (the model's P, or host_rows, n_rows x k, dense): the n pairs
// (users[x], items[x]), and where their ranks go.
struct RankRequest {
    const float* host_rows = nullptr;
    int32_t n_rows = 0;
    const int32_t *users = nullptr, *items = nullptr;
    int64_t n = 0;
    Exclusions excl;
    int32_t* out_rank = nullptr;
};

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

}  // namespace mfsgd

using namespace mfsgd;

extern "C" {

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

}  // extern "C"
