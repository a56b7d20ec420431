// MatrixFactorizationSGD.hpp -- C++ host mirror of the Java surface over the C-ABI.
//
// The reference's toolchain (a JDK) is absent from this image, so the compiled
// host side above the C-ABI is C++ (the task's rule for compiled references);
// it mirrors java/MatrixFactorizationSGD.java method for method: same names,
// same argument meaning, a non-zero status becomes std::runtime_error where
// Java throws RuntimeException.  Header only; link against libmfsgd.so.
#pragma once

#include <array>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mfsgd.h"

class MatrixFactorizationSGD {
   public:
    // n_parts >= 2: one rank of a DSGD job (this rank's users, the GLOBAL item count, world * parts-per-rank item
    // partitions) -- Java: MatrixFactorizationSGD(users, items, k, lr, lambda, seed, device, nParts)
    MatrixFactorizationSGD(int users, int items, int k, float lr, float lambda, long long seed, int device = 0, int n_parts = 0)
        : users_(users), items_(items), k_(k), n_parts_(n_parts > 1 ? n_parts : 1), seed_(seed) {
        mfsgd_config cfg = {};
        cfg.n_users = users;
        cfg.n_items = items;
        cfg.k = k;
        cfg.lr = lr;
        cfg.lambda = lambda;
        cfg.device = device;
        cfg.n_parts = n_parts;
        const int rc = mfsgd_create(&cfg, &h_);
        if (rc != MFSGD_OK) throw std::runtime_error(std::string("mfsgd_create: ") + mfsgd_last_error(nullptr));
    }
    ~MatrixFactorizationSGD() { close(); }
    MatrixFactorizationSGD(const MatrixFactorizationSGD&) = delete;
    MatrixFactorizationSGD& operator=(const MatrixFactorizationSGD&) = delete;

    // what every top-N call returns: {index, scores}, row-major rows x topN
    using TopN = std::pair<std::vector<int32_t>, std::vector<float>>;

    // double[] train(int[] u, int[] i, float[] r, int epochs): RMSE after each epoch
    std::vector<double> train(const std::vector<int32_t>& u, const std::vector<int32_t>& i, const std::vector<float>& r,
                              int epochs) {
        if (u.size() != i.size() || u.size() != r.size()) throw std::invalid_argument("length mismatch");
        check(mfsgd_set_ratings(h_, u.data(), i.data(), r.data(), (int64_t)u.size()));
        if (!initialised_) {
            check(mfsgd_init_factors(h_, seed_));
            initialised_ = true;
        }
        std::vector<double> rmse((size_t)epochs, 0.0);
        check(mfsgd_train(h_, epochs, rmse.data()));
        return rmse;
    }

    float predict(int u, int i) {
        float out = 0.f;
        const int32_t uu = u, ii = i;
        check(mfsgd_predict(h_, &uu, &ii, &out, 1));
        return out;
    }
    std::vector<float> predict(const std::vector<int32_t>& u, const std::vector<int32_t>& i) {
        if (u.size() != i.size()) throw std::invalid_argument("length mismatch");
        std::vector<float> out(u.size());
        check(mfsgd_predict(h_, u.data(), i.data(), out.data(), (int64_t)u.size()));
        return out;
    }

    // int[][] recommend(int[] users, int topN): best items per user, best first (row-major users x topN)
    TopN recommend(const std::vector<int32_t>& users, int topn) {
        TopN out = top_n(users.size(), topn);
        check(mfsgd_recommend(h_, users.data(), (int32_t)users.size(), topn, out.first.data(), out.second.data()));
        return out;
    }
    // int[][] recommend(int[] users, int topN, int[] exclU, int[] exclI): as above, never an item (exclU[x], exclI[x]) names
    // for that user; rows short of eligible items end in item -1, score NaN
    TopN recommend(const std::vector<int32_t>& users, int topn,
                   const std::vector<int32_t>& excl_u,
                   const std::vector<int32_t>& excl_i) {
        if (excl_u.size() != excl_i.size()) throw std::invalid_argument("length mismatch");
        TopN out = top_n(users.size(), topn);
        check(mfsgd_recommend_excluding(h_, users.data(), (int32_t)users.size(), topn, excl_u.data(), excl_i.data(),
                                        (int64_t)excl_u.size(), out.first.data(), out.second.data()));
        return out;
    }

    // float[] foldIn(long[] rowPtr, int[] items, float[] ratings, int epochs[, float[] init]): rows (n_new x k, row-major)
    // of users that are not in the model, against the fixed item factors; without init the rows start seeded
    std::vector<float> foldIn(const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& items,
                              const std::vector<float>& ratings, int epochs, int64_t seed) {
        return foldIn(row_ptr, items, ratings, epochs, nullptr, seed);
    }
    std::vector<float> foldIn(const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& items,
                              const std::vector<float>& ratings, int epochs, const std::vector<float>& init) {
        if (row_ptr.empty() || init.size() != (row_ptr.size() - 1) * (size_t)k_) throw std::invalid_argument("length mismatch");
        return foldIn(row_ptr, items, ratings, epochs, init.data(), 0);
    }
    // float[] foldInItems(long[] rowPtr, int[] users, float[] ratings, int epochs[, float[] init]): the same for items that
    // are not in the model, against the fixed user factors
    std::vector<float> foldInItems(const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& users,
                                   const std::vector<float>& ratings, int epochs, int64_t seed) {
        return foldIn(row_ptr, users, ratings, epochs, nullptr, seed, mfsgd_fold_in_items);
    }
    std::vector<float> foldInItems(const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& users,
                                   const std::vector<float>& ratings, int epochs, const std::vector<float>& init) {
        if (row_ptr.empty() || init.size() != (row_ptr.size() - 1) * (size_t)k_) throw std::invalid_argument("length mismatch");
        return foldIn(row_ptr, users, ratings, epochs, init.data(), 0, mfsgd_fold_in_items);
    }
    // int addUsers(float[] rows) / addUsers(int n, long seed), addItems likewise: rows (n x k; for instance a fold-in's)
    // or n seeded rows appended to the live model, nothing rebuilt; returns the index of the first new row
    int addUsers(const std::vector<float>& rows) { return append(mfsgd_append_users, users_, &rows, 0, 0); }
    int addUsers(int n, int64_t seed) { return append(mfsgd_append_users, users_, nullptr, n, seed); }
    int addItems(const std::vector<float>& rows) { return append(mfsgd_append_items, items_, &rows, 0, 0); }
    int addItems(int n, int64_t seed) { return append(mfsgd_append_items, items_, nullptr, n, seed); }
    // void reserve(int users, int items): room for that many in all (0: leave that side alone), so that appends up to
    // there keep P and Q where they are, and with them the cached training graphs
    void reserve(int users, int items) { check(mfsgd_reserve_rows(h_, users, items)); }
    // int[] capacity(): {users, items}
    std::pair<int, int> capacity() {
        int32_t u = 0, i = 0;
        check(mfsgd_get_capacity(h_, &u, &i));
        return {u, i};
    }
    int users() const { return users_; }
    int items() const { return items_; }
    // int[][] recommendRows(float[] rows, int topN, int[] exclRow, int[] exclItem): recommend for rows (n x k) that are
    // not in the model, such as foldIn's; exclRow indexes rows
    TopN recommendRows(const std::vector<float>& rows, int topn,
                       const std::vector<int32_t>& excl_row = {},
                       const std::vector<int32_t>& excl_item = {}) {
        if (excl_row.size() != excl_item.size() || rows.size() % (size_t)k_ != 0) throw std::invalid_argument("length mismatch");
        const size_t n = rows.size() / (size_t)k_;
        TopN out = top_n(n, topn);
        check(mfsgd_recommend_rows(h_, rows.data(), (int32_t)n, topn, excl_row.data(), excl_item.data(),
                                   (int64_t)excl_row.size(), out.first.data(), out.second.data()));
        return out;
    }
    // int[][] recommendAmong(int[] users, int topN, long[] candPtr, int[] candItems, int[] exclU, int[] exclI): the best
    // topN of each row's candidates only -- candPtr empty: one list, candItems, for every row; otherwise CSR over the rows
    // of users (users.length + 1 offsets).  Lists may be unsorted and repeat items; rows short of candidates are padded
    TopN recommendAmong(const std::vector<int32_t>& users, int topn,
                        const std::vector<int64_t>& cand_ptr,
                        const std::vector<int32_t>& cand_items,
                        const std::vector<int32_t>& excl_u = {},
                        const std::vector<int32_t>& excl_i = {}) {
        if (excl_u.size() != excl_i.size() || (!cand_ptr.empty() && cand_ptr.size() != users.size() + 1))
            throw std::invalid_argument("length mismatch");
        TopN out = top_n(users.size(), topn);
        check(mfsgd_recommend_among(h_, users.data(), (int32_t)users.size(), topn, cand_ptr.empty() ? nullptr : cand_ptr.data(),
                                    cand_items.data(), (int64_t)cand_items.size(), excl_u.data(), excl_i.data(),
                                    (int64_t)excl_u.size(), out.first.data(), out.second.data()));
        return out;
    }
    // int[][] recommendRowsAmong(float[] rows, int topN, long[] candPtr, int[] candItems, int[] exclRow, int[] exclItem):
    // the same for rows (n x k) that are not in the model; candPtr and exclRow index rows
    TopN recommendRowsAmong(const std::vector<float>& rows, int topn,
                            const std::vector<int64_t>& cand_ptr,
                            const std::vector<int32_t>& cand_items,
                            const std::vector<int32_t>& excl_row = {},
                            const std::vector<int32_t>& excl_item = {}) {
        if (excl_row.size() != excl_item.size() || rows.size() % (size_t)k_ != 0) throw std::invalid_argument("length mismatch");
        const size_t n = rows.size() / (size_t)k_;
        if (!cand_ptr.empty() && cand_ptr.size() != n + 1) throw std::invalid_argument("length mismatch");
        TopN out = top_n(n, topn);
        check(mfsgd_recommend_rows_among(h_, rows.data(), (int32_t)n, topn, cand_ptr.empty() ? nullptr : cand_ptr.data(),
                                         cand_items.data(), (int64_t)cand_items.size(), excl_row.data(), excl_item.data(),
                                         (int64_t)excl_row.size(), out.first.data(), out.second.data()));
        return out;
    }

    // int[][] similarItems(int[] items, int topN) / similarUsers(int[] users, int topN): per query the topN other rows of
    // Q / of P with the largest cosine, best first, never the query itself (row-major queries x topN, with the scores)
    TopN similarItems(const std::vector<int32_t>& items, int topn) {
        TopN out = top_n(items.size(), topn);
        check(mfsgd_similar_items(h_, items.data(), (int32_t)items.size(), topn, out.first.data(), out.second.data()));
        return out;
    }
    TopN similarUsers(const std::vector<int32_t>& users, int topn) {
        TopN out = top_n(users.size(), topn);
        check(mfsgd_similar_users(h_, users.data(), (int32_t)users.size(), topn, out.first.data(), out.second.data()));
        return out;
    }
    // int[][] similarRows(float[] rows, int topN, int side): the same for query vectors (n x k) that are not in the model,
    // against the rows of Q (MFSGD_SIDE_ITEMS) or P (MFSGD_SIDE_USERS); nothing is excluded
    TopN similarRows(const std::vector<float>& rows, int topn,
                     int side = MFSGD_SIDE_ITEMS) {
        if (rows.size() % (size_t)k_ != 0) throw std::invalid_argument("length mismatch");
        const size_t n = rows.size() / (size_t)k_;
        TopN out = top_n(n, topn);
        check(mfsgd_similar_rows(h_, side, rows.data(), (int32_t)n, topn, out.first.data(), out.second.data()));
        return out;
    }
    // float[] rowInvNorms(int side): 1 / sqrt(dot(row, row)) of every row of P or Q, 0 for a zero row
    std::vector<float> rowInvNorms(int side) {
        if (side != MFSGD_SIDE_USERS && side != MFSGD_SIDE_ITEMS) throw std::invalid_argument("side");
        std::vector<float> out((size_t)(side == MFSGD_SIDE_ITEMS ? items_ : users_));
        check(mfsgd_row_inv_norms(h_, side, out.data()));
        return out;
    }

    // int[] rankItems(int[] u, int[] i, int[] exclU, int[] exclI): per held-out pair the number of items that come before
    // it in its user's recommendation order (its index in recommend(u, items, exclU, exclI)'s row)
    std::vector<int32_t> rankItems(const std::vector<int32_t>& u, const std::vector<int32_t>& i,
                                   const std::vector<int32_t>& excl_u = {}, const std::vector<int32_t>& excl_i = {}) {
        if (u.size() != i.size() || excl_u.size() != excl_i.size()) throw std::invalid_argument("length mismatch");
        std::vector<int32_t> ranks(u.size());
        check(mfsgd_rank_items(h_, u.data(), i.data(), (int64_t)u.size(), excl_u.data(), excl_i.data(),
                               (int64_t)excl_u.size(), ranks.data()));
        return ranks;
    }
    // int[] rankItemsRows(float[] rows, int[] row, int[] i, int[] exclRow, int[] exclItem): the same for rows (n x k) that
    // are not in the model, such as foldIn's
    std::vector<int32_t> rankItemsRows(const std::vector<float>& rows, const std::vector<int32_t>& row,
                                       const std::vector<int32_t>& i, const std::vector<int32_t>& excl_row = {},
                                       const std::vector<int32_t>& excl_item = {}) {
        if (row.size() != i.size() || excl_row.size() != excl_item.size() || rows.size() % (size_t)k_ != 0)
            throw std::invalid_argument("length mismatch");
        std::vector<int32_t> ranks(row.size());
        check(mfsgd_rank_items_rows(h_, rows.data(), (int32_t)(rows.size() / (size_t)k_), row.data(), i.data(),
                                    (int64_t)row.size(), excl_row.data(), excl_item.data(), (int64_t)excl_row.size(),
                                    ranks.data()));
        return ranks;
    }
    // RankingMetrics evaluateRanking(int[] u, int[] i, int topN, int[] exclU, int[] exclI): the ranks and their hit rate,
    // precision, recall, NDCG at topN and MRR (means over the users that have a pair)
    std::pair<mfsgd_ranking_metrics, std::vector<int32_t>> evaluateRanking(const std::vector<int32_t>& u,
                                                                           const std::vector<int32_t>& i, int topn,
                                                                           const std::vector<int32_t>& excl_u = {},
                                                                           const std::vector<int32_t>& excl_i = {}) {
        if (u.size() != i.size() || excl_u.size() != excl_i.size()) throw std::invalid_argument("length mismatch");
        mfsgd_ranking_metrics m{};
        std::vector<int32_t> ranks(u.size());
        check(mfsgd_evaluate_ranking(h_, u.data(), i.data(), (int64_t)u.size(), topn, excl_u.data(), excl_i.data(),
                                     (int64_t)excl_u.size(), &m, ranks.data()));
        return {m, std::move(ranks)};
    }

    // The seen-item index: what each user has already seen, built once on the device and kept there, so that the
    // ...Unseen calls below serve "items this user has not seen" without the pair list.
    // void setSeen(int[] u, int[] i): the index becomes the distinct pairs; markSeen: their union with the index (a merge
    // on the device, the index is not sorted again); clearSeen: no index; long seenSize(): its pairs, -1 without one
    void setSeen(const std::vector<int32_t>& u, const std::vector<int32_t>& i) {
        if (u.size() != i.size()) throw std::invalid_argument("length mismatch");
        check(mfsgd_set_seen(h_, u.data(), i.data(), (int64_t)u.size()));
    }
    void markSeen(const std::vector<int32_t>& u, const std::vector<int32_t>& i) {
        if (u.size() != i.size()) throw std::invalid_argument("length mismatch");
        check(mfsgd_mark_seen(h_, u.data(), i.data(), (int64_t)u.size()));
    }
    void clearSeen() { check(mfsgd_clear_seen(h_)); }
    int64_t seenSize() {
        int64_t n = -1;
        check(mfsgd_seen_size(h_, &n));
        return n;
    }
    // {long[] rowPtr, int[] items} seen(int[] users): the requested users' seen items, ascending within a user, CSR over
    // users as given
    std::pair<std::vector<int64_t>, std::vector<int32_t>> seen(const std::vector<int32_t>& users) {
        std::vector<int64_t> ptr(users.size() + 1, 0);
        check(mfsgd_get_seen(h_, users.data(), (int32_t)users.size(), ptr.data(), nullptr, 0));
        std::vector<int32_t> items((size_t)ptr.back());
        if (!items.empty())
            check(mfsgd_get_seen(h_, users.data(), (int32_t)users.size(), ptr.data(), items.data(), (int64_t)items.size()));
        return {std::move(ptr), std::move(items)};
    }
    // int[][] recommendUnseen(int[] users, int topN): recommend(users, topN, exclU, exclI) with the index's pairs
    TopN recommendUnseen(const std::vector<int32_t>& users, int topn) {
        TopN out = top_n(users.size(), topn);
        check(mfsgd_recommend_unseen(h_, users.data(), (int32_t)users.size(), topn, out.first.data(), out.second.data()));
        return out;
    }
    // int[][] recommendUnseenAmong(int[] users, int topN, long[] candPtr, int[] candItems): recommendAmong likewise
    TopN recommendUnseenAmong(const std::vector<int32_t>& users, int topn,
                              const std::vector<int64_t>& cand_ptr,
                              const std::vector<int32_t>& cand_items) {
        if (!cand_ptr.empty() && cand_ptr.size() != users.size() + 1) throw std::invalid_argument("length mismatch");
        TopN out = top_n(users.size(), topn);
        check(mfsgd_recommend_unseen_among(h_, users.data(), (int32_t)users.size(), topn,
                                           cand_ptr.empty() ? nullptr : cand_ptr.data(), cand_items.data(),
                                           (int64_t)cand_items.size(), out.first.data(), out.second.data()));
        return out;
    }
    // int[] rankItemsUnseen(int[] u, int[] i) / RankingMetrics evaluateRankingUnseen(int[] u, int[] i, int topN): rankItems
    // and evaluateRanking with the index's pairs not competing
    std::vector<int32_t> rankItemsUnseen(const std::vector<int32_t>& u, const std::vector<int32_t>& i) {
        if (u.size() != i.size()) throw std::invalid_argument("length mismatch");
        std::vector<int32_t> ranks(u.size());
        check(mfsgd_rank_items_unseen(h_, u.data(), i.data(), (int64_t)u.size(), ranks.data()));
        return ranks;
    }
    std::pair<mfsgd_ranking_metrics, std::vector<int32_t>> evaluateRankingUnseen(const std::vector<int32_t>& u,
                                                                                 const std::vector<int32_t>& i, int topn) {
        if (u.size() != i.size()) throw std::invalid_argument("length mismatch");
        mfsgd_ranking_metrics m{};
        std::vector<int32_t> ranks(u.size());
        check(mfsgd_evaluate_ranking_unseen(h_, u.data(), i.data(), (int64_t)u.size(), topn, &m, ranks.data()));
        return {m, std::move(ranks)};
    }

    double rmse() {
        double out = 0.0;
        check(mfsgd_rmse(h_, &out));
        return out;
    }

    // void setHyper(float lr, float lambda): another lr and lambda for the live model; the schedules are re-baked in
    // place, nothing is rebuilt, the factors stay
    void setHyper(float lr, float lambda) { check(mfsgd_set_hyper(h_, lr, lambda)); }
    // {lr, lambda} the model holds now
    std::pair<float, float> hyper() {
        float lr = 0.f, lambda = 0.f;
        check(mfsgd_get_hyper(h_, &lr, &lambda));
        return {lr, lambda};
    }
    // double[] trainSchedule(float[] lr, float[] lambda /*nullable*/): one epoch per entry over the ratings of the last
    // train() call, epoch e at lr[e] and lambda[e]; the RMSE after each epoch.  The model keeps the last epoch's values
    std::vector<double> trainSchedule(const std::vector<float>& lr, const std::vector<float>* lambda = nullptr) {
        if (lambda && lambda->size() != lr.size()) throw std::invalid_argument("length mismatch");
        std::vector<double> rmse(lr.size());
        check(mfsgd_train_schedule(h_, (int32_t)lr.size(), lr.data(), lambda ? lambda->data() : nullptr, rmse.data()));
        return rmse;
    }
    // double[] trainBoldDriver(int epochs, float up, float down, float[] lrUsed): the rate grows by `up` after an epoch
    // that lowered the RMSE and shrinks by `down` otherwise; {lrUsed, rmse}, one entry per epoch each
    std::pair<std::vector<float>, std::vector<double>> trainBoldDriver(int epochs, float up = 1.05f, float down = 0.5f) {
        if (epochs < 0) throw std::invalid_argument("negative epochs");
        std::vector<float> used((size_t)epochs);
        std::vector<double> rmse((size_t)epochs);
        check(mfsgd_train_bold_driver(h_, epochs, up, down, used.data(), rmse.data()));
        return {std::move(used), std::move(rmse)};
    }

    // ---- online updates -----------------------------------------------------------------------------------------------
    // float[] partialFit(int[] u, int[] i, float[] r): applies the ratings to the live model in the order given, bit for
    // bit the sequential per-rating loop at the current lr / lambda (include/mfsgd.h, "online updates"); returns each
    // rating's error just before its own update.  The stored ratings, their schedules and the held-out set are not
    // touched, and none is needed.  info (nullable): pieces, levels, widest level, kernel launches
    std::vector<float> partialFit(const std::vector<int32_t>& u, const std::vector<int32_t>& i, const std::vector<float>& r,
                                  mfsgd_online_info* info = nullptr) {
        if (u.size() != i.size() || u.size() != r.size()) throw std::invalid_argument("length mismatch");
        std::vector<float> err(u.size());
        check(mfsgd_apply_ratings(h_, u.data(), i.data(), r.data(), (int64_t)u.size(), err.data(), info));
        return err;
    }
    // int[] onlineLevels(int[] u, int[] i): the dependency level of every rating inside its piece, as partialFit would
    // run the list; host only
    std::vector<int32_t> onlineLevels(const std::vector<int32_t>& u, const std::vector<int32_t>& i, mfsgd_online_info* info = nullptr) {
        if (u.size() != i.size()) throw std::invalid_argument("length mismatch");
        std::vector<int32_t> level(u.size());
        check(mfsgd_online_levels(h_, u.data(), i.data(), (int64_t)u.size(), level.data(), info));
        return level;
    }

    // ---- held-out validation and early stopping on it ------------------------------------------------------------------
    // void setValidation(int[] u, int[] i, float[] r): the held-out set of the model, copied and kept on the device from
    // the first call that measures it; empty arrays clear it
    void setValidation(const std::vector<int32_t>& u, const std::vector<int32_t>& i, const std::vector<float>& r) {
        if (u.size() != i.size() || u.size() != r.size()) throw std::invalid_argument("length mismatch");
        check(mfsgd_set_validation(h_, u.data(), i.data(), r.data(), (int64_t)u.size()));
    }
    int64_t validationSize() {
        int64_t n = 0;
        check(mfsgd_validation_size(h_, &n));
        return n;
    }
    // double validationRmse(): RMSE of the held-out set under the current factors (sse, nullable: the sum of squares)
    double validationRmse(double* sse = nullptr) {
        double out = 0.0;
        check(mfsgd_validation_rmse(h_, &out, sse));
        return out;
    }
    // double rmseOn(int[] u, int[] i, float[] r): the same for pairs of the caller's; nothing is kept
    double rmseOn(const std::vector<int32_t>& u, const std::vector<int32_t>& i, const std::vector<float>& r, double* sse = nullptr) {
        if (u.size() != i.size() || u.size() != r.size()) throw std::invalid_argument("length mismatch");
        double out = 0.0;
        check(mfsgd_rmse_pairs(h_, u.data(), i.data(), r.data(), (int64_t)u.size(), &out, sse));
        return out;
    }
    // EarlyStopping trainEarlyStopping(int maxEpochs, int patience, double minDelta, boolean restoreBest, float[] lr,
    // float[] lambda, boolean trainRmse): trains until the held-out RMSE has not improved by more than minDelta for
    // `patience` epochs in a row (include/mfsgd.h states the rule); with restoreBest the model ends with the factors of
    // the best epoch.  lr / lambda: nullable, maxEpochs entries.  valRmse / trainRmse hold epochsRun entries
    struct EarlyStopping {
        std::vector<double> valRmse, trainRmse;
        int32_t epochsRun = 0, bestEpoch = -1;
    };
    EarlyStopping trainEarlyStopping(int maxEpochs, int patience = 3, double minDelta = 0.0, bool restoreBest = true,
                                     const std::vector<float>* lr = nullptr, const std::vector<float>* lambda = nullptr,
                                     bool trainRmse = false) {
        if (maxEpochs < 0) throw std::invalid_argument("negative maxEpochs");
        if ((lr && lr->size() != (size_t)maxEpochs) || (lambda && lambda->size() != (size_t)maxEpochs))
            throw std::invalid_argument("length mismatch");
        EarlyStopping out;
        out.valRmse.resize((size_t)maxEpochs);
        if (trainRmse) out.trainRmse.resize((size_t)maxEpochs);
        const int rc = mfsgd_train_early_stop(h_, maxEpochs, patience, minDelta, restoreBest ? 1 : 0, lr ? lr->data() : nullptr,
                                              lambda ? lambda->data() : nullptr, out.valRmse.data(),
                                              trainRmse ? out.trainRmse.data() : nullptr, &out.epochsRun, &out.bestEpoch);
        check(rc);
        out.valRmse.resize((size_t)out.epochsRun);
        if (trainRmse) out.trainRmse.resize((size_t)out.epochsRun);
        return out;
    }

    std::pair<std::vector<float>, std::vector<float>> factors() {
        std::vector<float> p((size_t)users_ * k_), q((size_t)items_ * k_);
        check(mfsgd_get_factors(h_, p.data(), q.data()));
        return {std::move(p), std::move(q)};
    }

    // ---- DSGD over the GPUs of one node: Java distributedId() / plan() / trainDistributed() / itemBlocks() ---------
    using RingId = std::array<unsigned char, MFSGD_DSGD_ID_BYTES>;
    static RingId distributedId() {
        RingId id{};
        if (mfsgd_dsgd_unique_id(id.data()) != MFSGD_OK) throw std::runtime_error(mfsgd_dsgd_last_error(nullptr));
        return id;
    }
    // {userBegin[nParts + 1], itemPart[items]}
    static std::pair<std::vector<int32_t>, std::vector<int32_t>> plan(const std::vector<int64_t>& deg_user,
                                                                       const std::vector<int64_t>& deg_item, int n_parts) {
        std::vector<int32_t> ub((size_t)n_parts + 1), ip(deg_item.size());
        if (mfsgd_dsgd_plan(deg_user.data(), deg_item.data(), (int32_t)deg_user.size(), (int32_t)deg_item.size(), n_parts, ub.data(),
                            ip.data()) != MFSGD_OK)
            throw std::invalid_argument("plan: bad argument");
        return {std::move(ub), std::move(ip)};
    }
    // double[] trainDistributed(u, i, r, epochs, rank, world, id, itemPart /*nullable*/, userOffset, usersTotal):
    // u are LOCAL user indices, i global item indices; collective; returns the global RMSE after each epoch
    std::vector<double> trainDistributed(const std::vector<int32_t>& u, const std::vector<int32_t>& i, const std::vector<float>& r,
                                         int epochs, int rank, int world, const RingId& id, const std::vector<int32_t>* item_part,
                                         long long user_offset, long long users_total) {
        if (n_parts_ < 2) throw std::logic_error("created without item partitions");
        if (u.size() != i.size() || u.size() != r.size()) throw std::invalid_argument("length mismatch");
        if (!ring_) {
            if (item_part) {
                if ((int)item_part->size() != items_) throw std::invalid_argument("itemPart must have one entry per item");
                check(mfsgd_set_item_partition(h_, item_part->data()));
            }
            check(mfsgd_set_ratings(h_, u.data(), i.data(), r.data(), (int64_t)u.size()));
            check(mfsgd_init_p_offset(h_, seed_, user_offset));
            if (mfsgd_dsgd_create(h_, rank, world, id.data(), &ring_) != MFSGD_OK) throw std::runtime_error(mfsgd_dsgd_last_error(nullptr));
            slots_ = n_parts_ / world;
            dcheck(mfsgd_dsgd_init_q(ring_, seed_, users_total));
            initialised_ = true;
        }
        std::vector<double> rmse((size_t)epochs, 0.0);
        dcheck(mfsgd_dsgd_train(ring_, epochs, rmse.data()));
        return rmse;
    }
    double rmseDistributed() {
        double out = 0.0;
        dcheck(mfsgd_dsgd_rmse(ring_, &out));
        return out;
    }
    std::vector<float> userFactors() {
        std::vector<float> p((size_t)users_ * k_);
        check(mfsgd_get_factors(h_, p.data(), nullptr));
        return p;
    }
    // the Q blocks held between epochs: {partition id, rows x k block} per slot
    std::vector<std::pair<int, std::vector<float>>> itemBlocks() {
        std::vector<std::pair<int, std::vector<float>>> out;
        for (int j = 0; j < slots_; ++j) {
            int32_t part = 0, rows = 0;
            dcheck(mfsgd_dsgd_get_q(ring_, j, &part, &rows, nullptr));
            std::vector<float> blk((size_t)rows * k_);
            dcheck(mfsgd_dsgd_get_q(ring_, j, &part, &rows, blk.data()));
            out.emplace_back(part, std::move(blk));
        }
        return out;
    }
    // {sub-epoch trainings, of those with the recovery point, of those re-run as round launches, bytes sent}
    std::array<long long, 4> ringStats() {
        int64_t s[4] = {0, 0, 0, 0};
        if (ring_) mfsgd_dsgd_stats(ring_, s);
        return {s[0], s[1], s[2], s[3]};
    }

    void close() {
        if (ring_) mfsgd_dsgd_destroy(ring_);
        ring_ = nullptr;
        if (h_) mfsgd_destroy(h_);
        h_ = nullptr;
    }

   private:
    using FoldInCall = int (*)(mfsgd_handle*, int32_t, const int64_t*, const int32_t*, const float*, int32_t, const float*,
                               int64_t, float*);
    std::vector<float> foldIn(const std::vector<int64_t>& row_ptr, const std::vector<int32_t>& ids,
                              const std::vector<float>& ratings, int epochs, const float* init, int64_t seed,
                              FoldInCall call = mfsgd_fold_in_users) {
        if (row_ptr.empty() || ids.size() != ratings.size() || (int64_t)ids.size() != row_ptr.back())
            throw std::invalid_argument("length mismatch");
        std::vector<float> rows((row_ptr.size() - 1) * (size_t)k_);
        check(call(h_, (int32_t)(row_ptr.size() - 1), row_ptr.data(), ids.data(), ratings.data(), epochs, init, seed,
                   rows.data()));
        return rows;
    }
    int append(int (*call)(mfsgd_handle*, int32_t, const float*, int64_t, int32_t*), int& count, const std::vector<float>* rows,
               int n, int64_t seed) {
        if (rows && rows->size() % (size_t)k_ != 0) throw std::invalid_argument("rows must be n x k");
        if (rows) n = (int)(rows->size() / (size_t)k_);
        int32_t first = -1;
        check(call(h_, n, rows ? rows->data() : nullptr, seed, &first));
        count += n;
        return first;
    }
    // the two vectors of a top-N result, n x topn entries each, for the C call to fill
    static TopN top_n(size_t n, int topn) {
        return {std::vector<int32_t>(n * (size_t)topn), std::vector<float>(n * (size_t)topn)};
    }
    void check(int rc) {
        if (rc != MFSGD_OK) throw std::runtime_error(mfsgd_last_error(h_));
    }
    void dcheck(int rc) {
        if (rc != MFSGD_OK) throw std::runtime_error(mfsgd_dsgd_last_error(ring_));
    }
    mfsgd_handle* h_ = nullptr;
    mfsgd_dsgd* ring_ = nullptr;
    int users_, items_, k_, n_parts_, slots_ = 0;
    long long seed_;
    bool initialised_ = false;
};
