// sampling.cpp -- the calls that sample among the items a user has NOT seen, behind the entry points of handle.cpp:
// mfsgd_sample_unseen (uniform draws), mfsgd_sample_unseen_weighted (draws by item weight), mfsgd_sample_unseen_hard (the
// best-scoring of a row's draws) and mfsgd_sample_unseen_violating (the first of them that violates a margin), and the
// last two over weighted draws (mfsgd_sample_unseen_hard_weighted, mfsgd_sample_unseen_violating_weighted).  They read
// the seen-item index (handle.hpp, Seen; seen_index.cpp builds it) and share their checks, their pieces and their
// staging, which are stated once, here; the kernels are sample.hip's and pick.hip's.
#include <algorithm>

#include "handle.hpp"
#include "serve_util.hpp"

namespace mfsgd {
namespace {

// What tells the calls apart in the checks they share.
struct Family {
    const char* name;
    int32_t m_min;          // the smallest m: 0 ("m is negative" below it) or 1 ("m is below 1")
    bool reads_factors;     // the picks are made under the factors
    const char* row;        // what the range message calls a row
    bool has_pos = false;   // a positive per row beside its user, and a margin
    bool weighted = false;  // the draw needs item weights, set for the items the model has now
};

// The argument and state checks of the family, in the order include/mfsgd.h states for every one of them, before any
// device work; after MFSGD_OK, n * m == 0 means that there is nothing to do (and nothing was read).  pos_items and
// margin are the call's when it has_pos, and anything (margin: not a NaN) otherwise.
int check_sample(const mfsgd_handle* h, const Family& k, const int32_t* users, const int32_t* pos_items, int64_t n, int32_t m,
                 float margin, int64_t first, const void* out_items) {
    const std::string call = std::string(k.name) + ": ";
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n is negative");
    if (m < k.m_min) return fail(h, MFSGD_ERR_INVALID_ARG, call + (k.m_min > 0 ? "m is below 1" : "m is negative"));
    if (margin != margin) return fail(h, MFSGD_ERR_INVALID_ARG, call + "margin is NaN");
    if (first < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "first is negative");
    if ((m > 0 && n > INT64_MAX / m) || first > INT64_MAX - n * m)
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "first + n * m exceeds 2^63 - 1");
    const bool empty = n * m == 0;
    if (!empty && (!users || (k.has_pos && !pos_items) || !out_items))
        return fail(h, MFSGD_ERR_INVALID_ARG,
                    call + (k.has_pos ? "users, pos_items or out_items is null" : "users or out_items is null"));
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    if (!h->seen.present) return fail(h, MFSGD_ERR_STATE, call + "no seen set");
    const ItemWeights& iw = h->weights;
    if (k.weighted && !iw.present) return fail(h, MFSGD_ERR_STATE, call + "no item weights");
    if (k.weighted && iw.n != h->cfg.n_items)
        return fail(h, MFSGD_ERR_STATE,
                    call + "item weights cover " + std::to_string(iw.n) + " items, the model has " + std::to_string(h->cfg.n_items));
    if (k.reads_factors)
        if (const int rc = check_reads_factors(h, k.name)) return rc;
    if (empty) return MFSGD_OK;
    const int64_t x_bad = k.has_pos ? first_outside(users, h->cfg.n_users, pos_items, h->cfg.n_items, n)
                                    : first_outside(users, n, h->cfg.n_users);
    if (x_bad >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + k.row + " " + std::to_string(x_bad) + " out of range");
    return MFSGD_OK;
}

// An output column of a call, `stride` elements a row: the caller's array U*, null when the call was not asked for it,
// and its staging on the device, which exists only when it was.
template <class T, class U = T>
struct Column {
    mfsgd_handle* h;
    U* out;
    int64_t stride;
    DevArray<T> dev;
    Column(mfsgd_handle* h_, U* out_, int64_t stride_ = 1) : h(h_), out(out_), stride(stride_) {}
    int alloc(int64_t rows) { return out ? dev_alloc(h, dev, (size_t)(rows * stride)) : MFSGD_OK; }
    T* data() const { return out ? dev.data() : nullptr; }
    // the piece of c rows from row x0 on, down to its place
    hipError_t down(int64_t x0, int64_t c) const {
        return out ? copy_down(out + x0 * stride, dev, (size_t)(c * stride), h->stream) : hipSuccess;
    }
};

// The pieces of a call: the rows go up and the draws or picks come down in pieces of whole rows, at most kSampleChunk
// draws or candidates each (a row with more is a piece of its own); draw d of row x has the counter first + x * m + d
// wherever the pieces are cut.  Nothing per candidate is ever stored by the calls that pick.
// piece_rows: the rows of the largest piece, which the staging is sized for.  Per piece of c rows from row x0 on,
// sample_pieces sends its users up, calls launch(the users on the device, x0, c, counter of the piece's first draw) ->
// hipError_t, brings the columns down, everything on h->stream, and synchronises; the staging is gone on return.
int64_t piece_rows(int64_t n, int32_t m) { return std::min(n, std::max<int64_t>(1, kSampleChunk / m)); }

template <class Launch, class... Cols>
int sample_pieces(mfsgd_handle* h, const Family& k, const int32_t* users, int64_t n, int32_t m, int64_t first, Launch&& launch,
                  Cols&... cols) {
    const int64_t rows = piece_rows(n, m);
    DevArray<int32_t> d_users;
    int rc = dev_alloc(h, d_users, (size_t)rows);
    ((rc = rc ? rc : cols.alloc(rows)), ...);
    if (rc) return rc;
    const std::string prefix = std::string(k.name) + ": ";
    for (int64_t x0 = 0; x0 < n; x0 += rows) {
        const int64_t c = std::min(rows, n - x0);
        hipError_t e = copy_up(d_users, users + x0, (size_t)c, h->stream);
        if (e == hipSuccess) e = launch(d_users.data(), x0, c, (uint64_t)first + (uint64_t)(x0 * m));
        ((e = e != hipSuccess ? e : cols.down(x0, c)), ...);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (pageable memory: the staging is free for the next piece)
        if (e != hipSuccess) return serve_fail(h, prefix.c_str(), e);
    }
    return MFSGD_OK;
}

// The lists of the index for a kernel: no offsets when it holds no pairs (every list is empty).
const long long* seen_off(const Seen& s) { return s.n > 0 ? s.off.data() : nullptr; }

}  // namespace

// Body of mfsgd_sample_unseen (handle.cpp): row x of out_items receives m draws among the items users[x] has not seen.
int seen_sample(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first, int32_t* out_items) {
    static const Family k{"sample_unseen", 0, false, "user"};
    int rc = check_sample(h, k, users, nullptr, n, m, 0.0f, first, out_items);
    if (rc || n * m == 0 || (rc = ensure_device(h))) return rc;
    const Seen& s = h->seen;
    Column<int32_t> items(h, out_items, m);
    return sample_pieces(h, k, users, n, m, first, [&](const int32_t* d_users, int64_t, int64_t c, uint64_t c_first) {
        return sample_unseen_draws(seen_off(s), s.items.data(), d_users, c * m, m, h->cfg.n_items, seed, c_first,
                                   items.data(), h->stream);
    }, items);
}

// Body of mfsgd_sample_unseen_weighted (handle.cpp): seen_sample with the weighted draw -- the same pieces, the same
// counters, and a row's unseen weight beside its draws when asked.
int seen_sample_weighted(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                         int32_t* out_items, int64_t* out_mass) {
    static const Family k{"sample_unseen_weighted", 0, false, "user", false, true};
    int rc = check_sample(h, k, users, nullptr, n, m, 0.0f, first, out_items);
    if (rc || n * m == 0) return rc;
    const Seen& s = h->seen;
    if (s.n > 0 && !s.mass)  // (never: it is eager)
        return fail(h, MFSGD_ERR_STATE, "sample_unseen_weighted: the index has no unseen-mass table");
    if ((rc = ensure_device(h))) return rc;
    Column<int32_t> items(h, out_items, m);
    Column<long long, int64_t> mass(h, out_mass);
    return sample_pieces(h, k, users, n, m, first, [&](const int32_t* d_users, int64_t, int64_t c, uint64_t c_first) {
        return sample_weighted_draws(seen_off(s), s.items.data(), s.mass.data(), h->weights.C.data(), d_users, c * m, m,
                                     h->cfg.n_items, seed, c_first, items.data(), mass.data(), h->stream);
    }, items, mass);
}

// Body of mfsgd_sample_unseen_hard (handle.cpp): row x receives the best-scoring of the m draws seen_sample would give it,
// scored under the factors as they are.
int seen_sample_hard(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first, int32_t* out_items,
                     float* out_scores, int32_t* out_draw) {
    static const Family k{"sample_unseen_hard", 1, true, "user"};
    int rc = check_sample(h, k, users, nullptr, n, m, 0.0f, first, out_items);
    if (rc || n == 0 || (rc = factors_to_device(h))) return rc;
    const Seen& s = h->seen;
    Column<int32_t> items(h, out_items), draw(h, out_draw);
    Column<float> scores(h, out_scores);
    return sample_pieces(h, k, users, n, m, first, [&](const int32_t* d_users, int64_t, int64_t c, uint64_t c_first) {
        return launch_hard_negatives(h->geo.L, h->dP.data(), h->dQ.data(), seen_off(s), s.items.data(), d_users, c, m,
                                     h->cfg.n_items, seed, c_first, items.data(), scores.data(), draw.data(), h->stream);
    }, items, scores, draw);
}

// Body of mfsgd_sample_unseen_violating (handle.cpp): row x receives the first of the m draws seen_sample would give it
// that violates the margin against the row's positive, under the factors as they are.
int seen_sample_violating(mfsgd_handle* h, const int32_t* users, const int32_t* pos_items, int64_t n, int32_t m, float margin,
                          int64_t seed, int64_t first, int32_t* out_items, int32_t* out_draw, float* out_margin, int32_t* out_rank) {
    static const Family k{"sample_unseen_violating", 1, true, "row", true};
    int rc = check_sample(h, k, users, pos_items, n, m, margin, first, out_items);
    if (rc || n == 0 || (rc = factors_to_device(h))) return rc;
    const Seen& s = h->seen;
    DevArray<int32_t> d_pos;
    if ((rc = dev_alloc(h, d_pos, (size_t)piece_rows(n, m)))) return rc;
    Column<int32_t> items(h, out_items), draw(h, out_draw), rank(h, out_rank);
    Column<float> margins(h, out_margin);
    return sample_pieces(h, k, users, n, m, first, [&](const int32_t* d_users, int64_t x0, int64_t c, uint64_t c_first) {
        const hipError_t e = copy_up(d_pos, pos_items + x0, (size_t)c, h->stream);
        if (e != hipSuccess) return e;
        return launch_first_violating(h->geo.L, h->dP.data(), h->dQ.data(), seen_off(s), s.items.data(), d_users,
                                      d_pos.data(), c, m, margin, h->cfg.n_items, seed, c_first, items.data(), draw.data(),
                                      margins.data(), rank.data(), h->stream);
    }, items, draw, margins, rank);
}

// The weighted draw of a pick call on a checked handle: the index's mass table, the weights' prefix, the column of the
// rows' unseen weights.
static PickWeights pick_weights(const mfsgd_handle* h, const Column<long long, int64_t>& mass) {
    return PickWeights{h->seen.mass.data(), h->weights.C.data(), mass.data()};
}

// Body of mfsgd_sample_unseen_hard_weighted (handle.cpp): seen_sample_hard over the candidates seen_sample_weighted would
// give the row -- the same pieces and counters, and a row's unseen weight beside its pick when asked.
int seen_sample_hard_weighted(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                              int32_t* out_items, float* out_scores, int32_t* out_draw, int64_t* out_mass) {
    static const Family k{"sample_unseen_hard_weighted", 1, true, "user", false, true};
    int rc = check_sample(h, k, users, nullptr, n, m, 0.0f, first, out_items);
    if (rc || n == 0) return rc;
    const Seen& s = h->seen;
    if (s.n > 0 && !s.mass)  // (never: it is eager)
        return fail(h, MFSGD_ERR_STATE, "sample_unseen_hard_weighted: the index has no unseen-mass table");
    if ((rc = factors_to_device(h))) return rc;
    Column<int32_t> items(h, out_items), draw(h, out_draw);
    Column<float> scores(h, out_scores);
    Column<long long, int64_t> mass(h, out_mass);
    return sample_pieces(h, k, users, n, m, first, [&](const int32_t* d_users, int64_t, int64_t c, uint64_t c_first) {
        return launch_hard_negatives(h->geo.L, h->dP.data(), h->dQ.data(), seen_off(s), s.items.data(), d_users, c, m,
                                     h->cfg.n_items, seed, c_first, items.data(), scores.data(), draw.data(), h->stream,
                                     pick_weights(h, mass));
    }, items, scores, draw, mass);
}

// Body of mfsgd_sample_unseen_violating_weighted (handle.cpp): seen_sample_violating over those candidates.
int seen_sample_violating_weighted(mfsgd_handle* h, const int32_t* users, const int32_t* pos_items, int64_t n, int32_t m,
                                   float margin, int64_t seed, int64_t first, int32_t* out_items, int32_t* out_draw,
                                   float* out_margin, int32_t* out_rank, int64_t* out_mass) {
    static const Family k{"sample_unseen_violating_weighted", 1, true, "row", true, true};
    int rc = check_sample(h, k, users, pos_items, n, m, margin, first, out_items);
    if (rc || n == 0) return rc;
    const Seen& s = h->seen;
    if (s.n > 0 && !s.mass)  // (never: it is eager)
        return fail(h, MFSGD_ERR_STATE, "sample_unseen_violating_weighted: the index has no unseen-mass table");
    if ((rc = factors_to_device(h))) return rc;
    DevArray<int32_t> d_pos;
    if ((rc = dev_alloc(h, d_pos, (size_t)piece_rows(n, m)))) return rc;
    Column<int32_t> items(h, out_items), draw(h, out_draw), rank(h, out_rank);
    Column<float> margins(h, out_margin);
    Column<long long, int64_t> mass(h, out_mass);
    return sample_pieces(h, k, users, n, m, first, [&](const int32_t* d_users, int64_t x0, int64_t c, uint64_t c_first) {
        const hipError_t e = copy_up(d_pos, pos_items + x0, (size_t)c, h->stream);
        if (e != hipSuccess) return e;
        return launch_first_violating(h->geo.L, h->dP.data(), h->dQ.data(), seen_off(s), s.items.data(), d_users,
                                      d_pos.data(), c, m, margin, h->cfg.n_items, seed, c_first, items.data(), draw.data(),
                                      margins.data(), rank.data(), h->stream, pick_weights(h, mass));
    }, items, draw, margins, rank, mass);
}

}  // namespace mfsgd
