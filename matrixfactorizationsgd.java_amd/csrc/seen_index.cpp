// seen_index.cpp -- the seen-item index of a handle, behind the entry points of handle.cpp: mfsgd_set_seen builds it from
// (user, item) pairs, mfsgd_mark_seen merges a batch into it without sorting it again, mfsgd_get_seen reads lists back,
// and the growth calls extend its per-user tables here; so are the item weights (mfsgd_set_item_weights and its kin).  The
// index itself is described in handle.hpp (Seen), its device code is seen.hip, and the calls that read it are serve_topn.cpp's and serve_rank.cpp's
// (_unseen) and sampling.cpp's (mfsgd_sample_unseen and its kin).
#include <algorithm>
#include <cstring>

#include "handle.hpp"
#include "serve_util.hpp"

namespace mfsgd {

// The argument checks of set_seen and mark_seen; `call` ends in ": ".
static int check_pairs(const mfsgd_handle* h, const std::string& call, const int32_t* u, const int32_t* i, int64_t n) {
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n is negative");
    if (n > 0 && (!u || !i)) return fail(h, MFSGD_ERR_INVALID_ARG, call + "u or i is null");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    const int64_t x = first_outside(u, h->cfg.n_users, i, h->cfg.n_items, n);
    if (x >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "pair " + std::to_string(x) + " out of range");
    if (n > (int64_t)UINT32_MAX) return fail(h, MFSGD_ERR_INVALID_ARG, call + "more than 2^32 - 1 pairs");
    return MFSGD_OK;
}

// keys[x] = u[x] << 32 | i[x] for the n pairs, which go up in chunks of bounded size through staging that is gone when
// this returns.  Asynchronous but for the synchronise before a staging buffer is reused.
template <class Bad>
static int pairs_to_keys(mfsgd_handle* h, const Bad& bad, const int32_t* u, const int32_t* i, int64_t n, unsigned long long* keys) {
    DevArray<int32_t> cu, ci;
    const int64_t chunk = std::min(n, kExclChunk);
    int rc;
    if ((rc = dev_alloc(h, cu, (size_t)chunk)) || (rc = dev_alloc(h, ci, (size_t)chunk))) return rc;
    for (int64_t x0 = 0; x0 < n; x0 += chunk) {
        const int64_t c = std::min(chunk, n - x0);
        HIPCHK_OR(bad, copy_up(cu, u + x0, (size_t)c, h->stream));
        HIPCHK_OR(bad, copy_up(ci, i + x0, (size_t)c, h->stream));
        HIPCHK_OR(bad, seen_pair_keys(cu.data(), ci.data(), c, keys + x0, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));  // (pageable memory: the copies have read the caller's arrays)
    }
    return MFSGD_OK;
}

// The unseen-mass table (handle.hpp, Seen::mass) of an index {off, items} of n > 0 pairs under the weights w: complete,
// with the device idle, when this returns; its scratch (8 n bytes of scanned weights, and rocPRIM's) is gone by then.
// Weights set for fewer items than the model has now count the items appended since as weightless, so the table of a
// handle whose weights are stale is still well defined (the draw refuses until they are set again).
static int seen_mass_build(mfsgd_handle* h, const std::string& call, const ItemWeights& w, const long long* off, const int32_t* items,
                           int64_t n, int32_t cap, DevArray<unsigned long long>& mass) {
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    DevArray<unsigned long long> scanned;
    DevBuf temp;  // the rocPRIM scratch, bytes of no type
    int rc;
    if ((rc = dev_alloc(h, mass, (size_t)n)) || (rc = dev_alloc(h, scanned, (size_t)n))) return rc;
    HIPCHK_OR(bad, seen_unseen_mass(off, items, n, cap, w.C.data(), w.n, scanned.data(), mass.data(), temp, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

// A whole index from n > 0 checked pairs, complete before it takes the place of the one the handle has.
static int seen_build(mfsgd_handle* h, const std::string& call, const int32_t* u, const int32_t* i, int64_t n) {
    int rc = ensure_device(h);
    if (rc) return rc;
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    const int32_t cap = h->user_capacity();
    Seen made;
    {
        DevArray<unsigned long long> keys;
        DevBuf keys_tmp;  // read under two types: the sort's second key buffer, then the int32 items of the lists at its start
        DevArray<unsigned> count;
        DevBuf temp;  // the rocPRIM scratch, bytes of no type
        if ((rc = dev_alloc(h, keys, (size_t)n))) return rc;
        if ((rc = dev_alloc(h, keys_tmp, sizeof(unsigned long long) * (size_t)n))) return rc;
        if ((rc = dev_alloc(h, count, 4))) return rc;
        if ((rc = dev_alloc(h, made.off, (size_t)cap + 1)) || (rc = dev_alloc(h, made.slot, (size_t)cap))) return rc;
        if ((rc = pairs_to_keys(h, bad, u, i, n, keys.data()))) return rc;
        // the slots are the users up to the capacity: off[x] of a user without pairs, and of those above the count, is
        // where the next user's keys start.  The items land in keys_tmp, which the sort is done with by then.
        HIPCHK_OR(bad, recommend_excl_lists(keys.data(), keys_tmp.as<unsigned long long>(), n, cap, count.data(), made.off.data(),
                                            keys_tmp.as<int32_t>(), temp, h->stream));
        unsigned distinct = 0;
        HIPCHK_OR(bad, copy_down(&distinct, count, 1, h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
        made.n = (int64_t)distinct;
        if ((rc = dev_alloc(h, made.items, (size_t)made.n))) return rc;
        HIPCHK_OR(bad, hipMemcpyAsync(made.items.data(), keys_tmp.get(), sizeof(int32_t) * (size_t)made.n, hipMemcpyDeviceToDevice,
                                      h->stream));
        HIPCHK_OR(bad, seen_tables(nullptr, 0, 0, cap, nullptr, made.slot.data(), h->stream));
        HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    }
    if (h->weights.present &&
        (rc = seen_mass_build(h, call, h->weights, made.off.data(), made.items.data(), made.n, cap, made.mass)))
        return rc;
    made.present = true;
    made.capacity = cap;
    h->seen = std::move(made);
    return MFSGD_OK;
}

// The union of the index (which has items) and n > 0 checked pairs.
static int seen_merge_batch(mfsgd_handle* h, const std::string& call, const int32_t* u, const int32_t* i, int64_t n) {
    int rc = ensure_device(h);
    if (rc) return rc;
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    Seen& old = h->seen;
    DevArray<unsigned long long> keys, keys_tmp;
    DevArray<unsigned char> flags;
    DevArray<unsigned> count;
    DevArray<long long> off2;
    DevArray<int32_t> items2;
    DevBuf temp;  // the rocPRIM scratch, bytes of no type
    if ((rc = dev_alloc(h, keys, (size_t)n)) || (rc = dev_alloc(h, keys_tmp, (size_t)n))) return rc;
    if ((rc = dev_alloc(h, flags, (size_t)n))) return rc;
    if ((rc = dev_alloc(h, count, 4))) return rc;  // [0] distinct keys of the batch, [1] those the index does not hold
    if ((rc = pairs_to_keys(h, bad, u, i, n, keys.data()))) return rc;
    HIPCHK_OR(bad, seen_batch_fresh(keys.data(), keys_tmp.data(), n, h->cfg.n_users, old.off.data(), old.items.data(), flags.data(),
                                    count.data(), temp, h->stream));
    unsigned counts[2] = {0, 0};
    HIPCHK_OR(bad, copy_down(counts, count, 2, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    const int64_t fresh = (int64_t)counts[1];
    if (fresh == 0) return MFSGD_OK;
    if (old.n + fresh > (int64_t)UINT32_MAX) return fail(h, MFSGD_ERR_INVALID_ARG, call + "more than 2^32 - 1 pairs");
    if ((rc = dev_alloc(h, off2, (size_t)old.capacity + 1)) || (rc = dev_alloc(h, items2, (size_t)(old.n + fresh)))) return rc;
    HIPCHK_OR(bad, seen_merge(old.off.data(), old.items.data(), old.n, old.capacity, keys_tmp.data(), fresh, off2.data(),
                              items2.data(), h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    if (h->weights.present) {  // the merged index's unseen-mass table, before anything of the old index is released
        DevArray<unsigned long long> mass2;
        if ((rc = seen_mass_build(h, call, h->weights, off2.data(), items2.data(), old.n + fresh, old.capacity, mass2))) return rc;
        old.mass = std::move(mass2);
    }
    old.off = std::move(off2);
    old.items = std::move(items2);
    old.n += fresh;
    return MFSGD_OK;
}

// Body of mfsgd_set_seen (merge == false) and mfsgd_mark_seen (handle.cpp).
int seen_update(mfsgd_handle* h, const char* name, bool merge, const int32_t* u, const int32_t* i, int64_t n) {
    const std::string call = std::string(name) + ": ";
    if (const int rc = check_pairs(h, call, u, i, n)) return rc;
    if (merge && h->seen.present && h->seen.n > 0) return n == 0 ? MFSGD_OK : seen_merge_batch(h, call, u, i, n);
    if (n == 0) {  // host only: an empty index holds nothing on the device
        if (!merge || !h->seen.present) h->seen = Seen{};
        h->seen.present = true;
        return MFSGD_OK;
    }
    return seen_build(h, call, u, i, n);
}

int seen_grown_tables(mfsgd_handle* h, const char* prefix, int32_t new_cap, DevArray<long long>& off2, DevArray<int32_t>& slot2) {
    const Seen& s = h->seen;
    if (s.n == 0 || new_cap <= s.capacity) return MFSGD_OK;
    int rc = ensure_device(h);
    if (rc) return rc;
    if ((rc = dev_alloc(h, off2, (size_t)new_cap + 1)) || (rc = dev_alloc(h, slot2, (size_t)new_cap))) return rc;
    const hipError_t e = seen_tables(s.off.data(), s.capacity, s.n, new_cap, off2.data(), slot2.data(), h->stream);
    if (e != hipSuccess) return serve_fail(h, prefix, e);
    return MFSGD_OK;
}

void seen_adopt_tables(mfsgd_handle* h, int32_t new_cap, DevArray<long long>& off2, DevArray<int32_t>& slot2) {
    if (!off2) return;
    h->seen.off = std::move(off2);
    h->seen.slot = std::move(slot2);
    h->seen.capacity = new_cap;
}

// Body of mfsgd_get_seen (handle.cpp).
int seen_get(mfsgd_handle* h, const int32_t* users, int32_t n_users, int64_t* row_ptr, int32_t* items, int64_t items_capacity) {
    if (n_users < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "get_seen: n_users is negative");
    if (!row_ptr) return fail(h, MFSGD_ERR_INVALID_ARG, "get_seen: row_ptr is null");
    if (n_users > 0 && !users) return fail(h, MFSGD_ERR_INVALID_ARG, "get_seen: users is null");
    if (items && items_capacity < 0) return fail(h, MFSGD_ERR_INVALID_ARG, "get_seen: items_capacity is negative");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "get_seen: single-partition handles only");
    if (!h->seen.present) return fail(h, MFSGD_ERR_STATE, "get_seen: no seen set");
    const int64_t j_bad = first_outside(users, n_users, h->cfg.n_users);
    if (j_bad >= 0) return fail(h, MFSGD_ERR_INVALID_ARG, "get_seen: user " + std::to_string(j_bad) + " out of range");
    std::fill(row_ptr, row_ptr + (size_t)n_users + 1, (int64_t)0);
    const Seen& s = h->seen;
    if (n_users == 0 || s.n == 0) return MFSGD_OK;
    int rc = ensure_device(h);
    if (rc) return rc;
    auto bad = [h](hipError_t e) { return serve_fail(h, "get_seen: ", e); };
    DevArray<int32_t> d_users, d_out;
    DevArray<long long> d_ptr;
    if ((rc = dev_alloc(h, d_users, (size_t)n_users)) || (rc = dev_alloc(h, d_ptr, (size_t)n_users + 1))) return rc;
    HIPCHK_OR(bad, copy_up(d_users, users, (size_t)n_users, h->stream));
    HIPCHK_OR(bad, seen_lengths(s.off.data(), d_users.data(), n_users, d_ptr.data() + 1, h->stream));
    HIPCHK_OR(bad, copy_down(row_ptr + 1, d_ptr, (size_t)n_users, h->stream, 1));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    int64_t longest = 0;
    for (int32_t j = 0; j < n_users; ++j) {  // lengths to offsets
        longest = std::max(longest, row_ptr[j + 1]);
        row_ptr[j + 1] += row_ptr[j];
    }
    const int64_t total = row_ptr[n_users];
    if (!items) return MFSGD_OK;
    if (items_capacity < total)
        return fail(h, MFSGD_ERR_INVALID_ARG,
                    "get_seen: items_capacity is " + std::to_string(items_capacity) + ", the lists hold " + std::to_string(total));
    if (total == 0) return MFSGD_OK;
    if ((rc = dev_alloc(h, d_out, (size_t)total))) return rc;
    HIPCHK_OR(bad, copy_up(d_ptr, row_ptr, (size_t)n_users + 1, h->stream));
    HIPCHK_OR(bad, seen_gather(s.off.data(), s.items.data(), d_users.data(), n_users, d_ptr.data(), longest, d_out.data(), h->stream));
    HIPCHK_OR(bad, copy_down(items, d_out, (size_t)total, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

// Body of mfsgd_set_item_weights (handle.cpp).  The prefix is summed on the host (8 (n + 1) bytes, once per call) and goes
// up whole; with an index that has pairs the unseen-mass table follows.  Both are complete before either takes the place
// of what the handle has.
int weights_set(mfsgd_handle* h, const uint32_t* w, int32_t n) {
    const std::string call = "set_item_weights: ";
    if (n < 0) return fail(h, MFSGD_ERR_INVALID_ARG, call + "n is negative");
    if (!w) return fail(h, MFSGD_ERR_INVALID_ARG, call + "w is null");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, call + "single-partition handles only");
    if (n != h->cfg.n_items)
        return fail(h, MFSGD_ERR_INVALID_ARG, call + "n is " + std::to_string(n) + ", the model has " + std::to_string(h->cfg.n_items) + " items");
    int rc = ensure_device(h);
    if (rc) return rc;
    auto bad = [h, &call](hipError_t e) { return serve_fail(h, call.c_str(), e); };
    std::vector<unsigned long long> prefix((size_t)n + 1);
    prefix[0] = 0;
    for (int32_t x = 0; x < n; ++x) prefix[(size_t)x + 1] = prefix[x] + w[x];  // (below 2^31 * 2^32: no wrap)
    ItemWeights made;
    DevArray<unsigned long long> mass;
    if ((rc = dev_alloc(h, made.C, prefix.size()))) return rc;
    HIPCHK_OR(bad, copy_up(made.C, prefix.data(), prefix.size(), h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    made.present = true;
    made.n = n;
    const Seen& s = h->seen;
    if (s.n > 0 && (rc = seen_mass_build(h, call, made, s.off.data(), s.items.data(), s.n, s.capacity, mass))) return rc;
    h->weights = std::move(made);
    if (mass) h->seen.mass = std::move(mass);
    return MFSGD_OK;
}

// Body of mfsgd_get_item_weights (handle.cpp): the differences of the prefix, for the item count it was set for.
int weights_get(mfsgd_handle* h, uint32_t* w, int32_t* n) {
    if (!n) return fail(h, MFSGD_ERR_INVALID_ARG, "get_item_weights: n is null");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "get_item_weights: single-partition handles only");
    const ItemWeights& iw = h->weights;
    *n = iw.present ? iw.n : -1;
    if (!iw.present || !w) return MFSGD_OK;
    int rc = ensure_device(h);
    if (rc) return rc;
    auto bad = [h](hipError_t e) { return serve_fail(h, "get_item_weights: ", e); };
    std::vector<unsigned long long> prefix((size_t)iw.n + 1);
    HIPCHK_OR(bad, copy_down(prefix.data(), iw.C, prefix.size(), h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    for (int32_t x = 0; x < iw.n; ++x) w[x] = (uint32_t)(prefix[(size_t)x + 1] - prefix[x]);
    return MFSGD_OK;
}

// Body of mfsgd_clear_item_weights (handle.cpp).
int weights_clear(mfsgd_handle* h) {
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "clear_item_weights: single-partition handles only");
    if (h->device_ready) {
        (void)hipSetDevice(h->cfg.device);
        (void)hipStreamSynchronize(h->stream);
    }
    h->weights = ItemWeights{};
    h->seen.mass.reset();
    return MFSGD_OK;
}

// Body of mfsgd_seen_item_counts (handle.cpp).
int seen_item_histogram(mfsgd_handle* h, int64_t* counts) {
    if (!counts) return fail(h, MFSGD_ERR_INVALID_ARG, "seen_item_counts: counts is null");
    if (h->n_parts != 1) return fail(h, MFSGD_ERR_STATE, "seen_item_counts: single-partition handles only");
    if (!h->seen.present) return fail(h, MFSGD_ERR_STATE, "seen_item_counts: no seen set");
    const size_t n_items = (size_t)h->cfg.n_items;
    std::fill(counts, counts + n_items, (int64_t)0);
    const Seen& s = h->seen;
    if (s.n == 0) return MFSGD_OK;  // host only: an empty index holds nothing on the device
    int rc = ensure_device(h);
    if (rc) return rc;
    auto bad = [h](hipError_t e) { return serve_fail(h, "seen_item_counts: ", e); };
    DevArray<long long> d_counts;  // (summed as unsigned: no count reaches 2^63)
    if ((rc = dev_alloc(h, d_counts, n_items))) return rc;
    HIPCHK_OR(bad, hipMemsetAsync(d_counts.data(), 0, sizeof(long long) * n_items, h->stream));
    HIPCHK_OR(bad, seen_item_counts(s.items.data(), s.n, reinterpret_cast<unsigned long long*>(d_counts.data()), h->stream));
    HIPCHK_OR(bad, copy_down(counts, d_counts, n_items, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    return MFSGD_OK;
}

}  // namespace mfsgd
