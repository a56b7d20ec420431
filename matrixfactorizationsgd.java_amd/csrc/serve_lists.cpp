// serve_lists.cpp -- the steps the serving units share: the row matrix of a call on the device, the check of its
// exclusion pairs, and the lists made of keys there (serve_lists.hpp).
#include "serve_lists.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>

namespace mfsgd {

int KeyLists::alloc(mfsgd_handle* h, int64_t n_keys, int64_t n_slots) {
    int rc;
    if ((rc = alloc_counter(h))) return rc;
    if ((rc = dev_alloc(h, keys, (size_t)n_keys)) || (rc = dev_alloc(h, keys_tmp, (size_t)n_keys))) return rc;
    if ((rc = dev_alloc(h, off, (size_t)n_slots + 1)) || (rc = dev_alloc(h, items, (size_t)n_keys))) return rc;
    return MFSGD_OK;
}

hipError_t KeyLists::finish(int64_t n_keys, int64_t n_slots, DevBuf& temp, hipStream_t st) {
    return recommend_excl_lists(keys.data(), keys_tmp.data(), n_keys, (int32_t)n_slots, count.data() + distinct_at(), off.data(),
                                items.data(), temp, st);
}

std::vector<int32_t> all_rows(int32_t n) {
    std::vector<int32_t> all((size_t)n);
    std::iota(all.begin(), all.end(), 0);
    return all;
}

int upload_rows(mfsgd_handle* h, const float* host_rows, int32_t n_rows, DevArray<float>& buf, const float** rows,
                const DevArray<float> mfsgd_handle::*own) {
    *rows = (h->*own).data();
    if (!host_rows) return MFSGD_OK;
    const int k = h->cfg.k, kp = h->geo.kp;
    std::vector<float> padded((size_t)n_rows * kp, 0.0f);
    for (int64_t x = 0; x < n_rows; ++x) std::memcpy(&padded[(size_t)x * kp], host_rows + x * k, sizeof(float) * (size_t)k);
    const int rc = upload(h, buf, padded);
    *rows = buf.data();
    return rc;
}

int count_exclusions(const mfsgd_handle* h, const ServeName& what, const std::vector<int32_t>& slot_of_user, int32_t n_rows,
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

// The `kept` appended keys made into lists, which `lists` takes over from the scratch, and `ex` pointing into them.
// Ends in a synchronise.
static hipError_t excl_lists_end(mfsgd_handle* h, const Slots& slots, int64_t kept, KeyLists& k, ExclLists& lists, DevBuf& temp,
                                 RecommendExcl& ex) {
    hipError_t e = k.finish(kept, slots.n(), temp, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return e;
    lists.off = std::move(k.off);
    lists.items = std::move(k.items);
    ex = RecommendExcl{lists.slot.data(), lists.off.data(), lists.items.data()};
    return e;
}

int exclusions_to_device(mfsgd_handle* h, const ServeName& what, const Slots& slots, const Exclusions& excl, int64_t kept,
                         ExclLists& lists, DevBuf& temp, RecommendExcl& ex) {
    const std::string prefix = std::string(what.call) + ": exclusion lists: ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    DevArray<int32_t> cu, ci;
    KeyLists k(true);
    const int64_t chunk = std::min(excl.n, kExclChunk);
    int rc;
    if ((rc = upload(h, lists.slot, slots.slot_of_row)) || (rc = k.alloc(h, kept, slots.n()))) return rc;
    if ((rc = dev_alloc(h, cu, (size_t)chunk)) || (rc = dev_alloc(h, ci, (size_t)chunk))) return rc;
    HIPCHK_OR(bad, k.zero_counter(h->stream));
    for (int64_t x0 = 0; x0 < excl.n; x0 += chunk) {
        const int64_t c = std::min(chunk, excl.n - x0);
        HIPCHK_OR(bad, copy_up(cu, excl.u + x0, (size_t)c, h->stream));
        HIPCHK_OR(bad, copy_up(ci, excl.i + x0, (size_t)c, h->stream));
        HIPCHK_OR(bad, recommend_excl_filter(lists.slot.data(), cu.data(), ci.data(), c, k.keys.data(), k.n_appended(), kept, h->stream));
    }
    HIPCHK_OR(bad, excl_lists_end(h, slots, kept, k, lists, temp, ex));
    return MFSGD_OK;
}

int audience_to_device(mfsgd_handle* h, const ServeName& what, const Slots& slots, const Seen& seen, ExclLists& lists, DevBuf& temp,
                       RecommendExcl& ex) {
    const std::string prefix = std::string(what.call) + ": exclusion lists: ";
    auto bad = [h, &prefix](hipError_t e) { return serve_fail(h, prefix.c_str(), e); };
    KeyLists k(true);
    auto pass = [&](unsigned long long* to, int64_t cap) {
        return seen_audience_keys(lists.slot.data(), (int32_t)slots.slot_of_row.size(), seen.off.data(), seen.items.data(),
                                  std::min(h->cfg.n_users, seen.capacity), seen.n, to, k.n_appended(), cap, h->stream);
    };
    unsigned long long kept = 0;
    int rc;
    if ((rc = upload(h, lists.slot, slots.slot_of_row)) || (rc = k.alloc_counter(h))) return rc;
    HIPCHK_OR(bad, k.zero_counter(h->stream));
    HIPCHK_OR(bad, pass(nullptr, 0));
    HIPCHK_OR(bad, hipMemcpyAsync(&kept, k.n_appended(), sizeof(kept), hipMemcpyDeviceToHost, h->stream));
    HIPCHK_OR(bad, hipStreamSynchronize(h->stream));
    if (kept > (unsigned long long)UINT32_MAX)
        return fail(h, MFSGD_ERR_INVALID_ARG, std::string(what.call) + ": more than 2^32 - 1 excluded pairs of " + what.whose);
    if (kept == 0) return MFSGD_OK;
    if ((rc = k.alloc(h, (int64_t)kept, slots.n()))) return rc;
    HIPCHK_OR(bad, k.zero_counter(h->stream));  // (the counter counts again)
    HIPCHK_OR(bad, pass(k.keys.data(), (int64_t)kept));
    HIPCHK_OR(bad, excl_lists_end(h, slots, (int64_t)kept, k, lists, temp, ex));
    return MFSGD_OK;
}

}  // namespace mfsgd
