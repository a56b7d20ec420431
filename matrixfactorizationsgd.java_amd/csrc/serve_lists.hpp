// serve_lists.hpp -- what the serving units share (serve_topn.cpp, serve_rank.cpp, serve_fold.cpp): how a call speaks of
// itself, what it leaves out, its row matrix on the device, and the lists it builds there out of keys.
#pragma once

#include <string>
#include <vector>

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

// The exclusion lists of one call on the device, as RecommendExcl reads them.
struct ExclLists {
    DevArray<int32_t> slot, items;
    DevArray<long long> off;
};

// (what follows is the serving units' own: hidden, so that none of it is in the library's dynamic symbol table)
#pragma GCC visibility push(hidden)

// Keys on the device on their way to lists: slot << 32 | id, written in no particular order, then sorted through
// keys_tmp and made distinct into one ascending CSR list per slot, (off, items) -- recommend.hip.  The exclusion
// lists, the candidate lists and the positives of a pairwise fold-in batch are all made this way; what differs is who
// writes the keys, and so what the 16 bytes of `count` hold.  `appended`: kernels that keep some of their input append
// through it (recommend_excl_filter, seen_audience_keys), the u64 append count at [0], and the u32 distinct count lies
// behind it; otherwise every key has its place (recommend_cand_keys) and the distinct count is the first word.
struct KeyLists {
    const bool appended;
    explicit KeyLists(bool appended_ = false) : appended(appended_) {}
    DevArray<unsigned long long> keys, keys_tmp;
    DevArray<unsigned> count;
    DevArray<long long> off;
    DevArray<int32_t> items;

    unsigned long long* n_appended() const { return reinterpret_cast<unsigned long long*>(count.data()); }
    size_t distinct_at() const { return appended ? 2 : 0; }  // (an index into count)
    // The counter alone, for a pass that counts the keys before there is room for them; the caller zeroes it before
    // each pass that appends or counts.
    int alloc_counter(mfsgd_handle* h) { return dev_alloc(h, count, 4); }
    hipError_t zero_counter(hipStream_t st) { return hipMemsetAsync(count.data(), 0, 16, st); }
    // Room for n_keys keys and for the lists they become: 20 bytes per key (two key buffers and the lists' ids), and an
    // offset per slot.  Buffers that are large enough are kept, so a loop allocates once, for its largest round.
    int alloc(mfsgd_handle* h, int64_t n_keys, int64_t n_slots);
    // The first n_keys keys into the lists of n_slots slots, on st; no synchronise.
    hipError_t finish(int64_t n_keys, int64_t n_slots, DevBuf& temp, hipStream_t st);
};

// Rows 0 .. n - 1, all of them: what the _rows calls ask for.
std::vector<int32_t> all_rows(int32_t n);

// The row matrix of a serving call on the device: the model's P (`own`: or its Q, for an item-side call), or host_rows
// (n_rows x k, dense), which goes up into a kp-padded temporary (`buf`) for the length of the call.
int upload_rows(mfsgd_handle* h, const float* host_rows, int32_t n_rows, DevArray<float>& buf, const float** rows,
                const DevArray<float> mfsgd_handle::*own = &mfsgd_handle::dP);

// Range check of the exclusion pairs (n_scanned: the rows of the scanned side, the model's items unless the call is an
// item-side one), and *kept = how many of them belong to a user that has a slot.
int count_exclusions(const mfsgd_handle* h, const ServeName& what, const std::vector<int32_t>& slot_of_user, int32_t n_rows,
                     int32_t n_scanned, const Exclusions& excl, int64_t* kept);

// Exclusion lists of one recommend call on the device: the pairs go up in chunks of bounded size, those of requested
// users are kept (slot << 32 | item), then sorted and made distinct into one list per slot (KeyLists).
// Scratch lives as long as this function; `ex` points into `lists`, which is the caller's.
// `what` starts the message of a HIP failure: the call the lists are built for.
// (kExclChunk pairs per upload, handle.hpp)
int exclusions_to_device(mfsgd_handle* h, const ServeName& what, const Slots& slots, const Exclusions& excl, int64_t kept,
                         ExclLists& lists, DevBuf& temp, RecommendExcl& ex);

// The same lists for an item-side _unseen call (slots: of the requested items), made of the seen-item index, which is
// CSR by user and cannot be read where it lies for an item: one pass over its pairs counts those of requested items
// -- how many are kept is not known before -- and a second writes them as slot << 32 | user (audience.hip); from there
// they are a caller's pairs.  No pair kept: nothing is built and ex stays empty.  The index's lists are read up to the
// user count (the offsets above it hold the total).  mfsgd_mark_seen keeps an index below 2^32 pairs, so the cap of a
// pair list cannot be met here; it is asked all the same, the lists' counters being 32 bits wide.
int audience_to_device(mfsgd_handle* h, const ServeName& what, const Slots& slots, const Seen& seen, ExclLists& lists, DevBuf& temp,
                       RecommendExcl& ex);

#pragma GCC visibility pop

}  // namespace mfsgd
