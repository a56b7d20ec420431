// handle.hpp -- what the units of the C-ABI that see inside the handle share (handle.cpp, seen_index.cpp, sampling.cpp, ratings.cpp,
// train.cpp, online_update.cpp, serve_lists.cpp, serve_topn.cpp, serve_rank.cpp, serve_fold.cpp): the handle, its partitions, the error channel, the guard with that channel, and the helpers that cross
// units.  Internal: installed nowhere.  dsgd.cpp and io.cpp see the handle through include/mfsgd.h only, and take the
// guard from guard.hpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <map>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mfsgd.h"
#include "devmem.hpp"
#include "guard.hpp"
#include "kernels.hpp"
#include "schedule.hpp"

namespace mfsgd {

struct Part {
    Schedule sched;
    int32_t q_rows = 0;  // rows of this partition's Q block
    // Forwarding and register-resident runs exist on the kernel's q side only.  The update is
    // symmetric in p and q, so when the heaviest USER outweighs the heaviest item the schedule
    // is built with the roles exchanged and the kernels get (Q, P) instead of (P, Q).
    bool swapped = false;
    bool on_device = false;
    DevArray<CellDesc> d_cells;
    DevArray<uint32_t> d_rows;
    DevArray<SubDesc> d_subs;
    DevArray<Entry> d_entries;
    DevBuf d_sse_partial;  // read under two types: the doubles of an SSE pass, or the u64 stamps of a diagnostic launch
    DevArray<double> d_sse_out;
    DevArray<unsigned> d_sync;  // persistent kernel: done[B] words (kDoneStride apart) + the abort word
    int persistent_np = -1;  // co-resident workgroups of the epoch kernel; 0 = use round launches; -1 = not probed
    // training graphs keyed by the (P, Q) pointers they were captured with (both are baked into the
    // kernel node; P changes when the factors are re-seeded, Q with every caller-owned block)
    std::map<std::pair<const void*, const void*>, hipGraphExec_t> graphs;

    Part() = default;
    Part(Part&&) = default;  // (the moved-from map is empty: nothing is destroyed twice)
    ~Part() { drop_graphs(); }
    void drop_graphs() {
        for (auto& kv : graphs)
            if (kv.second) (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
    }
};

// The held-out set of a handle (mfsgd_set_validation): the pairs on the host as given until the first call that needs
// them on the device, there from then on, with the scratch of the SSE pass over them (kPairsSlots partials, then the sum).
struct Validation {
    int64_t n = 0;
    std::vector<int32_t> hu, hi;
    std::vector<float> hr;
    bool on_device = false;
    DevArray<int32_t> du, di;
    DevArray<float> dr;
    DevArray<double> d_sse;
};

// The seen-item index of a handle (mfsgd_set_seen, mfsgd_mark_seen; seen.hip): what each user has already seen, one
// sorted, distinct item list per user in CSR form on the device, where the _unseen serving calls read it.
// present: the handle has an index, which may be empty (n == 0); the tables exist while n > 0.
//   items  n x int32: the list of user u is items[off[u] .. off[u + 1]), ascending
//   off    (capacity + 1) x int64, capacity = the handle's user_capacity() when the tables were made; every entry from
//          the user count on holds n, so users appended inside the capacity have empty lists and need no work
//   slot   capacity x int32, slot[u] = u: {slot, off, items} is a RecommendExcl whose slots are the user ids, so the
//          EXCL kernels of recommend.hip read the index as they read the lists of one call
// 4 n + 12 capacity + 8 bytes in all.  On a handle that has item weights (ItemWeights below) and n > 0, beside them
//   mass   n x uint64, parallel to items: mass[q] = the weight of the items below items[q] that q's user has NOT seen;
//          never decreasing along a list.  What the weighted draw searches (draw.hpp).  8 n bytes more.  It is made by
//          whichever call completes or changes that state (seen_index.cpp, seen_mass_build) and leaves with the index.
struct Seen {
    bool present = false;
    int64_t n = 0;
    int32_t capacity = 0;
    DevArray<long long> off;
    DevArray<int32_t> items, slot;
    DevArray<unsigned long long> mass;
    RecommendExcl excl() const { return n > 0 ? RecommendExcl{slot.data(), off.data(), items.data()} : RecommendExcl{}; }
};

// The item weights of a handle (mfsgd_set_item_weights): C, their exclusive prefix on the device, n + 1 x uint64 with
// C[0] = 0 and C[n] = W < 2^63; n is the item count they were set for, which mfsgd_append_items leaves behind.
struct ItemWeights {
    bool present = false;
    int32_t n = 0;
    DevArray<unsigned long long> C;
};

// Pairs (exclusions, candidates, seen pairs) per upload of a call that reads a caller's list: 32 MB of staging
constexpr int64_t kExclChunk = (int64_t)1 << 22;
// Draws per piece of mfsgd_sample_unseen, whose rows go up and whose draws come down in pieces of whole rows: 16 MB of
// draws and at most as much of rows (one row that asks for more draws is a piece of its own).  Candidates per piece of
// mfsgd_sample_unseen_hard and mfsgd_sample_unseen_violating too, which stage their rows and picks alone
constexpr int64_t kSampleChunk = (int64_t)1 << 22;

// d_sync: done[B] words (kDoneStride apart), then {arrivals, generation, -, -} of the kernel's start-of-launch
// barrier, then {abort code, launches that started, -, -}.  Zeroed once, when allocated; the kernel keeps it
// consistent from launch to launch by itself.
// Behind them the tile mailboxes of the persistent kernel: B x kp granules of 8 bytes ({value, tag}; only tiles the
// scheduler marked kCellLoneTile use theirs).
inline size_t sync_bytes(const Part& p) {
    return ((size_t)p.sched.B * kDoneStride + 8) * sizeof(unsigned) + (size_t)p.sched.B * (size_t)p.sched.geo.L * 4 * 8;
}
inline unsigned* abort_word(const Part& p) { return p.d_sync.data() + (size_t)p.sched.B * kDoneStride + 4; }

}  // namespace mfsgd

struct mfsgd_handle {
    mfsgd_config cfg{};
    mfsgd::Geometry geo{};
    int n_parts = 1;
    std::vector<mfsgd::Part> parts;
    bool have_ratings = false;
    int64_t nnz_total = 0;
    // DSGD item map (n_parts > 1): item i lives in partition item_part[i], row item_row[i] of that
    // partition's Q block.  Default: i % n_parts, i / n_parts; mfsgd_set_item_partition replaces it.
    std::vector<int32_t> item_part, item_row, part_q_rows;
    bool custom_item_map = false;

    // factors: host staging (kp-padded rows) until the device copy is created
    enum class Where { None, Host, Device } where = Where::None;
    std::vector<float> hP, hQ;
    mfsgd::DevArray<float> dP, dQ;
    // The handle holds a Q of its own: single-partition handles after mfsgd_init_factors, mfsgd_set_factors or
    // mfsgd_load_factors.  Not after mfsgd_init_p_offset, which seeds P alone (check_has_q).
    bool have_q = false;
    // Rows the caller reserved per side (mfsgd_reserve_rows; 0: none).  The device buffers hold user_capacity() /
    // item_capacity() rows of kp floats: the count, or the reserve where that is larger.  Rows from the count on are
    // written by an append before anything reads them.
    int32_t reserved_users = 0, reserved_items = 0;
    int32_t user_capacity() const { return cfg.n_users > reserved_users ? cfg.n_users : reserved_users; }
    int32_t item_capacity() const { return cfg.n_items > reserved_items ? cfg.n_items : reserved_items; }
    size_t p_bytes() const { return sizeof(float) * (size_t)cfg.n_users * (size_t)geo.kp; }  // the rows P has
    size_t q_bytes() const { return sizeof(float) * (size_t)cfg.n_items * (size_t)geo.kp; }

    mfsgd::Validation val;
    // Online updates (mfsgd_online_levels, mfsgd_apply_ratings): per user / per item, 1 + the level of the latest rating
    // of the piece being levelled that has it, 0 for none.  Host memory, allocated at the first such call; all zero
    // between calls (a piece resets the entries it touched).
    std::vector<int32_t> online_last_u, online_last_i;

    bool device_ready = false;
    int n_cu = 0;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;  // diagnostics only (mfsgd_debug_occupy)
    unsigned* occupy_started = nullptr; // ... pinned host word its workgroups count themselves in
    int64_t n_not_resident = 0;         // persistent launches that gave up at the residency check
    // identity of the rating set the schedules were built from: its length and a 128-bit hash of every
    // byte of u, i and r -- a repeated mfsgd_set_ratings with the same triples keeps the schedules
    uint64_t ratings_hash[2] = {0, 0};
    int64_t n_schedule_builds = 0, n_schedule_reuses = 0;
    // host seconds of the latest recommend call's two device halves, each up to its synchronise: building the candidate
    // and exclusion lists, then scoring and selecting (mfsgd_debug_serve_seconds)
    double serve_lists_s = 0.0, serve_topn_s = 0.0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    mutable std::string err;
    // what each user has already seen (mfsgd_set_seen, mfsgd_mark_seen): read by the _unseen serving calls
    mfsgd::Seen seen;
    // what the weighted draw draws in proportion to (mfsgd_set_item_weights): the items', not the index's
    mfsgd::ItemWeights weights;
};

namespace mfsgd {

// The message channel of the calls that have no handle (mfsgd_create, mfsgd_ranking_metrics_from_ranks): read with
// mfsgd_last_error(NULL), per thread.
extern thread_local std::string g_create_error;

int fail(const mfsgd_handle* h, int code, const std::string& msg);
int hip_fail(const mfsgd_handle* h, const std::string& what, hipError_t e);

#define HIPCHK(h, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return hip_fail((h), std::string(#call) + ": ", e_);              \
    } while (0)

// The serving calls name themselves instead of the HIP call that failed: `bad` makes the return code of an error ...
#define HIPCHK_OR(bad, call)                   \
    do {                                       \
        hipError_t e_ = (call);                \
        if (e_ != hipSuccess) return bad(e_);  \
    } while (0)

// ... and most of them leave no error behind in the runtime
int serve_fail(const mfsgd_handle* h, const char* prefix, hipError_t e);

// The guard (guard.hpp) with this error channel: every `int` entry point of these units runs its body in guarded()
// or, without a handle, in guarded_free().
// A null handle is MFSGD_ERR_INVALID_ARG.  std::bad_alloc becomes MFSGD_ERR_OOM, "<name>: out of host memory"; any other
// std::exception becomes `other`, "<name>: <what()>".
template <class F>
int guarded(const mfsgd_handle* h, const char* name, F&& body, int other = MFSGD_ERR_HIP) {
    if (!h) return MFSGD_ERR_INVALID_ARG;
    return guard_run(body, other, [&](int code, const char* what) { return fail(h, code, std::string(name) + ": " + what); });
}

// The same for a call without a handle: the message goes where mfsgd_create's go, or (name == nullptr) nowhere.
template <class F>
int guarded_free(const char* name, F&& body) {
    return guard_run(body, MFSGD_ERR_HIP, [&](int code, const char* what) {
        if (name) g_create_error = std::string(name) + ": " + what;
        return code;
    });
}

// MFSGD_OK, or MFSGD_ERR_INVALID_ARG with "<name>: bad partition".  (Not a Part*: h->parts is empty until
// mfsgd_set_ratings, and some callers ask before.)
int check_part(const mfsgd_handle* h, int32_t part, const char* name);

// What every call that reads the handle's own Q asks before it asks for a device: MFSGD_OK, or MFSGD_ERR_STATE with
// "<call>: Q is not initialised: ..." on a single-partition handle whose factors were seeded by mfsgd_init_p_offset
// (P alone).  Factors that were never initialised are the caller's own check, with the message it has always had.
int check_has_q(const mfsgd_handle* h, const char* call);
// What every call that reads the factors asks before it asks for a device, in this order: single-partition handles
// only, factors not initialised, then (unless the call reads P alone: reads_q == false) check_has_q.
int check_reads_factors(const mfsgd_handle* h, const char* call, bool reads_q = true);

// handle.cpp
int ensure_device(mfsgd_handle* h);
int dev_alloc(mfsgd_handle* h, DevBuf& b, size_t bytes);
int factors_to_device(mfsgd_handle* h);
// seen_index.cpp.  The tables of the seen-item index for a user capacity of new_cap, when it has tables and they are
// smaller: new ones (off2, slot2) filled on the handle's stream from the old, which stay as they are (the caller
// synchronises, then seen_adopt_tables).  Nothing to do leaves off2 empty.  `prefix` starts the message of a failure.
int seen_grown_tables(mfsgd_handle* h, const char* prefix, int32_t new_cap, DevArray<long long>& off2, DevArray<int32_t>& slot2);
void seen_adopt_tables(mfsgd_handle* h, int32_t new_cap, DevArray<long long>& off2, DevArray<int32_t>& slot2);
// ... and the bodies of mfsgd_set_seen (merge == false) / mfsgd_mark_seen, `name` being the call's, and of mfsgd_get_seen
int seen_update(mfsgd_handle* h, const char* name, bool merge, const int32_t* u, const int32_t* i, int64_t n);
int seen_get(mfsgd_handle* h, const int32_t* users, int32_t n_users, int64_t* row_ptr, int32_t* items, int64_t items_capacity);
// ... and of the item-weight calls and mfsgd_seen_item_counts (seen.hip)
int weights_set(mfsgd_handle* h, const uint32_t* w, int32_t n);
int weights_get(mfsgd_handle* h, uint32_t* w, int32_t* n);
int weights_clear(mfsgd_handle* h);
int seen_item_histogram(mfsgd_handle* h, int64_t* counts);
// sampling.cpp.  The bodies of mfsgd_sample_unseen and mfsgd_sample_unseen_weighted (the kernels are sample.hip's), of
// mfsgd_sample_unseen_hard and of mfsgd_sample_unseen_violating (pick.hip's)
int seen_sample(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first, int32_t* out_items);
int seen_sample_weighted(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                         int32_t* out_items, int64_t* out_mass);
int seen_sample_hard(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first, int32_t* out_items,
                     float* out_scores, int32_t* out_draw);
int seen_sample_violating(mfsgd_handle* h, const int32_t* users, const int32_t* pos_items, int64_t n, int32_t m, float margin,
                          int64_t seed, int64_t first, int32_t* out_items, int32_t* out_draw, float* out_margin, int32_t* out_rank);
// ... and of mfsgd_sample_unseen_hard_weighted and mfsgd_sample_unseen_violating_weighted: the same kernels under the
// weighted draw
int seen_sample_hard_weighted(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                              int32_t* out_items, float* out_scores, int32_t* out_draw, int64_t* out_mass);
int seen_sample_violating_weighted(mfsgd_handle* h, const int32_t* users, const int32_t* pos_items, int64_t n, int32_t m,
                                   float margin, int64_t seed, int64_t first, int32_t* out_items, int32_t* out_draw,
                                   float* out_margin, int32_t* out_rank, int64_t* out_mass);
// ratings.cpp
void default_item_map(mfsgd_handle* h);
int prepare_compute(mfsgd_handle* h);  // ratings present; factors and every partition's schedule on the device

// The typed forms: n elements, and a whole vector (std::vector or PodVec) of them.
template <class T>
int dev_alloc(mfsgd_handle* h, DevArray<T>& a, size_t n) {
    const hipError_t e = a.alloc(n);
    if (e != hipSuccess) return hip_fail(h, "hipMalloc(&b.p, bytes): ", e);  // (the text this failure has always had)
    return MFSGD_OK;
}
template <class T, class V>
int upload(mfsgd_handle* h, DevArray<T>& a, const V& v) {
    static_assert(std::is_same_v<std::remove_cv_t<std::remove_reference_t<decltype(*v.data())>>, T>, "element type");
    int rc = dev_alloc(h, a, v.size());
    if (rc) return rc;
    if (!v.empty()) HIPCHK(h, hipMemcpy(a.data(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return MFSGD_OK;
}

// n elements of the host's into / out of a typed array, from its element `at` on, asynchronously on st.  U is T, or the
// other name of the same integer (int64_t and long long); more than the array was allocated for is refused.
template <class T, class U>
constexpr bool kSameElement = std::is_same_v<T, U> || (std::is_integral_v<T> && std::is_integral_v<U> && sizeof(T) == sizeof(U) &&
                                                       std::is_signed_v<T> == std::is_signed_v<U>);
template <class T, class U>
hipError_t copy_up(const DevArray<T>& a, const U* src, size_t n, hipStream_t st, size_t at = 0) {
    static_assert(kSameElement<T, U>, "element type");
    if (at + n > a.size()) return hipErrorInvalidValue;
    return hipMemcpyAsync(a.data() + at, src, n * sizeof(T), hipMemcpyHostToDevice, st);
}
template <class T, class U>
hipError_t copy_down(U* dst, const DevArray<T>& a, size_t n, hipStream_t st, size_t at = 0) {
    static_assert(kSameElement<T, U>, "element type");
    if (at + n > a.size()) return hipErrorInvalidValue;
    return hipMemcpyAsync(dst, a.data() + at, n * sizeof(T), hipMemcpyDeviceToHost, st);
}

}  // namespace mfsgd
