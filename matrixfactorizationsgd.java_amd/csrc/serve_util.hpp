// serve_util.hpp -- host-side steps the serving calls share: range checks of index lists, a slot per distinct row, and
// batches of whole rows under a cap.  The standard library only: tests/test_serve_util_cpu.py builds it into a program.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace mfsgd {

// The first x < n for which outside(x) is not 0, or -1.  In blocks of 4096 without a branch, so that the compiler
// vectorises the pass that finds nothing (these lists are the most the host reads).
template <class Outside>
int64_t first_where(int64_t n, Outside outside) {
    for (int64_t x0 = 0; x0 < n; x0 += 4096) {
        const int64_t x1 = std::min(n, x0 + 4096);
        uint32_t any = 0;
        for (int64_t x = x0; x < x1; ++x) any |= outside(x);
        for (int64_t x = x0; any && x < x1; ++x)
            if (outside(x)) return x;
    }
    return -1;
}

// The index of the first of the n values outside [0, bound), or -1 ...
inline int64_t first_outside(const int32_t* v, int64_t n, int32_t bound) {
    const uint32_t B = (uint32_t)bound;
    return first_where(n, [v, B](int64_t x) { return (uint32_t)((uint32_t)v[x] >= B); });
}
// ... and of the first pair (a[x], b[x]) either half of which is outside its own bound.
inline int64_t first_outside(const int32_t* a, int32_t bound_a, const int32_t* b, int32_t bound_b, int64_t n) {
    const uint32_t A = (uint32_t)bound_a, B = (uint32_t)bound_b;
    return first_where(n, [a, b, A, B](int64_t x) { return (uint32_t)((uint32_t)a[x] >= A) | (uint32_t)((uint32_t)b[x] >= B); });
}

// A slot per distinct row among the n asked for (each below n_rows), in the order of first mention: a row asked for
// twice shares its slot.  slot_of_row is -1 where unasked; count[s] (with_counts): how often the row of slot s was asked for.
struct Slots {
    std::vector<int32_t> slot_of_row, row_of_slot;
    std::vector<long long> count;
    int32_t n() const { return (int32_t)row_of_slot.size(); }
};
inline Slots slots_of(const int32_t* rows, int64_t n, int32_t n_rows, bool with_counts = false) {
    Slots s;
    s.slot_of_row.assign((size_t)n_rows, -1);
    for (int64_t x = 0; x < n; ++x) {
        int32_t& slot = s.slot_of_row[(size_t)rows[x]];
        if (slot < 0) {
            slot = s.n();
            s.row_of_slot.push_back(rows[x]);
            if (with_counts) s.count.push_back(0);
        }
        if (with_counts) ++s.count[(size_t)slot];
    }
    return s;
}

// Rows 0 .. n - 1 in batches of whole rows: batch c is rows cut[c] .. cut[c + 1] - 1.  A batch always takes its first
// row (one over the cap is a batch of its own), then further rows while it has fewer than cap_rows and the weights add
// up to cap_weight at most.  max_rows / max_weight: the largest batch, which sizes the staging.
struct Batches {
    std::vector<int32_t> cut{0};
    int64_t max_rows = 0, max_weight = 0;
    size_t count() const { return cut.size() - 1; }
};
template <class Weight>
Batches cut_batches(int32_t n, Weight weight, int64_t cap_weight, int64_t cap_rows) {
    Batches b;
    for (int32_t r0 = 0; r0 < n;) {
        int32_t r1 = r0 + 1;
        int64_t w = weight(r0);
        while (r1 < n && r1 - r0 < cap_rows && (int64_t)weight(r1) <= cap_weight - w) w += weight(r1++);
        b.cut.push_back(r1);
        b.max_rows = std::max<int64_t>(b.max_rows, r1 - r0);
        b.max_weight = std::max(b.max_weight, w);
        r0 = r1;
    }
    return b;
}

}  // namespace mfsgd
