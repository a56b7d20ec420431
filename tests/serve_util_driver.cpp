// The host helpers of csrc/serve_util.hpp in a program of their own (tests/test_serve_util_cpu.py builds and runs it
// under AddressSanitizer and UBSan): cut_batches against a brute-force loop, first_outside around its 4096-blocks, and
// slots_of with repeated and unrequested rows.  Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <cstdlib>

#include "serve_util.hpp"

using namespace mfsgd;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

// The batching as the serving cores wrote it out before they shared it: a batch takes rows while it has fewer than
// cap_rows and, but for its first row, while the weights stay within cap_weight.
struct Brute {
    std::vector<int32_t> cut{0};
    int64_t max_rows = 0, max_weight = 0;
};
static Brute brute(const std::vector<int64_t>& w, int64_t cap_weight, int64_t cap_rows) {
    Brute out;
    const int32_t n = (int32_t)w.size();
    for (int32_t b0 = 0; b0 < n;) {
        int32_t b1 = b0;
        int64_t sum = 0;
        while (b1 < n && b1 - b0 < cap_rows && (b1 == b0 || sum + w[(size_t)b1] <= cap_weight)) sum += w[(size_t)b1++];
        out.cut.push_back(b1);
        out.max_rows = std::max<int64_t>(out.max_rows, b1 - b0);
        out.max_weight = std::max(out.max_weight, sum);
        b0 = b1;
    }
    return out;
}

static Batches check_cut(const std::vector<int64_t>& w, int64_t cap_weight, int64_t cap_rows) {
    const Batches got = cut_batches((int32_t)w.size(), [&w](int32_t r) { return w[(size_t)r]; }, cap_weight, cap_rows);
    const Brute want = brute(w, cap_weight, cap_rows);
    CHECK(got.cut == want.cut);
    CHECK(got.max_rows == want.max_rows && got.max_weight == want.max_weight);
    CHECK(got.count() + 1 == got.cut.size() && got.cut.back() == (int32_t)w.size());
    return got;
}

static void test_cut_batches() {
    const int64_t cap = (int64_t)64 << 20;
    CHECK((check_cut({cap, 1}, cap, 65535).cut == std::vector<int32_t>{0, 1, 2}));
    const Batches over = check_cut({cap + 1}, cap, 65535);  // one row over the cap is a batch of its own
    CHECK((over.cut == std::vector<int32_t>{0, 1}) && over.max_weight == cap + 1);
    CHECK((check_cut({1, cap + 1, 1}, cap, 65535).cut == std::vector<int32_t>{0, 1, 2, 3}));
    const Batches rows = check_cut(std::vector<int64_t>(65536, 0), cap, 65535);  // cap_rows + 1 rows of weight 0
    CHECK((rows.cut == std::vector<int32_t>{0, 65535, 65536}) && rows.max_rows == 65535 && rows.max_weight == 0);
    const Batches none = check_cut({}, cap, 65535);
    CHECK(none.count() == 0 && none.max_rows == 0 && none.max_weight == 0);
    CHECK(check_cut({5, 5, 5}, INT64_MAX, 2).cut == (std::vector<int32_t>{0, 2, 3}));  // (the weight cap off: fused)
    uint64_t lcg = 12345;
    auto next = [&lcg](uint64_t m) { return (int64_t)(((lcg = lcg * 6364136223846793005ull + 1442695040888963407ull) >> 33) % m); };
    for (int trial = 0; trial < 300; ++trial) {
        std::vector<int64_t> w((size_t)next(40));
        for (int64_t& x : w) x = next(4) == 0 ? 0 : next(30);
        check_cut(w, 1 + next(40), 1 + next(6));
    }
}

static void test_first_outside() {
    const int64_t n = 8193;
    const int32_t bound = 10;
    std::vector<int32_t> v((size_t)n), other((size_t)n, 0);
    for (int64_t x = 0; x < n; ++x) v[(size_t)x] = (int32_t)(x % bound);
    CHECK(first_outside(v.data(), n, bound) == -1);
    CHECK(first_outside(v.data(), 0, bound) == -1 && first_outside(nullptr, 0, bound) == -1);
    for (const int64_t at : {(int64_t)0, (int64_t)4095, (int64_t)4096, n - 1}) {
        for (const int32_t bad : {bound, -1, INT32_MIN, INT32_MAX}) {  // (negative values are outside)
            std::vector<int32_t> w = v;
            w[(size_t)at] = bad;
            CHECK(first_outside(w.data(), n, bound) == at);
            CHECK(first_outside(w.data(), bound, other.data(), 1, n) == at);
            CHECK(first_outside(other.data(), 1, w.data(), bound, n) == at);
            if (at + 1 < n) {  // the first one counts, in whichever array it is
                std::vector<int32_t> o = other;
                o[(size_t)at + 1] = 1;
                w[(size_t)n - 1] = bad;
                CHECK(first_outside(w.data(), n, bound) == at);
                CHECK(first_outside(w.data(), bound, o.data(), 1, n) == at);
                w[(size_t)at] = 0;
                CHECK(first_outside(w.data(), bound, o.data(), 1, n) == at + 1);
            }
        }
    }
    CHECK(first_outside(v.data(), n, bound - 1) == bound - 1);  // the bound itself is outside
    CHECK(first_outside(v.data(), n, 0) == 0);
}

static void test_slots() {
    const std::vector<int32_t> rows{3, 1, 3, 0, 1, 3};
    const Slots s = slots_of(rows.data(), (int64_t)rows.size(), 5, true);
    CHECK((s.slot_of_row == std::vector<int32_t>{2, 1, -1, 0, -1}));
    CHECK((s.row_of_slot == std::vector<int32_t>{3, 1, 0}) && s.n() == 3);
    CHECK((s.count == std::vector<long long>{3, 2, 1}));
    const Slots plain = slots_of(rows.data(), (int64_t)rows.size(), 5);
    CHECK(plain.slot_of_row == s.slot_of_row && plain.row_of_slot == s.row_of_slot && plain.count.empty());
    const Slots none = slots_of(nullptr, 0, 3, true);
    CHECK((none.slot_of_row == std::vector<int32_t>{-1, -1, -1}) && none.n() == 0 && none.count.empty());
}

int main() {
    test_cut_batches();
    test_first_outside();
    test_slots();
    std::printf("ok\n");
    return 0;
}
