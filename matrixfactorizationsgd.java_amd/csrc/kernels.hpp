// kernels.hpp -- host-callable launchers of every kernel unit: epoch.hip, cells.hip, kernels.hip, foldin.hip,
// foldin_pairwise.hip, online.hip, pairwise.hip, rehyper.hip, recommend.hip, rank.hip, seen.hip, audience.hip, sample.hip, pick.hip,
// similar.hip, solve.hip, validate.hip and grow.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "devmem.hpp"
#include "schedule.hpp"

namespace mfsgd {

struct CellLaunch {
    float* P;
    float* Q;
    const CellDesc* cells;
    const uint32_t* rows;
    const SubDesc* subs;
    const Entry* entries;
    int B;
    int rd;          // round (training only)
    int grid;        // workgroups: B for a training round, B*B for an SSE pass
    int lds_bytes;   // dynamic LDS per workgroup
    int sched_cap;   // bytes of one of its two schedule buffers
    float lr;
    float c;         // 1 - lr*lambda
    double* sse_partial;
    bool diag = false;  // diagnostic launch: in-kernel cycle stamps are written to sse_partial (as u64 words)
};

// cells.hip.  One training round (train = true) or the SSE pass over every cell.
hipError_t launch_cell(bool train, int L, int W, const CellLaunch& a, hipStream_t st);
// epoch.hip.  Persistent epoch kernel: a.grid workgroups (all must be co-resident: at most
// blocks_per_cu x CUs) run n_rounds rounds; `done` holds B words spaced kDoneStride
// apart (the kernel resets its own flags at the start of every launch: the caller zeroes
// nothing between launches), `abort_word` one word.
constexpr int kDoneStride = 32;
hipError_t epoch_blocks_per_cu(int L, int W, const CellLaunch& a, int* blocks_per_cu);
hipError_t launch_epoch_persistent(int L, int W, const CellLaunch& a, int n_rounds, unsigned* done,
                                   unsigned* abort_word, hipStream_t st);
// SSE pass, persistent form: a.grid workgroups walk n_cells cells; a.sse_partial gets a.grid doubles.
hipError_t launch_sse_persistent(int L, int W, const CellLaunch& a, int n_cells, hipStream_t st);
hipError_t launch_reduce_sse(const double* partial, int64_t n, double* out, hipStream_t st);
hipError_t launch_predict(int L, const float* P, const float* Q, const int32_t* u, const int32_t* i,
                          float* out, int64_t n, hipStream_t st);

// foldin.hip.  Fold-in of the nb new rows of one batch against the fixed side's factors F (kp-padded rows: Q for new
// users, P for new items -- the update is symmetric in its two rows): group g takes new row x = perm[g], whose ratings
// are entries row_ptr[x] - base .. row_ptr[x + 1] - base of ids / ratings (row_ptr: nb + 1 words; ids name rows of F),
// and runs `epochs` passes of its half of the canonical update over them, in the order given.
// rows: nb x k dense, the start rows on entry and the folded rows on return.  perm is best sorted by length, longest
// first (a wave runs as long as its longest list); the result does not depend on it.  The batch holds at least one
// rating, and every id is a row of F: the caller checks.
hipError_t launch_fold_in(int L, const float* F, float* rows, int k, const long long* row_ptr, long long base,
                          const int32_t* perm, int nb, const int32_t* ids, const float* ratings, int epochs, float lr,
                          float c, hipStream_t st);

// foldin_pairwise.hip.  Pairwise fold-in of the nb new users of one batch against Q (include/mfsgd.h,
// mfsgd_fold_in_users_pairwise): group g takes new user x = perm[g], whose positives are entries ptr[x] .. ptr[x + 1] of
// ids (ptr: nb + 1 words counting from the batch's first positive, which is positive `base` of the call) and whose
// sorted distinct list is s_items[s_off[x] .. s_off[x + 1]) (recommend_excl_lists' output for the keys x << 32 | id),
// and runs `epochs` passes of the rule over them: step tau of the user draws its m candidates at the counters
// first + ((base + ptr[x]) * epochs + tau) * m + d.  rows: nb x k dense, the start rows on entry and the folded rows on
// return.  out_margin / out_neg (either nullable): entry ptr[x] * epochs + tau receives step tau's margin and negative;
// 0x7FC00000 and -1 throughout for a user whose list names every item.  perm is best sorted by length, longest first;
// the result does not depend on it.  The batch holds at least one positive, every id is a row of Q and m >= 1: the
// caller checks.  Asynchronous on st.
struct PairwiseFold {
    const float* Q;
    float* rows;
    int k;
    const long long* ptr;
    long long base;
    const int32_t* perm;
    int nb;
    const int32_t* ids;
    const long long* s_off;
    const int32_t* s_items;
    int n_items, epochs, m;
    float lr, c;  // c = 1 - lr * lambda
    unsigned long long seed, first;
    float* out_margin;
    int32_t* out_neg;
    // mfsgd_fold_in_users_pairwise_weighted: the draws are sample_weighted_draws' for the lists {s_off, s_items}, s_mass
    // their unseen-mass table (seen_unseen_mass over the batch's distinct pairs) and C the prefix of exactly n_items
    // weights; a user whose unseen weight is 0 takes no step (0x7FC00000 and -1), the rest is as above.  C == nullptr:
    // the uniform draw.
    const unsigned long long* s_mass = nullptr;
    const unsigned long long* C = nullptr;
};
hipError_t launch_fold_in_pairwise(int L, const PairwiseFold& a, hipStream_t st);

// online.hip.  Levels l0 .. l1 - 1 of one piece of an online update against the live P and Q (kp-padded rows): level l is
// the ratings level_ptr[l] .. level_ptr[l + 1] - 1 of u / i / r, which share no user and no item; each gets the whole
// canonical update, and err[orig[j]] (err nullable) the error before it.  One level may be given to any number of
// workgroups; several levels (their order is the barrier between them) go to ONE workgroup, which walks them -- anything
// else is hipErrorInvalidValue.  Every user is a row of P, every item a row of Q, and every orig an entry of err: the
// caller checks.  Asynchronous on st.
hipError_t launch_apply_levels(int L, float* P, float* Q, const int32_t* u, const int32_t* i, const float* r,
                               const int32_t* orig, const int32_t* level_ptr, int l0, int l1, int workgroups, int k,
                               float lr, float c, float* err, hipStream_t st);

// pairwise.hip.  The same for the triples (u, i, jn) of a pairwise update ("Pairwise ranking (BPR)"): the
// triples of a level share no row of P and no row of Q in either item position, and i[t] != jn[t]; each gets the
// three-row update of section 3, and margin[orig[t]] (margin nullable) the margin x before it.  Levels, workgroups,
// what the caller checks and the stream are launch_apply_levels'.  w (nullable; one weight per triple, in the order of
// u, and no NaN but 0x7FC00000): the step size of triple t is lr * w[t] in place of lr * lsig(x), the rest alike.
hipError_t launch_apply_triple_levels(int L, float* P, float* Q, const int32_t* u, const int32_t* i, const int32_t* jn,
                                      const float* w, const int32_t* orig, const int32_t* level_ptr, int l0, int l1,
                                      int workgroups, int k, float lr, float c, float* margin, hipStream_t st);

// rehyper.hip.  Re-bakes lr and c = 1 - lr*lambda into the entries of a schedule on the device, in place: afterwards
// they are byte for byte what the packers write for those values (schedule.cpp, rehyper_schedule, is the host's form).
// cells / subs: the n_descs chunk descriptors and their W*W sub-cell records each; entries: n_entries records.
// Asynchronous on st; allocates nothing.
hipError_t launch_rehyper(const CellDesc* cells, const SubDesc* subs, Entry* entries, int64_t n_descs, int64_t n_entries,
                          int W, int G, float lr, float c, hipStream_t st);

// rows x kp floats: java.util.Random(seed) draws first_pos + row * k ... scaled, zero padded (device-side seeding).
hipError_t launch_init_rows(float* dst, long long rows, int k, int kp, long long seed, unsigned long long first_pos, float scale,
                            hipStream_t st);

// grow.hip.  dst[x * kp + f] = canon_nan(src[x * k + f]) for f < k and 0.0f for k <= f < kp, x = 0 .. rows - 1: dense
// rows of the caller's (src: device memory) into kp-padded rows of the live factors (dst: 16-byte aligned, as every row
// of a kp-strided matrix is).  16-byte stores throughout; 16-byte loads where k is a multiple of 4 and src is aligned.
// Asynchronous on st.
hipError_t launch_place_rows(float* dst, const float* src, long long rows, int k, int kp, hipStream_t st);

// Diagnostic (tests): `workgroups` one-wave workgroups, each holding lds_bytes of LDS, spin for `ticks` x 10 ns.
// `started` (device-accessible host memory, or null): every workgroup adds one to it as it starts
hipError_t launch_occupy(int workgroups, int lds_bytes, unsigned long long ticks, unsigned* started, hipStream_t st);

// recommend.hip.  Exclusions of one recommend call: the slot of each requested user (slot_of_user[n_users], -1 for the
// rest) and, per slot s, the sorted distinct excluded items items[off[s] .. off[s + 1]).  slot == nullptr: none.
struct RecommendExcl {
    const int32_t* slot = nullptr;
    const long long* off = nullptr;
    const int32_t* items = nullptr;
};
// What is scored: ra == nullptr, dot(P[u], Q[j]) (recommend); otherwise the cosine (dot * ra[u]) * rb[j] of DESIGN.md
// section 3, ra / rb being the inverse norms of the rows of P / Q (similar.hip).  Selection, ties, exclusions and
// padding are the same code for both.
struct CosineScale {
    const float* ra = nullptr;
    const float* rb = nullptr;
};
// Top-N among candidates (mfsgd_recommend_among): request row b of a batch scores the sorted, distinct items
// items[off[r] .. off[r + 1]) only, r = b (per_row == 1: a list per request row, off pointing at the batch's first
// row) or 0 (per_row == 0: one list for every row).  The kernels are the same with the list in the place of "every
// item"; the score is the dot.
struct RecommendAmong {
    const long long* off = nullptr;
    const int32_t* items = nullptr;
    int per_row = 0;
};
// One batch of a top-N call: for each of the nb rows d_users[...] of P (device memory, kp-padded rows) the topn rows of
// Q with the largest score, into out_s / out_i (nb x topn).  among == nullptr: every one of the n_items rows of Q is
// scored; otherwise the lists (the dot only).  `longest` is the most one row scores, `total` what all rows score.
struct TopnJob {
    int L = 0, nb = 0;
    const float *P = nullptr, *Q = nullptr;
    const int32_t* d_users = nullptr;
    int32_t n_items = 0, topn = 0;
    RecommendExcl ex;
    CosineScale cs;
    const RecommendAmong* among = nullptr;
    int64_t total = 0, longest = 0;
    float* out_s = nullptr;
    int32_t* out_i = nullptr;
};
// The sort path's buffers, the caller's (one set serves all batches): `total` scores or keys and ids in and out, nb + 1
// offsets, and the sorts' scratch, grown when it is too small.
struct TopnScratch {
    float *s_in, *s_out;
    int32_t *id_in, *id_out;
    long long* d_off;
    DevBuf* temp;
};
// Fused score + select (one workgroup per row, nothing but the winners goes to memory) for the (longest row, topn)
// recommend_is_fused() accepts: recommend_topn without scratch.  With scratch it is the sort path, for the rest.
bool recommend_is_fused(int64_t longest, int32_t topn);
hipError_t recommend_topn(const TopnJob& job, const TopnScratch* scratch, hipStream_t st);
// Building the candidate lists: keys[x0 + x] = row << 32 | items[x] for a chunk of n candidates that starts at position
// x0 of the call's, row being the request row whose range of ptr (n_rows + 1 entries, CSR; nullptr: row 0) holds the
// position.  recommend_excl_lists below then makes the lists of them, n_slots being the request rows (or 1).
hipError_t recommend_cand_keys(const long long* ptr, int32_t n_rows, const int32_t* items, int64_t x0, int64_t n,
                               unsigned long long* keys, hipStream_t st);
// Building the lists: each chunk of pairs appends slot << 32 | item to keys[*count ...] for the pairs of requested users
// (count starts at 0; at most cap are written) ...
hipError_t recommend_excl_filter(const int32_t* slot_of_user, const int32_t* u, const int32_t* i, int64_t n,
                                 unsigned long long* keys, unsigned long long* count, int64_t cap, hipStream_t st);
// ... then the n keys are sorted (through keys_tmp) and made distinct, back into keys: *n_distinct of them,
// off[n_slots + 1] and items[n] as RecommendExcl reads them.
hipError_t recommend_excl_lists(unsigned long long* keys, unsigned long long* keys_tmp, int64_t n, int32_t n_slots,
                                unsigned* n_distinct, long long* off, int32_t* items, DevBuf& temp, hipStream_t st);

// rank.hip.  Ranks of held-out items: slot s (of n_slots) is row rows[s] of P (kp-padded rows), its pairs are
// items[off[s] - base .. off[s + 1] - base), and out[...] at the same places receives, per pair, the number of items
// that come before it in that row's recommendation order (recommend.hip's), the items of the slot's exclusion list
// left out (ex.off / ex.items indexed by the same slots; ex.off == nullptr: none; ex.slot is not read).  Every item is
// a row of Q and every off[s] - base .. off[s + 1] - base lies inside items and out: the caller checks.
// ex_by_user: the lists are those of the seen-item index instead, reached through the slot's user: ex.off[rows[s]].
hipError_t launch_rank_items(int L, const float* P, const float* Q, const int32_t* rows, int n_slots, const long long* off,
                             long long base, const int32_t* items, int32_t n_items, const RecommendExcl& ex,
                             int32_t* out, hipStream_t st, bool ex_by_user = false);

// seen.hip.  The seen-item index (handle.hpp, Seen): off (capacity + 1 entries, those from the user count on holding the
// total), items, and the identity slot table that makes {slot, off, items} a RecommendExcl over user ids.
// keys[x] = u[x] << 32 | i[x] for a chunk of pairs; recommend_excl_lists then makes a whole index of the keys.
hipError_t seen_pair_keys(const int32_t* u, const int32_t* i, int64_t n, unsigned long long* keys, hipStream_t st);
// The tables of a capacity: slot[x] = x for x < new_cap and, with off2 != nullptr, off2[x] = old_off[x] for x <= old_cap
// and `total` for old_cap < x <= new_cap.
hipError_t seen_tables(const long long* old_off, int32_t old_cap, int64_t total, int32_t new_cap, long long* off2, int32_t* slot,
                       hipStream_t st);
// The m keys of a batch sorted and made distinct (keys, through keys_tmp), and those the index {off, items} does not
// hold, ascending, into keys_tmp: counts[0] distinct keys, counts[1] of them new.  flags: m bytes of scratch.
hipError_t seen_batch_fresh(unsigned long long* keys, unsigned long long* keys_tmp, int64_t m, int32_t n_users,
                            const long long* off, const int32_t* items, unsigned char* flags, unsigned* counts, DevBuf& temp,
                            hipStream_t st);
// The index {off, items} (`total` items, cap + 1 offsets) merged with n_fresh sorted distinct keys none of which it
// holds, into off2 (cap + 1) and items2 (total + n_fresh).  Every user of a key is below cap: the caller checks.
hipError_t seen_merge(const long long* off, const int32_t* items, int64_t total, int32_t cap, const unsigned long long* fresh,
                      int64_t n_fresh, long long* off2, int32_t* items2, hipStream_t st);
// len[b] = the length of the list of users[b]; out[row_ptr[b] ...] = that list (longest: the largest len).
hipError_t seen_lengths(const long long* off, const int32_t* users, int32_t n, long long* len, hipStream_t st);
hipError_t seen_gather(const long long* off, const int32_t* items, const int32_t* users, int32_t n, const long long* row_ptr,
                       int64_t longest, int32_t* out, hipStream_t st);

// The unseen-mass table of the index {off, items} (`total` > 0 pairs, cap + 1 offsets) under item weights given by their
// exclusive prefix C (n_w + 1 entries; items from n_w on weigh nothing): mass[x] = the weight of the items below items[x]
// that the list of x's user does not hold.  G: `total` entries of scratch (the scan of the pairs' weights).
hipError_t seen_unseen_mass(const long long* off, const int32_t* items, int64_t total, int32_t cap, const unsigned long long* C,
                            int32_t n_w, unsigned long long* G, unsigned long long* mass, DevBuf& temp, hipStream_t st);
// counts[i] += the number of lists that hold item i (counts: one zeroed entry per item of the model).
hipError_t seen_item_counts(const int32_t* items, int64_t total, unsigned long long* counts, hipStream_t st);

// audience.hip.  The index {off, items} (`total` pairs; off[0 .. n_users] is read) by item: for every pair whose item has
// a slot (slot_of_item[n_items], -1 for the rest) the key slot << 32 | user is appended to keys[*count ...], in no
// particular order (count starts at 0; at most cap are written).  keys == nullptr: *count receives their number alone.
// recommend_excl_lists then makes the lists of them, one ascending user list per slot.
hipError_t seen_audience_keys(const int32_t* slot_of_item, int32_t n_items, const long long* off, const int32_t* items,
                              int32_t n_users, int64_t total, unsigned long long* keys, unsigned long long* count, int64_t cap,
                              hipStream_t st);

// sample.hip.  Uniform draws among the items a user has not seen (include/mfsgd.h, mfsgd_sample_unseen): out[x], x <
// n_draws, is draw x % m of row x / m of `users` (every one a user of the index {off, items}; off == nullptr: an index
// without pairs) with the counter first + x, among n_items items; -1 where the user has seen them all.  n_draws < 2^31.
hipError_t sample_unseen_draws(const long long* off, const int32_t* items, const int32_t* users, int64_t n_draws, int32_t m,
                               int32_t n_items, int64_t seed, uint64_t first, int32_t* out, hipStream_t st);

// The same in proportion to the items' weights (mfsgd_sample_unseen_weighted): mass is the index's unseen-mass table
// (seen_unseen_mass), C the prefix of exactly n_items weights; -1 where every item of positive weight is seen.
// row_mass[x / m] (nullable) receives the unseen weight of the row's user.
hipError_t sample_weighted_draws(const long long* off, const int32_t* items, const unsigned long long* mass,
                                 const unsigned long long* C, const int32_t* users, int64_t n_draws, int32_t m, int32_t n_items,
                                 int64_t seed, uint64_t first, int32_t* out, long long* row_mass, hipStream_t st);

// pick.hip.  The weighted draw of a pick launch (mfsgd_sample_unseen_hard_weighted, mfsgd_sample_unseen_violating_weighted):
// mass is the index's unseen-mass table (seen_unseen_mass; not read where off == nullptr), C the prefix of exactly
// n_items weights, out_mass (nullable) receives each row's unseen weight.  C == nullptr: the uniform draw, the launch
// as it is described below.  With weights the candidates are those sample_weighted_draws gives the row, a row has
// nothing to draw where its user's unseen WEIGHT is 0, and everything else -- scores, rules, outputs, the unseen item
// count in the rank -- is unchanged.
struct PickWeights {
    const unsigned long long* mass = nullptr;
    const unsigned long long* C = nullptr;
    long long* out_mass = nullptr;
};

// pick.hip.  Hard negatives (include/mfsgd.h, mfsgd_sample_unseen_hard): for each of the n rows of `users` (every one a
// user of the index {off, items} and a row of P; off == nullptr: an index without pairs) the best-scoring of the m >= 1
// candidates sample_unseen_draws gives that row for the same (m, n_items, seed, first), the score being dot(P[user],
// Q[candidate]) (kp-padded rows; the bits launch_predict returns) and the pick the header's rule: out_items[x] the item,
// out_scores[x] its score and out_draw[x] its d (either nullable); -1, 0x7FC00000 and -1 where the user has seen every
// item.  n <= 2^22 (a piece).  Asynchronous on st.
hipError_t launch_hard_negatives(int L, const float* P, const float* Q, const long long* off, const int32_t* items,
                                 const int32_t* users, int64_t n, int32_t m, int32_t n_items, int64_t seed, uint64_t first,
                                 int32_t* out_items, float* out_scores, int32_t* out_draw, hipStream_t st,
                                 const PickWeights& w = {});

// pick.hip.  The negative of a WARP step (include/mfsgd.h, mfsgd_sample_unseen_violating): rows, index, candidates and
// dots as for launch_hard_negatives, pos[x] (a row of Q) the row's positive.  Of the row's m >= 1 candidates the first in
// d with candidate != pos[x] and dot(P[user], Q[pos]) - dot(P[user], Q[candidate]) < margin: out_items[x] the item,
// out_draw[x] its d, out_margin[x] that difference and out_rank[x] = max(1, unseen items / (d + 1)) (the last three
// nullable); -1, m, 0x7FC00000 and 0 where no candidate does, -1, -1, 0x7FC00000 and 0 where the user has seen every
// item.  n <= 2^22 (a piece).  Asynchronous on st.
hipError_t launch_first_violating(int L, const float* P, const float* Q, const long long* off, const int32_t* items,
                                  const int32_t* users, const int32_t* pos, int64_t n, int32_t m, float margin, int32_t n_items,
                                  int64_t seed, uint64_t first, int32_t* out_items, int32_t* out_draw, float* out_margin,
                                  int32_t* out_rank, hipStream_t st, const PickWeights& w = {});

// similar.hip.  out[x] = rn(row x) = 1 / sqrt(dot(row, row)), or 0 where that dot is 0, for the
// n_rows kp-padded rows of M.  Asynchronous on st.
hipError_t launch_row_inv_norms(int L, const float* M, int64_t n_rows, float* out, hipStream_t st);

// solve.hip.  The Gram matrix of the n >= 1 kp-padded rows of F (include/mfsgd.h, "least-squares fold-in"): tile t of
// gram_tile_rows(n) rows is one chain into partial[t] (room for gram_tiles(n) x k x k floats), and G (k x k, symmetric)
// is the partials added in tile order.  Asynchronous on st.
int64_t gram_tile_rows(int64_t n);
int64_t gram_tiles(int64_t n);
hipError_t launch_gram(int L, const float* F, int64_t n, int k, float* partial, float* G, hipStream_t st);
// The nb new rows of one batch by least squares against the fixed side F: workgroup g takes new row x = perm[g], whose
// list is entries ptr[x] - base .. ptr[x + 1] - base of ids / a / b (a nullable: all 1), builds the system of the
// rule -- alpha * G on top where alpha != 0 (G is not read otherwise), ridge_per_entry * len + ridge on the diagonal --
// and solves it by Cholesky.  rows (nb x k dense) gets the solution, zeros for an empty list, 0x7FC00000 where a pivot
// is not positive; status[x] (nullable) 0 or the 1-based pivot.  A list is one chain: it is not split across
// workgroups.  Every id is a row of F: the caller checks.  Asynchronous on st.
struct SolveRows {
    const float* F;
    float* rows;
    int k;
    const long long* ptr;
    long long base;
    const int32_t* perm;
    int nb;
    const int32_t* ids;
    const float *a, *b;
    const float* G;
    float alpha, ridge, ridge_per_entry;
    int32_t* status;
};
hipError_t launch_solve_rows(int L, const SolveRows& a, hipStream_t st);

// validate.hip.  Sum over the n >= 1 pairs of (double)e * (double)e with e = r[j] - dot(P[u[j]], Q[i[j]]) in fp32 (the
// bits launch_predict returns), into *out.  Pair j is added to partial j mod kPairsSlots, each partial in ascending j,
// and launch_reduce_sse folds the pairs_sse_partials(n) partials that have a pair: the 64 bits of *out are a function of
// the factors, the pair list in its order and k, of nothing else.  partial: room for kPairsSlots doubles.  Every user
// is a row of P and every item a row of Q (kp-padded rows): the caller checks.  Asynchronous on st.
constexpr int kPairsSlots = 16384;
int64_t pairs_sse_partials(int64_t n);
hipError_t launch_pairs_sse(int L, const float* P, const float* Q, const int32_t* u, const int32_t* i, const float* r,
                            int64_t n, double* partial, double* out, hipStream_t st);

}  // namespace mfsgd
