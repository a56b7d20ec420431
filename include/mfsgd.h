/*
 * mfsgd.h -- C-ABI of libmfsgd.so, the MI355X (gfx950) matrix-factorisation
 * SGD trainer.  This is the drop-in boundary: what a JNI / ctypes / cgo stub
 * binds.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Reference interface replaced: NONE EXISTS.  /root/reference/README.md:1-2 is
 * the whole reference repository (a title and a course attribution); it has no
 * class, no FFI and no operator interface.  The surface below follows
 * SURVEY.md section 8b, which derives it from BASELINE.json's north_star
 * ("keeping the Java MatrixFactorizationSGD train()/predict() surface ...
 * through a thin JNI C-ABI").  Each entry point names the Java method it backs
 * (matrixfactorizationsgd.java_amd/java/MatrixFactorizationSGD.java).
 *
 * Conventions
 *  - every function returns MFSGD_OK (0) or a negative mfsgd_status;
 *    the message is available from mfsgd_last_error();
 *  - no C++ exception and no HIP error crosses this boundary;
 *  - the caller owns every host array passed in or out; the library copies;
 *  - the handle owns all device memory; mfsgd_destroy() frees it;
 *  - a handle is not thread-safe; distinct handles are independent;
 *  - there is NO CPU fallback: compute entry points return
 *    MFSGD_ERR_NO_DEVICE when no gfx950 device is usable.  Host-only entry
 *    points (create, set_ratings = schedule construction, schedule queries)
 *    work without a GPU.
 */
#ifndef MFSGD_H
#define MFSGD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFSGD_ABI_VERSION 3 /* 3 (round 3): + mfsgd_part_settle, mfsgd_dsgd_plan_ex, mfsgd_dsgd_stats; solo-record word order in the debug arrays; + mfsgd_recommend_excluding, mfsgd_fold_in_users, mfsgd_recommend_rows; + mfsgd_rank_items, mfsgd_rank_items_rows, mfsgd_ranking_metrics_from_ranks, mfsgd_evaluate_ranking; + mfsgd_set_hyper, mfsgd_get_hyper, mfsgd_train_schedule, mfsgd_train_bold_driver; + mfsgd_set_validation, mfsgd_validation_size, mfsgd_validation_rmse, mfsgd_rmse_pairs, mfsgd_train_early_stop; + mfsgd_row_inv_norms, mfsgd_similar_items, mfsgd_similar_users, mfsgd_similar_rows; + mfsgd_online_levels, mfsgd_apply_ratings; + mfsgd_fold_in_items, mfsgd_append_users, mfsgd_append_items, mfsgd_reserve_rows, mfsgd_get_capacity; + mfsgd_recommend_among, mfsgd_recommend_rows_among, mfsgd_debug_serve_seconds; + mfsgd_set_seen, mfsgd_mark_seen, mfsgd_clear_seen, mfsgd_seen_size, mfsgd_get_seen, mfsgd_recommend_unseen, mfsgd_recommend_unseen_among, mfsgd_rank_items_unseen, mfsgd_evaluate_ranking_unseen; + mfsgd_sample_unseen; + mfsgd_triple_levels, mfsgd_apply_triples, mfsgd_bpr_weights; + mfsgd_sample_unseen_hard; + mfsgd_sample_unseen_violating, mfsgd_apply_triples_weighted, mfsgd_warp_weights; + mfsgd_fold_in_users_pairwise; + mfsgd_sample_unseen_hard_weighted, mfsgd_sample_unseen_violating_weighted, mfsgd_fold_in_users_pairwise_weighted; + mfsgd_recommend_users, mfsgd_recommend_users_among, mfsgd_recommend_users_unseen, mfsgd_recommend_users_unseen_among, mfsgd_recommend_users_rows, mfsgd_recommend_users_rows_among (additions: no existing call changed) */

typedef enum mfsgd_status {
    MFSGD_OK = 0,
    MFSGD_ERR_INVALID_ARG = -1,
    MFSGD_ERR_NO_DEVICE = -2,   /* no HIP device / wrong architecture          */
    MFSGD_ERR_HIP = -3,         /* a HIP runtime call failed (see last_error)  */
    MFSGD_ERR_OOM = -4,         /* host or device allocation failed            */
    MFSGD_ERR_STATE = -5,       /* call order violated (e.g. train before set) */
    MFSGD_ERR_UNSUPPORTED = -6, /* e.g. k > MFSGD_MAX_K                        */
    MFSGD_ERR_SCHEDULE = -7     /* schedule could not be built (bad index, 32-bit overflow) */
} mfsgd_status;

#define MFSGD_MAX_K 256

typedef struct mfsgd_handle mfsgd_handle;

/* Hyper-parameters and geometry.  Zero in an "auto" field selects the default.
 * Java: constructor MatrixFactorizationSGD(users, items, k, lr, lambda, seed). */
typedef struct mfsgd_config {
    int32_t n_users;      /* U: rows of P held by this handle                       */
    int32_t n_items;      /* I: rows of Q (global item count)                       */
    int32_t k;            /* latent dimension, 1..MFSGD_MAX_K                       */
    float lr;             /* learning rate                                          */
    float lambda;         /* L2 regularisation, shared by P and Q                   */
    int32_t device;       /* HIP device ordinal                                     */
    int32_t blocks;       /* B: user blocks = item tiles per side; 0 = auto         */
    int32_t waves;        /* W: waves per workgroup (1,2,4,8); 0 = auto             */
    int32_t n_parts;      /* DSGD: item partitions (= GPUs); 0 or 1 = single device */
    int32_t host_threads; /* schedule-construction threads; 0 = hardware threads    */
    int32_t flags;        /* MFSGD_FLAG_*                                           */
    int32_t reserved[5];  /* must be zero                                           */
} mfsgd_config;

#define MFSGD_FLAG_NO_GRAPH 1     /* launch eagerly instead of replaying a hipGraph            */
#define MFSGD_FLAG_HOST_INGEST 4   /* bucket the ratings on the host even when a GPU is present     */
#define MFSGD_FLAG_DEVICE_INGEST 8 /* ... on the GPU even for small rating sets (default: >= 2^20)  */
#define MFSGD_FLAG_HOST_PACK 32     /* pack the cells on the host even when the device could (tests: both build the same bytes) */
#define MFSGD_FLAG_NO_SOLO 16      /* schedule without solo runs (A/B measurements, tests)           */
#define MFSGD_FLAG_ROUND_LAUNCH 2 /* one kernel launch per round instead of the persistent      */
                                  /* epoch kernel (which hands item tiles between workgroups)   */

/* What the scheduler built; for tests, bench.py's roofline arithmetic, DESIGN. */
typedef struct mfsgd_schedule_info {
    int64_t nnz;          /* ratings in this part                                   */
    int32_t part;         /* item partition this describes                          */
    int32_t blocks;       /* B                                                      */
    int32_t waves;        /* W                                                      */
    int32_t group_lanes;  /* L: lanes per rating (row bytes / 16)                   */
    int32_t slots;        /* G = 64 / L ratings per wave step                       */
    int32_t kp;           /* padded row length in floats (device stride)            */
    int32_t rounds;       /* rounds per epoch (= B)                                 */
    int32_t lds_bytes;    /* dynamic LDS requested per workgroup                    */
    int64_t total_steps;  /* wave steps over all cells                              */
    int64_t total_rows;   /* factor rows gathered (and scattered) per epoch         */
    int64_t max_cell_nnz;
    int64_t max_cell_rows;  /* rows of the largest chunk */
    int64_t max_cell_steps; /* critical path of the slowest cell (sum over sub-rounds of max wave steps) */
    int64_t sum_round_steps; /* sum over rounds of the slowest cell's critical path */
    double build_seconds;
    int32_t swapped;      /* 1: roles exchanged (users on the kernel's forwarding side): in the   */
    int32_t device_ingest; /* 1: degree histograms and bucket order were computed on the GPU; 2: the cells */
                           /* were packed there too (rows / entries / order never existed on the host)  */
    int64_t chunks;       /* chunk descriptors (>= blocks*blocks: one per cell + extra chunks)    */
    int64_t split_cells;  /* cells cut into more than one chunk because they exceed the LDS       */
} mfsgd_schedule_info;

/* ---- lifetime ------------------------------------------------------------- */
int mfsgd_abi_version(void);
/* Number of usable gfx950 devices; 0 (and MFSGD_OK) when there are none. */
int mfsgd_device_count(int32_t* out);
/* Java: constructor.  Does not touch the GPU. */
int mfsgd_create(const mfsgd_config* cfg, mfsgd_handle** out);
/* Java: close(). NULL is allowed. */
void mfsgd_destroy(mfsgd_handle* h);
/* Message of the last failure on this handle (h == NULL: of the last failed
 * mfsgd_create, mfsgd_ranking_metrics_from_ranks, mfsgd_bpr_weights or mfsgd_warp_weights on this thread).  Never NULL;
 * valid until the next call. */
const char* mfsgd_last_error(const mfsgd_handle* h);

/* ---- ratings -> schedule (host) -------------------------------------------
 * Java: first half of train(int[] u, int[] i, float[] r, int epochs).
 * COO triples; 0 <= u < n_users, 0 <= i < n_items.  Buckets the ratings into
 * B x B (user block, item tile) cells per item partition and packs every cell
 * into conflict-free wave steps.  Works without a GPU; with one (and >= 2^20
 * ratings) the streaming passes -- degree histograms, bucket order -- run on it,
 * with identical results.  Replaces any earlier ratings -- unless they ARE the
 * earlier ratings: the same triples again (length and a 128-bit hash of every
 * byte of the three arrays) keep the schedules and their device copies, so a host
 * may hand train() the same arrays on every call at the cost of one pass over them. */
int mfsgd_set_ratings(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r,
                      int64_t nnz);

/* ---- factors --------------------------------------------------------------
 * Host layout is dense row-major: P is n_users x k, Q is n_items x k.
 * init: java.util.Random(seed).nextFloat() * (float)(1/sqrt(k)), P then Q.
 * With n_parts > 1 only P (and nothing of Q) lives in the handle: Q travels
 * in caller-owned device blocks (mfsgd_part_* below); pass Q = NULL here.
 * NaN: which entries are NaN is kept, a NaN's sign and payload are not.  Every
 * NaN that enters the library -- a factor given to mfsgd_set_factors,
 * mfsgd_load_factors, mfsgd_append_users, mfsgd_append_items or
 * mfsgd_dsgd_set_q, a rating given to mfsgd_set_ratings
 * (in the schedules) or mfsgd_apply_ratings, a weight given to
 * mfsgd_apply_triples_weighted (lr * w is the step size of three factor rows)
 * -- is replaced by the quiet NaN
 * 0x7FC00000: the training kernels use the word 0xFFFFFFFF, itself a NaN, as
 * "not posted yet" between two of their waves, and arithmetic hands a NaN
 * operand's payload on.  mfsgd_get_factors before any training therefore
 * returns 0x7FC00000 where a NaN of another payload went in.
 * Inf: overflow propagates as the arithmetic of k columns says where k is a
 * multiple of 4 times a power of two (k == kp: 4, 8, 16, 32, 64, 128, 256).
 * At other k a device row carries zero pad columns, and in the TRAINING
 * kernels an infinite step size makes them NaN (Inf * 0): such a row turns NaN
 * one step of its own earlier than the definition's, which keeps Inf there.
 * mfsgd_apply_ratings keeps its pad columns zero and follows the definition.  */
int mfsgd_init_factors(mfsgd_handle* h, int64_t seed);
int mfsgd_set_factors(mfsgd_handle* h, const float* P, const float* Q);
int mfsgd_get_factors(mfsgd_handle* h, float* P, float* Q);

/* ---- the hot path ---------------------------------------------------------
 * Java: second half of train(...).  Runs `epochs` passes over the schedule on
 * the device.  If rmse_per_epoch != NULL it receives the RMSE after each epoch
 * (one extra read-only pass per epoch).  Blocks until the device is idle.    */
int mfsgd_train(mfsgd_handle* h, int32_t epochs, double* rmse_per_epoch);
/* RMSE over the stored ratings with the current factors. */
int mfsgd_rmse(mfsgd_handle* h, double* out);
/* Java: predict(int u, int i) / predict(int[] u, int[] i). */
int mfsgd_predict(mfsgd_handle* h, const int32_t* u, const int32_t* i, float* out, int64_t n);

/* Top-N scoring: for each of n_users users the topn items with the largest
 * dot(P[u], Q[i]) -- the same bits mfsgd_predict() returns -- best first, ties by the
 * smaller item index.  out_items / out_scores: n_users x topn, row-major.          */
int mfsgd_recommend(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, int32_t* out_items,
                    float* out_scores);
/* Top-N as mfsgd_recommend, except that item j is never returned in row b when (users[b], j) is
 * one of the n_excl pairs (excl_u[x], excl_i[x]).  Typical use: pass the u / i arrays the model
 * was trained on, so users are recommended only items they have not rated.
 * Pairs whose user is not requested are ignored.  Duplicate pairs are allowed.
 * A row with fewer than topn eligible items is padded with item -1 and score NaN.
 * n_excl == 0 (pointers may then be NULL) gives exactly mfsgd_recommend's output.
 * Every pair must lie in range (0 <= excl_u < n_users, 0 <= excl_i < n_items); a bad argument
 * is reported before any device work.  topn > n_items stays an error, a topn above the
 * number of eligible items is not.  The pairs are read in chunks of bounded size; the
 * per-user lists are built on the device for this call and freed before it returns.     */
int mfsgd_recommend_excluding(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, const int32_t* excl_u,
                              const int32_t* excl_i, int64_t n_excl, int32_t* out_items, float* out_scores);

/* Fold-in: rows for n_new users that are not in the model, against the model's item factors Q, which stay fixed.
 * New user x owns the ratings row_ptr[x] .. row_ptr[x + 1] (CSR, row_ptr[0] == 0) of items / ratings.  Its row starts
 * as init_rows[x] (n_new x k, dense) or, with init_rows == NULL, as row x of the P that mfsgd_init_factors(seed) gives
 * a model of n_new users (element f: draw x * k + f of java.util.Random(seed), nextFloat() / sqrt(k)).  Then, `epochs`
 * times over the user's ratings in the order given, the P half of the canonical update:
 *     q = Q[items[j]];  d = dot(row, q);  s = fma(-lr, d, lr * ratings[j]);  row[f] = fma(s, q[f], (1 - lr * lambda) * row[f])
 * with the handle's lr and lambda.  out_rows (n_new x k, dense) receives the rows: bit for bit what the CPU oracle's
 * update gives for p.  A user without ratings and epochs == 0 are valid (the start row comes back), and so is an item
 * twice in one list (two steps).  The model is not modified.  A user's chain is sequential: one very long user costs
 * length x epochs dependent steps however many other users there are.
 * Arguments are checked before any device work (MFSGD_ERR_INVALID_ARG, message "fold_in: ..."): negative n_new or
 * epochs, a null array that is needed, row_ptr[0] != 0, a decreasing row_ptr, an item outside [0, n_items).
 * MFSGD_ERR_STATE: n_parts != 1 (the handle does not hold Q), or factors never initialised, set or loaded.
 * n_new == 0 is MFSGD_OK.  Ratings go to the device in batches of whole users of bounded size.                      */
int mfsgd_fold_in_users(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* items, const float* ratings,
                        int32_t epochs, const float* init_rows, int64_t seed, float* out_rows);
/* The mirror of mfsgd_fold_in_users: rows for n_new ITEMS that are not in the model, against the model's user factors P,
 * which stay fixed.  New item x owns the ratings row_ptr[x] .. row_ptr[x + 1] of users / ratings.  Its row starts as
 * init_rows[x] or, with init_rows == NULL, as row x of the P that mfsgd_init_factors(seed) gives a model of n_new users
 * (the same draws mfsgd_fold_in_users starts from).  Then, `epochs` times over the item's ratings in the order given:
 *     p = P[users[j]];  d = dot(row, p);  s = fma(-lr, d, lr * ratings[j]);  row[f] = fma(s, p[f], (1 - lr * lambda) * row[f])
 * The canonical dot and the update are bitwise symmetric in their two rows, so out_rows is bit for bit what the CPU
 * oracle's update gives for q.  Checks, their order, the state errors (the call asks for a Q in the handle as well,
 * for the symmetry of the contract) and the batching are those of mfsgd_fold_in_users; the messages start with
 * "fold_in_items: " and name the user of a rating where those name its item.  The model is not modified.             */
int mfsgd_fold_in_items(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* users, const float* ratings,
                        int32_t epochs, const float* init_rows, int64_t seed, float* out_rows);
/* Pairwise fold-in: rows for n_new users that are not in the model, from their positives alone, for a model that only
 * orders items (mfsgd_apply_triples: fit_bpr, fit_warp).  Each new user runs a BPR chain of its own against the model's
 * item factors Q, which stay fixed, and draws its own negatives among the items it has not named.  New user x owns the
 * positives A = items[row_ptr[x] .. row_ptr[x + 1]) (CSR, row_ptr[0] == 0), of length len, in the order given; an item
 * twice in one list gives two steps per epoch.  T = row_ptr[n_new].  The start rows are mfsgd_fold_in_users': init_rows
 * (n_new x k, dense) or, with init_rows == NULL, the rows seeded by `seed`.
 * The rule.  A pure function of the start row, A, Q's bits, n_items, lr, lambda, epochs, m, draw_seed and the row's
 * counter range.  S is A sorted and made distinct, of length s; cnt = n_items - s.  For e = 0 .. epochs - 1, then
 * a = 0 .. len - 1, the step tau = e * len + a:
 *     c_d     = first + ((row_ptr[x] * epochs + tau) * m + d),  d = 0 .. m - 1      unsigned 64-bit, as mfsgd_sample_unseen
 *     cand[d] = mfsgd_sample_unseen's draw for (draw_seed, c_d, S, n_items): with r its 32-bit mix, t = (r * cnt) >> 32,
 *               cand[d] = t + p, p = the number of q in [0, s) with S[q] - q <= t
 *     pick    = 0 if m == 1, otherwise mfsgd_sample_unseen_hard's pick over score(d) = dot(row, Q[cand[d]]) with the row
 *               as it is NOW: the largest non-NaN score, scores equal as floats to the smaller d, all NaN to d = 0
 *     i = A[a];  j = cand[pick]
 *     xm = dot(row, Q[i]) - dot(row, Q[j]);  g = lsig(xm);  sz = lr * g;  c = 1 - lr * lambda
 *     row[f] = fma(sz, Q[i][f] - Q[j][f], c * row[f])                the p line of mfsgd_apply_triples, nothing else
 *     out_margin[row_ptr[x] * epochs + tau] = xm;  out_neg[row_ptr[x] * epochs + tau] = j         (either nullable)
 * dot is the canonical dot and lsig the logistic weight of DESIGN.md section 3; everything is fp32, nothing is
 * contracted.  With cnt == 0 (the list names every item) no step is taken: the start row comes back, the user's margins
 * are 0x7FC00000 and their negatives -1.  A user without positives and epochs == 0 are valid (the start row comes back).
 * Counters.  User x owns the counters first + row_ptr[x] * epochs * m .. first + row_ptr[x + 1] * epochs * m, so a call
 * can be split and reordered: users [a, b) of a call are the call on row_ptr rebased to a (row_ptr[a .. b] - row_ptr[a],
 * items + row_ptr[a], init_rows + a * k) with first + row_ptr[a] * epochs * m.  With seeded start rows the split call
 * must be given its rows through init_rows, the seeded rows being numbered from 0 in every call.
 * Checks, all before any device work, in this order ("fold_in_pairwise: ..."): MFSGD_ERR_INVALID_ARG for a negative n_new
 * or epochs; for m < 1; for a negative first, or first + T * epochs * m above 2^63 - 1; for a null array that is needed
 * (row_ptr and out_rows with n_new > 0, items with T > 0), row_ptr[0] != 0, a decreasing row_ptr or more than 2^32 - 1
 * positives of one user; for an item outside [0, n_items), the message naming its position in items.  Then
 * MFSGD_ERR_STATE as mfsgd_fold_in_users reports it: n_parts != 1, factors never initialised, set or loaded, or no Q.
 * Then n_new == 0 is MFSGD_OK and touches nothing.  A valid call with n_new > 0 and no usable GPU is MFSGD_ERR_NO_DEVICE.
 * The call needs no seen-item index and no stored ratings, and modifies neither the model nor any schedule, cached
 * graph, index, item weights or held-out set.  Positives go to the device in batches of whole users of at most 2^22
 * positives (a user with more is a batch of its own); each batch's lists S are built there, and 4 bytes per step come
 * down for each of out_margin and out_neg that is asked for.  All staging is freed before the call returns, on every
 * path -- mfsgd_debug_device_bytes is the same before and after.  A user's chain is sequential, as in
 * mfsgd_fold_in_users.  Not done here: WARP-style picks, new items, a lambda of its own for negatives (weighted draws:
 * mfsgd_fold_in_users_pairwise_weighted below). */
int mfsgd_fold_in_users_pairwise(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* items,
                                 int32_t epochs, int32_t m, const float* init_rows, int64_t seed, int64_t draw_seed,
                                 int64_t first, float* out_rows, float* out_margin /* nullable, T * epochs */,
                                 int32_t* out_neg /* nullable, T * epochs */);
/* mfsgd_fold_in_users_pairwise_weighted: mfsgd_fold_in_users_pairwise for a model trained against weighted negatives (item
 * weights: mfsgd_set_item_weights, further down).  It is that call's rule with one line replaced:
 *     cand[d] = mfsgd_sample_unseen_weighted's draw for (draw_seed, c_d, S, the handle's weights, n_items): with z its
 *               64-bit mix, cnt the unseen WEIGHT of S and g the unseen-mass table of S, t = (z * cnt) >> 64 and the
 *               two searches of that call
 * The counters c_d, the pick, the step, the outputs and the way a call can be split are unchanged.  "cnt == 0" reads
 * "the user's unseen weight is 0" -- the list names every item of positive weight, or all weights are zero --: no step
 * is taken, the start row comes back, the user's margins are 0x7FC00000 and their negatives -1.  An item of weight 0 is
 * never a negative.  Unit weights do NOT reproduce mfsgd_fold_in_users_pairwise: that call's draw uses the 32-bit r.
 * Checks, all before any device work, in this order ("fold_in_pairwise_weighted: ..."): the argument checks of
 * mfsgd_fold_in_users_pairwise; its state checks (n_parts != 1, factors never initialised, set or loaded, no Q); then
 * MFSGD_ERR_STATE for a handle without weights ("no item weights") and for weights that no longer cover the model ("item
 * weights cover X items, the model has Y", after mfsgd_append_items).  Then n_new == 0 is MFSGD_OK and touches nothing.  A
 * valid call with n_new > 0 and no usable GPU is MFSGD_ERR_NO_DEVICE.
 * The call needs no seen-item index and no stored ratings, and modifies nothing in the handle: not the model, the
 * weights, the index or its mass table, a schedule or a cached graph.  Per batch, after the lists S are built, their
 * unseen-mass table is built the way the index's is (the pairs' weights, one device-wide exclusive scan, g): staging of
 * 16 bytes per distinct positive of the batch plus the scan's scratch, on top of mfsgd_fold_in_users_pairwise's, all of
 * it freed before the call returns, on every path -- mfsgd_debug_device_bytes is the same before and after.             */
int mfsgd_fold_in_users_pairwise_weighted(mfsgd_handle* h, int32_t n_new, const int64_t* row_ptr, const int32_t* items,
                                          int32_t epochs, int32_t m, const float* init_rows, int64_t seed, int64_t draw_seed,
                                          int64_t first, float* out_rows, float* out_margin /* nullable, T * epochs */,
                                          int32_t* out_neg /* nullable, T * epochs */);
/* Top-N as mfsgd_recommend_excluding, where "user j" is rows[j] (n_rows x k, dense: for instance what
 * mfsgd_fold_in_users returned) instead of a row of P: every row is answered, in order, and excl_row[x] indexes rows.
 * Same ordering, padding, scores and argument checks, with n_rows in the place of n_users.                           */
int mfsgd_recommend_rows(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn, const int32_t* excl_row,
                         const int32_t* excl_item, int64_t n_excl, int32_t* out_items, float* out_scores);
/* Top-N among candidates: "the best topn of these items", for a re-ranking step whose lists come from retrieval, a
 * category, the stock.  Row b of the output holds the topn best items of row b's candidate list that no exclusion pair
 * of users[b] removes, ordered exactly as mfsgd_recommend_excluding orders (larger score first; scores that compare
 * equal as floats, -0.0 == +0.0, by the smaller ITEM INDEX, not by the place in the list), scores being the bits
 * mfsgd_predict() returns, and padded with item -1 and score NaN where fewer than topn are eligible: it is
 * mfsgd_recommend_excluding(users[b], topn = n_items, the same pairs) with every item outside the list deleted, cut or
 * padded to topn.  A list that names every item gives that call's row bit for bit; NaN scores are handled as there.
 * The lists: cand_ptr == NULL, one list cand_items[0 .. n_cand) shared by every requested row; otherwise CSR over the
 * REQUEST ROWS -- row b is the position in users, not the user id, so one user asked for twice may carry two lists --
 * row b owning cand_items[cand_ptr[b] .. cand_ptr[b + 1]), with cand_ptr[0] == 0, cand_ptr non-decreasing and
 * cand_ptr[n_users] == n_cand.  A list may come in any order and name an item more than once (it counts once); an
 * empty list is valid (a row of padding), and so is a topn above a list's length.
 * Arguments are checked before any device work, in mfsgd_recommend_excluding's order with the candidates after the
 * users and before the exclusion pairs (MFSGD_ERR_INVALID_ARG, message "recommend_among: ..."): that call's own checks
 * (topn < 1 and topn > n_items among them), then a negative n_cand, a null cand_items with n_cand > 0, each of the three
 * cand_ptr rules, a candidate outside [0, n_items) (the message names its position in cand_items), more than 2^32 - 1
 * candidates.  After mfsgd_append_items the new indices are valid candidates; those between count and capacity are not.
 * MFSGD_ERR_STATE and MFSGD_ERR_NO_DEVICE as mfsgd_recommend_excluding reports them; n_users == 0 is MFSGD_OK.
 * Cost: work and device memory per request row follow its list and its user's exclusion list, never n_items.  The
 * candidates are read in chunks of bounded size; the lists are sorted and made distinct on the device for this call
 * and freed before it returns, on every path.  The model is not modified.                                            */
int mfsgd_recommend_among(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, const int64_t* cand_ptr,
                          const int32_t* cand_items, int64_t n_cand, const int32_t* excl_u, const int32_t* excl_i,
                          int64_t n_excl, int32_t* out_items, float* out_scores);
/* mfsgd_recommend_among where "user j" is rows[j] (n_rows x k, dense), as mfsgd_recommend_rows is to
 * mfsgd_recommend_excluding: every row is answered, in order, cand_ptr (n_rows + 1 entries) and excl_row index the rows.
 * Messages start with "recommend_rows_among: ".                                                                      */
int mfsgd_recommend_rows_among(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn, const int64_t* cand_ptr,
                               const int32_t* cand_items, int64_t n_cand, const int32_t* excl_row, const int32_t* excl_item,
                               int64_t n_excl, int32_t* out_items, float* out_scores);

/* ---- ranking quality: where held-out items land, and the top-N metrics of that ------------------------------------
 * out_rank[x] = how many items come before items[x] in users[x]'s recommendation order, among the items that are
 * eligible for that user: the position (0 = best) items[x] takes in the list mfsgd_recommend_excluding(users[x],
 * topn = n_items, the same pairs) returns, with items[x] itself counted as eligible even if a pair excludes it.
 * Order: item j comes before item t when score(j) > score(t), or when the two scores compare equal as floats (-0.0
 * equals +0.0) and j < t; scores are the bits mfsgd_predict() returns.  Ranks are exact integers.  The rank of a pair
 * whose score is NaN is unspecified, and so are the ranks of a user any of whose items scores NaN.
 * Eligibility: item j competes for user u unless (u, j) is one of the n_excl pairs; a user's other held-out items
 * compete like any other item.  Duplicate pairs are allowed in both lists (a duplicate held-out pair gets the same
 * rank twice); exclusion pairs of users without a held-out pair are ignored.
 * Nothing of size users x n_items exists anywhere: the device counts, per pair, the items that beat it (csrc/rank.hip).
 * Arguments are checked before any device work (MFSGD_ERR_INVALID_ARG, message "rank_items: ..."): negative n or
 * n_excl, a null array that is needed, a user or item out of range in either list (also in exclusion pairs of users
 * nobody asked about); for mfsgd_rank_items_rows also a negative n_rows and a null rows with n_rows > 0, and "in range"
 * means below n_rows.  MFSGD_ERR_STATE: n_parts != 1, or (with n > 0) factors never initialised, set or loaded.
 * MFSGD_ERR_NO_DEVICE: a valid call with n > 0 and no usable GPU; there is never a CPU result.  n == 0 is MFSGD_OK and
 * touches nothing.  The model is not modified; the pairs go to the device in pieces of bounded size and
 * everything allocated there is freed before the call returns.                                                      */
int mfsgd_rank_items(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n,
                     const int32_t* excl_u, const int32_t* excl_i, int64_t n_excl, int32_t* out_rank);
/* The same where "user j" is rows[j] (n_rows x k, dense; e.g. what mfsgd_fold_in_users returned); row_of_pair and
 * excl_row index rows. */
int mfsgd_rank_items_rows(mfsgd_handle* h, const float* rows, int32_t n_rows, const int32_t* row_of_pair,
                          const int32_t* items, int64_t n, const int32_t* excl_row, const int32_t* excl_item,
                          int64_t n_excl, int32_t* out_rank);

typedef struct mfsgd_ranking_metrics {
    int64_t n_pairs, n_users;                                /* pairs given; distinct users among them */
    double hit_rate, precision, recall, ndcg, mrr;           /* means over those users */
} mfsgd_ranking_metrics;
/* Host only, no handle, works without a GPU: the metrics of (users[x], ranks[x]) pairs at cut-off topn.  For user u
 * with pairs T_u and their ranks r_t: hits = #{t : r_t < topn}; hit = (hits > 0); precision = hits / topn;
 * recall = hits / |T_u|; ndcg = DCG / IDCG with DCG = sum over r_t < topn of 1 / log2(r_t + 2) and IDCG = sum over
 * p < min(|T_u|, topn) of 1 / log2(p + 2); mrr = 1 / (min r_t + 1), which is not cut at topn.  Each field is the mean
 * of its per-user value over the users that have a pair, summed in fp64 in ascending user order; n == 0 gives zeros.
 * Duplicate pairs are NOT detected: the caller passes distinct (user, item) pairs for the metrics to mean anything.
 * MFSGD_ERR_INVALID_ARG (message "ranking_metrics: ...", from mfsgd_last_error(NULL)): negative n, topn < 1, a null
 * pointer that is needed, a negative rank.                                                                         */
int mfsgd_ranking_metrics_from_ranks(const int32_t* users, const int32_t* ranks, int64_t n, int32_t topn,
                                     mfsgd_ranking_metrics* out);
/* mfsgd_rank_items followed by mfsgd_ranking_metrics_from_ranks.  out_rank may be NULL.  topn < 1 and a null `out`
 * are MFSGD_ERR_INVALID_ARG as well, before any device work. */
int mfsgd_evaluate_ranking(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t topn,
                           const int32_t* excl_u, const int32_t* excl_i, int64_t n_excl,
                           mfsgd_ranking_metrics* out, int32_t* out_rank);

/* ---- the seen-item index: what each user has already seen, kept on the device ----------------------------------------
 * mfsgd_recommend_excluding and its kin take the complete (user, item) pair list on every call, check it, upload it and
 * sort it into per-user lists that are freed before they return.  The index is those lists built once and kept in the
 * handle: one sorted, distinct item list per user in CSR form on the device, extended in place as ratings arrive and
 * read by the _unseen calls below where it lies.  A handle has no index until mfsgd_set_seen or mfsgd_mark_seen; an
 * empty index (no pairs) is a valid state, and the _unseen calls then exclude nothing.
 * All of these calls are for single-partition handles (n_parts != 1: MFSGD_ERR_STATE), check their arguments before any
 * device work, run on the handle's stream and return with the device idle.
 * The index and the model do not touch each other: mfsgd_set_ratings, mfsgd_set_hyper, seeding, setting or loading
 * factors, training, mfsgd_apply_ratings (it does NOT mark: pass the same u / i to mfsgd_mark_seen), the validation calls,
 * fold-in and mfsgd_append_items leave the index as it is, and the index changes no factor bit, no schedule and no cached
 * training graph.  Users added by mfsgd_append_users have empty lists; inside the reserved capacity that append allocates
 * nothing for the index, and one that reallocates, like mfsgd_reserve_rows, copies the per-user tables device to device
 * into larger ones, new before old (MFSGD_ERR_OOM leaves everything as it was; every list is kept).
 * Memory: with D distinct pairs, 4 D + 12 user_capacity + 8 bytes of device memory (4 per pair; per user of capacity 8
 * of offset and 4 of the table through which the kernels reach a list by user id), all of it counted by
 * mfsgd_debug_device_bytes; an empty index and a handle without one hold nothing.  (A handle with item weights holds
 * 8 D bytes more beside the index: "weighted negatives" below.)
 *
 * mfsgd_set_seen: the index becomes the distinct pairs of (u[x], i[x]), x < n; duplicates count once.  Needs neither
 * factors nor ratings.  Every pair must satisfy 0 <= u < n_users and 0 <= i < n_items under the handle's CURRENT counts
 * (rows appended to the model are valid).  MFSGD_ERR_INVALID_ARG, message "set_seen: ...", in this order: a negative n; a
 * null array with n > 0; (then MFSGD_ERR_STATE for n_parts != 1;) a pair out of range -- the message names its position;
 * more than 2^32 - 1 pairs.  n == 0 leaves an empty index, on the host alone: it works without a GPU.  A valid call
 * with n > 0 and no usable GPU is MFSGD_ERR_NO_DEVICE.  The pairs go up in chunks of 2^22 (32 MB of staging, whatever
 * n is) and are sorted and made distinct on the device.  The new index is complete before the old one is released, so a
 * failure (MFSGD_ERR_OOM, MFSGD_ERR_HIP, MFSGD_ERR_NO_DEVICE) leaves the old one as it was.  Transient peak on top of the
 * old and the new index: 16 bytes per pair given (keys, and the sort's second buffer), the staging, and the sort's
 * scratch; all of it is freed before the call returns.
 * mfsgd_mark_seen: the index becomes the union of itself and the pairs; on a handle without an index, or with an empty
 * one, it is mfsgd_set_seen.  n == 0 touches nothing, except that a handle without an index gets an empty one.  Checks
 * and failure rule are mfsgd_set_seen's, the messages start with "mark_seen: ".  The index does not go through a sort
 * again: the batch is sorted and made distinct, the keys the index lacks are found by a binary search each, and every
 * element of the merged index is placed on its own -- work linear in D + n (times the logarithm of a search), nothing
 * serial in a user's list length.  A batch that adds nothing allocates no new index.  Transient peak: the old index
 * beside the new one (4 (D + new pairs) + 8 (user_capacity + 1)), 17 bytes per pair of the batch, staging and scratch.
 * mfsgd_clear_seen: the handle has no index afterwards, and all of its device memory is freed.
 * mfsgd_seen_size: *pairs = D, or -1 when the handle has no index.  Host only.
 * mfsgd_get_seen: row_ptr (n_users + 1 entries) receives the CSR offsets of the requested users' lists, in the order
 * requested; users may repeat.  With items != NULL and items_capacity >= row_ptr[n_users] it receives the lists too,
 * ascending; a smaller capacity is MFSGD_ERR_INVALID_ARG with the needed size in the message and in row_ptr.  A gather
 * kernel collects the lists: nothing of size D crosses the bus unless it was asked for.  MFSGD_ERR_INVALID_ARG
 * ("get_seen: ..."): negative n_users, null row_ptr, null users with n_users > 0, negative items_capacity; then
 * MFSGD_ERR_STATE for n_parts != 1 and for a handle without an index ("no seen set"); then a user out of range.
 * n_users == 0 is MFSGD_OK.                                                                                            */
int mfsgd_set_seen(mfsgd_handle* h, const int32_t* u, const int32_t* i, int64_t n);
int mfsgd_mark_seen(mfsgd_handle* h, const int32_t* u, const int32_t* i, int64_t n);
int mfsgd_clear_seen(mfsgd_handle* h);
int mfsgd_seen_size(const mfsgd_handle* h, int64_t* pairs);
int mfsgd_get_seen(mfsgd_handle* h, const int32_t* users, int32_t n_users, int64_t* row_ptr /* n_users + 1 */,
                   int32_t* items /* nullable */, int64_t items_capacity);
/* mfsgd_sample_unseen: negative sampling for implicit feedback (clicks, plays: positives only).  Row x of out_items
 * receives m items drawn uniformly, with replacement, among the items user users[x] has NOT seen according to the index;
 * users may repeat and come in any order.  "Unseen" means unseen by the index, whatever the rating set holds: pairs that
 * must never be drawn (held-out positives, say) belong in the index.  Items appended with mfsgd_append_items are unseen by
 * everybody, users appended with mfsgd_append_users have empty lists.
 * The draw.  Draw d of row x has the counter c = first + x * m + d and is a pure function of (seed, c), that user's list S
 * (sorted, distinct, length s) and the handle's current n_items -- not of n, of the other rows, of how a caller cuts one
 * call into several (rows [a, b) of a call are the call on users + a with first + a * m), or of the device.  All of it in
 * unsigned 64-bit arithmetic that wraps:
 *     z = (uint64)seed + 0x9E3779B97F4A7C15 * (c + 1)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *     z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *     z =  z ^ (z >> 31)
 *     r = z >> 32
 *     cnt = n_items - s;  cnt == 0: out = -1 (the user has seen everything)
 *     t = (r * cnt) >> 32                in [0, cnt), each value's probability within 2^-32 of 1 / cnt
 *     p = the number of positions q in [0, s) with S[q] - q <= t
 *     out = t + p                        the t-th unseen item, counting from 0 in ascending order
 * S[q] - q never decreases, so p is one binary search: a draw is exact, never rejected and retried, and costs O(log s)
 * however much the user has seen.  Two draws of a row may give the same item.  An empty index gives out = t.
 * Checks, all before any device work, in this order.  MFSGD_ERR_INVALID_ARG ("sample_unseen: ..."): a negative n or m; a
 * negative first, or first + n * m above 2^63 - 1; null users or out_items with n * m > 0.  Then MFSGD_ERR_STATE for
 * n_parts != 1 and for a handle without an index ("no seen set").  Then MFSGD_ERR_INVALID_ARG for a user outside
 * [0, n_users); the message names the row, and out_items is untouched.  n * m == 0 is MFSGD_OK past the state checks
 * and touches nothing.  A valid call with work to do and no usable GPU is MFSGD_ERR_NO_DEVICE, an empty index included:
 * there is never a CPU result.  Needs neither factors nor ratings, and modifies neither the model nor the index.
 * Cost: one thread per draw reads its user's two offsets and searches the list in the index where it lies; no pass over
 * the pairs of the index or over n_items.  The rows go up and the draws come down in pieces of whole rows of at most
 * 2^22 draws (a row with more is a piece of its own): at most 32 MB of staging whatever n is (more only for such a row),
 * all of it freed before the call returns, on every path -- mfsgd_debug_device_bytes is the same before and after.     */
int mfsgd_sample_unseen(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                        int32_t* out_items /* n x m, row-major */);
/* Weighted negatives: mfsgd_sample_unseen_weighted draws unseen items in proportion to a weight per item -- a power of
 * the item's popularity, usually (word2vec's count^0.75) -- where mfsgd_sample_unseen draws them uniformly.  With a
 * long-tailed catalogue nearly every uniform negative is an obscure item the model ranks low already.
 * Weights.  Integers, 0 <= w[i] < 2^32, one per item: integers keep the draw exact and the same on every device (no pow
 * decides a bit of it).  An item of weight 0 is never drawn; all weights zero is valid, and every draw is then -1.  The
 * handle keeps C, the exclusive prefix of w (C[0] = 0, C[n_items] = W < 2^63 by construction), uint64 on the device.
 * Weights belong to the items, not to the index: they survive mfsgd_set_seen, mfsgd_mark_seen and mfsgd_clear_seen, and
 * need no index to be set.  mfsgd_append_items leaves them as they are, so that they no longer cover the model:
 * mfsgd_sample_unseen_weighted is then MFSGD_ERR_STATE ("item weights cover X items, the model has Y") until they are set
 * again.  Single-partition handles only (MFSGD_ERR_STATE), like the index.
 * The unseen-mass table.  On a handle that has both weights and an index with pairs, g[q], for every pair of the index,
 * is the weight of the UNSEEN items below S[q] in that user's list: uint64, 8 bytes per pair, beside the index's items,
 * never decreasing along a list.  It is built eagerly by whichever call completes that state or changes either side --
 * mfsgd_set_item_weights, and mfsgd_set_seen / mfsgd_mark_seen on a handle that has weights -- on the device: the
 * pairs' weights are gathered, one device-wide exclusive scan (rocPRIM) sums them, and g[q] = C[S[q]] less the scanned
 * weight before q in its own list.  It follows the index's rule: the new table is complete before the old one is
 * released, and a failure leaves index, weights and table as they were.  A mark_seen that adds nothing builds nothing.
 * mfsgd_append_users and mfsgd_reserve_rows do not move pairs and do not touch it; mfsgd_clear_seen and an empty index
 * drop it; mfsgd_clear_item_weights drops it and C.  (Under weights that mfsgd_append_items left behind, the items
 * appended since weigh nothing in a table built meanwhile; setting the weights again rebuilds it.)
 * Memory on top of the index: 8 D + 8 (n_items + 1) bytes, all of it counted by mfsgd_debug_device_bytes; without pairs
 * 8 (n_items + 1).  Transient peak of a build, on top of what the call has otherwise: 8 D bytes of scanned weights and
 * the scan's scratch, freed before the call returns.  A handle that never sets weights allocates and runs nothing of this.
 *
 * mfsgd_set_item_weights: the weights become w[0 .. n).  MFSGD_ERR_INVALID_ARG ("set_item_weights: ..."): a negative n;
 * a null w; (then MFSGD_ERR_STATE for n_parts != 1;) n other than the current n_items.  Then a device is needed
 * (MFSGD_ERR_NO_DEVICE otherwise): the prefix is summed on the host and goes up whole.
 * mfsgd_get_item_weights: *n = the item count the weights were set for, or -1 when the handle has none; with w != NULL
 * and weights, w[i] = C[i + 1] - C[i] for those *n items.  A null n is MFSGD_ERR_INVALID_ARG.
 * mfsgd_clear_item_weights: the handle has no weights afterwards, and C and g are freed.
 * mfsgd_seen_item_counts: counts[i], i < n_items, = the number of users whose list holds item i -- the popularity the
 * weights are usually made of.  A histogram over the index's items on the device, with integer atomics: the result
 * does not depend on the order of arrival.  An empty index gives zeros, on the host alone.  MFSGD_ERR_INVALID_ARG for a
 * null counts, then MFSGD_ERR_STATE for n_parts != 1 and for a handle without an index ("no seen set").
 * mfsgd_sample_unseen_weighted: mfsgd_sample_unseen with the weighted draw -- the same rows, counters, pieces and
 * staging.  Draw d of row x has the counter c = first + x * m + d and is a pure function of (seed, c), the user's list S
 * (length s), the weights and n_items; unsigned 64-bit arithmetic but for the one 128-bit product:
 *     z    = mfsgd_sample_unseen's z, all 64 bits of it (no >> 32)
 *     cnt  = W                              if s == 0
 *          = g[s-1] + W - C[S[s-1] + 1]     otherwise               the user's unseen mass
 *     cnt == 0: out = -1                    (everything of positive weight is seen)
 *     t    = (z * cnt) >> 64                the upper half of the 128-bit product; in [0, cnt)
 *     p    = the number of q in [0, s) with g[q] <= t               one binary search, one 8-byte load per step
 *     base = C[S[p]] - g[p] if p < s, W - cnt otherwise             the seen mass below the gap the draw falls in
 *     out  = (the number of x in [0, n_items] with C[x] <= t + base) - 1          one binary search over C
 * out is unseen and has positive weight (zero-weight ties in C resolve to the item x with C[x + 1] > t + base); item x
 * comes out for exactly w[x] values of t, in ascending order, so its probability is w[x] / cnt within cnt / 2^64.  With
 * unit weights out = t + p, mfsgd_sample_unseen's rule on the 64-bit t.  An empty index gives p = 0 and base = 0.
 * out_mass[x] (nullable) receives the row's cnt: a host can weight or skip rows by it.  It is written for the rows of a
 * call that draws (n * m > 0).
 * Checks, all before any device work, in this order ("sample_unseen_weighted: ..."): mfsgd_sample_unseen's argument
 * checks; MFSGD_ERR_STATE for n_parts != 1, for a handle without an index ("no seen set"), for one without weights ("no
 * item weights"), for weights that no longer cover the model; n * m == 0 is then MFSGD_OK and touches nothing; then
 * MFSGD_ERR_INVALID_ARG for a user outside [0, n_users), named by its row, the outputs untouched.  A valid call with
 * work to do and no usable GPU is MFSGD_ERR_NO_DEVICE.  Modifies neither the model nor the index nor the weights; because
 * g is built eagerly a draw allocates staging only (as mfsgd_sample_unseen, plus 8 bytes per row of a piece with
 * out_mass), all of it freed before the call returns -- mfsgd_debug_device_bytes is the same before and after.         */
int mfsgd_set_item_weights(mfsgd_handle* h, const uint32_t* w, int32_t n /* the current n_items */);
int mfsgd_get_item_weights(mfsgd_handle* h, uint32_t* w /* nullable */, int32_t* n /* -1: none */);
int mfsgd_clear_item_weights(mfsgd_handle* h);
int mfsgd_seen_item_counts(mfsgd_handle* h, int64_t* counts /* n_items */);
int mfsgd_sample_unseen_weighted(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                                 int32_t* out_items /* n x m, row-major */, int64_t* out_mass /* nullable, n */);
/* mfsgd_sample_unseen_hard: hard negatives for pairwise ranking (dynamic negative sampling).  For each row x, the m
 * candidates mfsgd_sample_unseen would draw for users[x] are drawn, scored under the factors as they are now, and the one
 * the model likes best is returned: the negative a BPR step learns most from.  The candidates never exist in memory: 4
 * bytes per row go up and 4 to 12 come down, whatever m is.
 * Candidates.  The candidates of row x are exactly row x of mfsgd_sample_unseen(users, n, m, seed, first): candidate d has
 * the counter first + x * m + d, the same mix and the same search, off the index where it lies.
 * Score.  score(d) = dot(P[users[x]], Q[candidate d]), the canonical dot: the bits mfsgd_predict returns.
 * Pick.  The candidate with the largest non-NaN score.  Scores that compare equal as floats (-0.0 == +0.0) go to the
 * smaller d; a NaN score loses to every non-NaN score; if all m scores are NaN the pick is d = 0.  The rule does not
 * depend on the order in which candidates are examined.
 * Outputs.  out_items[x] is the picked item, out_scores[x] (nullable) its score bits, out_draw[x] (nullable) its d.  A
 * user who has seen everything gives item -1, score 0x7FC00000 and draw -1.  With m = 1 the items are
 * mfsgd_sample_unseen's column and the scores mfsgd_predict's; rows [a, b) of a call are the call on users + a with
 * first + a * m.
 * Checks, all before any device work, in this order ("sample_unseen_hard: ..."): MFSGD_ERR_INVALID_ARG for a negative n;
 * for m < 1; for a negative first, or first + n * m above 2^63 - 1; for null users or out_items with n > 0.  Then
 * MFSGD_ERR_STATE, whatever n is, for n_parts != 1, for a handle without an index ("no seen set"), and for factors that
 * were never initialised, set or loaded, or no Q after mfsgd_init_p_offset.  Then n == 0 is MFSGD_OK and touches nothing.
 * Then MFSGD_ERR_INVALID_ARG for a user outside [0, n_users); the message names the row, and the outputs are untouched.
 * A valid call with n > 0 and no usable GPU is MFSGD_ERR_NO_DEVICE, an empty index included: there is never a CPU result.
 * Modifies neither the model nor the index, nor any schedule or cached graph (factors still staged on the host move to
 * the device first, as for any call that reads them).  The users go up and the picks come down in pieces of whole rows of
 * at most 2^22 candidates (a row with more is a piece of its own), all staging freed before the call returns, on every
 * path -- mfsgd_debug_device_bytes is the same before and after.                                                       */
int mfsgd_sample_unseen_hard(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                             int32_t* out_items /* n */, float* out_scores /* nullable, n */, int32_t* out_draw /* nullable, n */);
/* mfsgd_sample_unseen_violating: the negative of a WARP step (Weston's weighted approximate-rank pairwise loss).  For each
 * row x, the m candidates mfsgd_sample_unseen would draw for users[x] are walked until one violates the margin against
 * the row's positive pos_items[x] under the factors as they are now; that candidate is returned with the number of draws
 * it took, from which the positive's rank is estimated.  The candidates never exist in memory: 8 bytes per row go up and
 * 4 to 16 come down, whatever m is.
 * The rule.  A pure function of seed and the row's counter range, the user's list, n_items and the factor bits.  For row
 * x with u = users[x], i = pos_items[x], S the user's list of length s and cnt = n_items - s:
 *     cand[d] = draw d of row x of mfsgd_sample_unseen(users, n, m, seed, first)    counter first + x * m + d, d = 0 .. m - 1
 *     sp      = dot(P[u], Q[i])                  the canonical dot: mfsgd_predict's bits
 *     x[d]    = sp - dot(P[u], Q[cand[d]])       one fp32 subtraction: the bits mfsgd_apply_triples reports as the margin
 *                                                of (u, i, cand[d]) under these factors
 *     viol(d) = cand[d] != i  and  x[d] < margin float compare: a NaN x never violates; -0.0 == +0.0; x == margin does not
 *     pick    = the smallest d with viol(d)
 *     out     = item cand[pick], draw pick, margin x[pick], rank max(1, cnt / (pick + 1))          (integer division)
 *     no d violates:           item -1, draw m,  margin 0x7FC00000, rank 0
 *     u has seen everything:   item -1, draw -1, margin 0x7FC00000, rank 0
 * cand[d] != i is part of the rule: mfsgd_apply_triples refuses i == j, and the positive need not be in the index.  rank
 * estimates how many of the cnt unseen items violate the margin: a violator at the first draw says nearly all, one at
 * draw d + 1 about one in d + 1.  The rule names a d without fixing the order in which candidates are examined: the
 * kernel skips the draws and the rows of Q past the pick, and no part of the result depends on what it skipped.  Rows
 * [a, b) of a call are the call on users + a, pos_items + a with first + a * m.
 * Checks, all before any device work, in this order ("sample_unseen_violating: ..."): MFSGD_ERR_INVALID_ARG for a negative
 * n; for m < 1; for a NaN margin (+Inf and -Inf are valid: everything but x = +Inf or NaN violates, nothing does); for a
 * negative first, or first + n * m above 2^63 - 1; for null users, pos_items or out_items with n > 0.  Then
 * MFSGD_ERR_STATE, whatever n is, for n_parts != 1, for a handle without an index ("no seen set"), and for factors that
 * were never initialised, set or loaded, or no Q after mfsgd_init_p_offset.  Then n == 0 is MFSGD_OK and touches nothing.
 * Then MFSGD_ERR_INVALID_ARG for a user outside [0, n_users) or a positive outside [0, n_items); the message names the
 * row, and the outputs are untouched.  A valid call with n > 0 and no usable GPU is MFSGD_ERR_NO_DEVICE, an empty index
 * included: there is never a CPU result.  Modifies neither the model nor the index, nor any schedule or cached graph
 * (factors still staged on the host move to the device first, as for any call that reads them).  The rows go up and the
 * picks come down in pieces of whole rows of at most 2^22 candidates (a row with more is a piece of its own), all
 * staging freed before the call returns, on every path -- mfsgd_debug_device_bytes is the same before and after.         */
int mfsgd_sample_unseen_violating(mfsgd_handle* h, const int32_t* users, const int32_t* pos_items, int64_t n, int32_t m,
                                  float margin, int64_t seed, int64_t first, int32_t* out_items /* n */,
                                  int32_t* out_draw /* nullable, n */, float* out_margin /* nullable, n */,
                                  int32_t* out_rank /* nullable, n */);
/* Weighted picks: mfsgd_sample_unseen_hard_weighted and mfsgd_sample_unseen_violating_weighted are the two calls above
 * over the candidates of mfsgd_sample_unseen_weighted, for hard negatives and WARP on a long-tailed catalogue, where
 * nearly every uniform candidate is an obscure item the model ranks low already.  The kernels are the same: the draw is
 * their only difference.
 * Candidates, both calls.  The candidates of row x are exactly row x of mfsgd_sample_unseen_weighted(users, n, m, seed,
 * first): candidate d has the counter first + x * m + d, the 64-bit z, cnt_w = the unseen weight of users[x],
 * t = (z * cnt_w) >> 64 and the two searches, over the index's mass table g and over C.  Rows [a, b) of a call are the
 * call on users + a (pos_items + a) with first + a * m.  out_mass[x] (nullable) receives the row's cnt_w, as
 * mfsgd_sample_unseen_weighted's does; it is written for every row of a call with n > 0.  Unit weights do NOT reproduce
 * the uniform calls: the uniform draw takes its rank from the 32-bit r, (r * cnt) >> 32, the weighted one from all 64
 * bits of z.  An item of weight 0 is never a candidate.
 * mfsgd_sample_unseen_hard_weighted.  mfsgd_sample_unseen_hard's score and pick over those candidates: the largest
 * non-NaN score, equal scores to the smaller d, d = 0 when all m scores are NaN.  A row with cnt_w == 0 -- the user has
 * seen everything of positive weight, or all weights are zero -- gives item -1, score 0x7FC00000 and draw -1.  With m = 1
 * the items are mfsgd_sample_unseen_weighted's column and the scores mfsgd_predict's.
 * mfsgd_sample_unseen_violating_weighted.  mfsgd_sample_unseen_violating's rule over those candidates, cand[d] != i, the
 * NaN margins that never violate and the margins of +-Inf included:
 *     out     = item cand[pick], draw pick, margin x[pick], rank max(1, N / (pick + 1))   with N = n_items - s
 *     no d violates:  item -1, draw m,  margin 0x7FC00000, rank 0
 *     cnt_w == 0:     item -1, draw -1, margin 0x7FC00000, rank 0       (N may be above 0: unseen items that weigh nothing)
 * N is the unseen item COUNT, the N of the uniform call, not cnt_w.  Under a weighted proposal the number of draws
 * estimates the violators' share of the unseen WEIGHT -- a violator at draw d + 1 says about one part in d + 1 of it --
 * and N scales that share to a number of items; it is the uniform call's estimate where popular and obscure items
 * violate alike, and counts a popular violator for more than one item otherwise.  mfsgd_warp_weights takes the result
 * unchanged.
 * Checks, all before any device work, in this order, the messages starting with the new call's name: the argument checks
 * of the uniform call (n, m, the margin, first, the null arrays); then MFSGD_ERR_STATE, whatever n is, for n_parts != 1,
 * for a handle without an index ("no seen set"), for one without weights ("no item weights"), for weights that no longer
 * cover the model ("item weights cover X items, the model has Y"), and for the factor state of the uniform call.  Then
 * n == 0 is MFSGD_OK and touches nothing.  Then MFSGD_ERR_INVALID_ARG for a user (or positive) out of range, named by its
 * row, the outputs untouched.  A valid call with n > 0 and no usable GPU is MFSGD_ERR_NO_DEVICE.  Model, index, weights,
 * mass table, schedules and cached graphs are not modified.  The pieces are the uniform calls': whole rows of at most 2^22
 * candidates (a row with more is a piece of its own), 8 more bytes per row of a piece with out_mass, all staging freed
 * before the call returns, on every path -- mfsgd_debug_device_bytes is the same before and after.
 * Cost on top of the uniform call: the second search, log2(n_items) dependent 8-byte loads per candidate.               */
int mfsgd_sample_unseen_hard_weighted(mfsgd_handle* h, const int32_t* users, int64_t n, int32_t m, int64_t seed, int64_t first,
                                      int32_t* out_items /* n */, float* out_scores /* nullable, n */,
                                      int32_t* out_draw /* nullable, n */, int64_t* out_mass /* nullable, n */);
int mfsgd_sample_unseen_violating_weighted(mfsgd_handle* h, const int32_t* users, const int32_t* pos_items, int64_t n, int32_t m,
                                           float margin, int64_t seed, int64_t first, int32_t* out_items /* n */,
                                           int32_t* out_draw /* nullable, n */, float* out_margin /* nullable, n */,
                                           int32_t* out_rank /* nullable, n */, int64_t* out_mass /* nullable, n */);
/* The serving calls against the index.  Each is the call it is named after -- mfsgd_recommend_excluding,
 * mfsgd_recommend_among, mfsgd_rank_items, mfsgd_evaluate_ranking -- given the index's pairs as its exclusion pairs:
 * order, ties, score bits, padding with -1 / NaN, the rule that a ranked pair's own item counts as eligible even if
 * excluded, and what those calls say about NaN scores carry over.  (One corner: where NO requested user has a pair, the
 * pair-list calls run their kernels without exclusions, these run them with empty lists; the two differ only in how a
 * score whose bits are all ones, a NaN no arithmetic of this library produces, ties with other NaNs.)
 * Checks are the base call's, in its order, the messages starting with the new call's name; "no seen set"
 * (MFSGD_ERR_STATE) comes right after the n_parts check, before the remaining argument checks and the factor and device
 * checks.  n_users == 0 / n == 0 stay MFSGD_OK.
 * Cost: no host loop, no upload and no device pass follows D: the kernels reach a user's list through the user id, in the
 * index where it lies, and nothing is allocated for exclusions.  mfsgd_debug_serve_seconds reports the two halves of the
 * recommend calls; the lists half covers the candidate lists only.  The model and the index are not modified.         */
int mfsgd_recommend_unseen(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn, int32_t* out_items,
                           float* out_scores);
int mfsgd_recommend_unseen_among(mfsgd_handle* h, const int32_t* users, int32_t n_users, int32_t topn,
                                 const int64_t* cand_ptr, const int32_t* cand_items, int64_t n_cand, int32_t* out_items,
                                 float* out_scores);
int mfsgd_rank_items_unseen(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t* out_rank);
int mfsgd_evaluate_ranking_unseen(mfsgd_handle* h, const int32_t* users, const int32_t* items, int64_t n, int32_t topn,
                                  mfsgd_ranking_metrics* out, int32_t* out_rank /* nullable */);

/* ---- item-side serving: the best users for an item ----------------------------------------------------------------
 * "Which users are the best audience for this item": the mfsgd_recommend family with the two sides exchanged.  Row b of
 * the output holds the topn users with the largest dot(P[u], Q[items[b]]) -- the canonical dot is bitwise symmetric in
 * its two rows, so these are the bits mfsgd_predict(u, items[b]) returns -- best first; scores that compare equal as
 * floats (-0.0 == +0.0) go to the smaller USER index; NaN scores are handled exactly as mfsgd_recommend_excluding
 * handles them; a row with fewer than topn eligible users is padded with user -1 and score NaN.  out_users /
 * out_scores: n x topn, row-major.  items may repeat and come in any order.
 * Exclusion pairs keep the orientation they have everywhere else in the library, (user, item): a caller passes the
 * same excl_u / excl_i arrays it passes to mfsgd_recommend_excluding, and user excl_u[x] is never returned in a row
 * whose item is excl_i[x].  Pairs of items nobody asked about are ignored; duplicates are allowed; n_excl == 0 (the
 * pointers may then be NULL) excludes nothing.  Every pair is range-checked under the current counts (0 <= excl_u <
 * n_users, 0 <= excl_i < n_items) before any device work.
 * The _unseen calls exclude user u from item j's row when the handle's seen-item index holds (u, j): the output is
 * byte for byte that of the pair call given the index's pairs.  A handle without an index is MFSGD_ERR_STATE ("no seen
 * set"); an empty index excludes nothing and builds nothing.  The index is CSR by user and nothing by item is kept in
 * the handle (mfsgd_set_seen, mfsgd_mark_seen, mfsgd_append_users and mfsgd_reserve_rows are what they were), so each
 * such call reads the whole index on the device (csrc/audience.hip): with D pairs in the index, two passes of 4 D
 * bytes each (one counts the pairs of requested items, one writes them), a search of log2(n_users) steps through the
 * offsets per kept pair to find its user, and 20 bytes of staging per kept pair, which are then sorted into one user
 * list per distinct requested item exactly as a caller's pairs are.  More than 2^32 - 1 kept pairs are refused, as for
 * a caller's list, here after that count.
 * Candidates ("the best 100 of this segment"): cand_users follows mfsgd_recommend_among's rules -- cand_ptr == NULL,
 * one list shared by every request row; otherwise CSR over the request rows (cand_ptr[0] == 0, non-decreasing,
 * cand_ptr[n] == n_cand).  Lists may be unsorted, repeat users and be empty; a list that names every user gives the
 * unrestricted call's row bit for bit; n_cand == 0 gives rows of padding without device work.  Users appended with
 * mfsgd_append_users are valid candidates; indices between count and capacity are not.
 * The _rows calls: "item b" is rows[b] (n_rows x k, dense: for instance what mfsgd_fold_in_items returned -- "who
 * should be shown this new item"); every row is answered, in order, and excl_row / cand_ptr index the rows.
 * Checks, all before any device work, in mfsgd_recommend_excluding's / mfsgd_recommend_among's order, the messages
 * starting with the call's own name ("recommend_users: ", "recommend_users_among: ", "recommend_users_unseen: ",
 * "recommend_users_unseen_among: ", "recommend_users_rows: ", "recommend_users_rows_among: "): MFSGD_ERR_INVALID_ARG for
 * a negative n or n_excl, topn < 1 or a null array that is needed ("bad argument"); then MFSGD_ERR_STATE for
 * n_parts != 1 and for "no seen set"; then MFSGD_ERR_INVALID_ARG for topn > n_users ("topn exceeds the number of
 * users"), "item X out of range" for a requested item, the candidate checks ("n_cand is negative", "cand_users is
 * null", the three cand_ptr rules, "candidate X out of range" against n_users, more than 2^32 - 1 candidates), "excluded
 * pair X out of range", more than 2^32 - 1 pairs of requested items.  Then n == 0 is MFSGD_OK.  Then MFSGD_ERR_STATE for
 * factors never initialised, set or loaded, or no Q; MFSGD_ERR_NO_DEVICE for a valid call with work to do and no usable
 * GPU.
 * Nothing in the handle is modified: not the factors, the index, its mass table, the item weights, a schedule or a
 * cached graph.  Every list and all staging is freed before return, on every path -- mfsgd_debug_device_bytes is the
 * same before and after.  mfsgd_debug_serve_seconds reports the two halves as for mfsgd_recommend; the lists half
 * covers the candidate lists, the exclusion lists and the read of the index.  Selection is mfsgd_recommend's, kernels
 * and all (csrc/recommend.hip), with P in the place of Q.
 * Not done here: ranks of users (a rank_users), a by-item index kept in the handle, multi-partition handles.          */
int mfsgd_recommend_users(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn, const int32_t* excl_u,
                          const int32_t* excl_i, int64_t n_excl, int32_t* out_users, float* out_scores);
int mfsgd_recommend_users_among(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn, const int64_t* cand_ptr,
                                const int32_t* cand_users, int64_t n_cand, const int32_t* excl_u, const int32_t* excl_i,
                                int64_t n_excl, int32_t* out_users, float* out_scores);
int mfsgd_recommend_users_unseen(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn, int32_t* out_users,
                                 float* out_scores);
int mfsgd_recommend_users_unseen_among(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn,
                                       const int64_t* cand_ptr, const int32_t* cand_users, int64_t n_cand,
                                       int32_t* out_users, float* out_scores);
int mfsgd_recommend_users_rows(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn, const int32_t* excl_row,
                               const int32_t* excl_user, int64_t n_excl, int32_t* out_users, float* out_scores);
int mfsgd_recommend_users_rows_among(mfsgd_handle* h, const float* rows, int32_t n_rows, int32_t topn,
                                     const int64_t* cand_ptr, const int32_t* cand_users, int64_t n_cand,
                                     const int32_t* excl_row, const int32_t* excl_user, int64_t n_excl, int32_t* out_users,
                                     float* out_scores);

/* ---- similar items and users: cosine nearest neighbours among the rows of Q, or of P --------------------------------
 * The arithmetic, all fp32, round to nearest even, subnormals kept, nothing contracted; dot is
 * the canonical dot, the bits mfsgd_predict() returns:
 *     n2(x)     = dot(x, x)
 *     rn(x)     = n2(x) > 0 ? 1.0f / sqrtf(n2(x)) : 0.0f      (sqrt and division each correctly rounded)
 *     cos(a, b) = (dot(a, b) * rn(a)) * rn(b)                 (a the query row, b the candidate: two roundings, in this order)
 * What follows from it: the score is not clamped -- cos(a, a) can be 1.0000001 or 0.99999994; cos(a, b) and cos(b, a)
 * may differ in the last bit; a row whose n2 is 0 (all +-0.0) has rn = 0, so as a query all its scores are zeros and its
 * neighbours are the smallest indices, and as a candidate it scores zero; a row scaled by a power of two has, barring
 * under- or overflow, bit-identical scores to the unscaled row, so the two tie exactly.  Rows whose n2 is not finite,
 * and any NaN, give unspecified ranks, as in mfsgd_rank_items.
 * Order: recommend's.  j comes before t when score(j) > score(t), or when the two compare equal as floats (-0.0 equals
 * +0.0) and j < t.  Outputs are n x topn, row-major, best first; the scores are the bits of cos above.
 * mfsgd_similar_items / _users never return the query's own index in its row: exclusion is by index, not by score, so a
 * duplicate row elsewhere stays eligible.  mfsgd_similar_rows excludes nothing.  A row with fewer than topn eligible
 * candidates is padded with index -1 and score NaN, as in mfsgd_recommend_excluding (that only happens when topn equals
 * the side's size).  A query asked for twice gets the same row twice; queries may come in any order.
 * Arguments are checked before any device work (MFSGD_ERR_INVALID_ARG, message "similar_items: ...", "similar_users:
 * ...", "similar_rows: ..." or "row_inv_norms: ..."): negative n or n_rows, topn < 1 or above the side's size, a null
 * array that is needed, an index out of range, a side other than MFSGD_SIDE_USERS / MFSGD_SIDE_ITEMS.
 * MFSGD_ERR_STATE: n_parts != 1, or factors never initialised, set or loaded.  MFSGD_ERR_NO_DEVICE: a valid call with
 * work to do and no usable GPU; there is never a CPU result.  n == 0 (n_rows == 0) is MFSGD_OK and touches nothing.
 * The model is not modified, everything allocated on the device is freed before return, and nothing is cached in the
 * handle between calls: the inverse norms are computed per call (one pass over the side, about what scoring one query
 * costs).  Selection is mfsgd_recommend's, kernels and all (csrc/recommend.hip); csrc/similar.hip adds the norms.   */
#define MFSGD_SIDE_USERS 0
#define MFSGD_SIDE_ITEMS 1
/* rn() of every row of P (side 0: n_users floats) or Q (side 1: n_items floats). */
int mfsgd_row_inv_norms(mfsgd_handle* h, int32_t side, float* out);
/* For each of the n query items the topn other items with the largest cos(Q[items[b]], Q[j]), best first. */
int mfsgd_similar_items(mfsgd_handle* h, const int32_t* items, int32_t n, int32_t topn,
                        int32_t* out_items, float* out_scores);
/* The same among users: P against P. */
int mfsgd_similar_users(mfsgd_handle* h, const int32_t* users, int32_t n, int32_t topn,
                        int32_t* out_users, float* out_scores);
/* Query vectors of the caller's (n_rows x k, dense: a folded-in user, a cold item's vector) against one side. */
int mfsgd_similar_rows(mfsgd_handle* h, int32_t side, const float* rows, int32_t n_rows, int32_t topn,
                       int32_t* out_index, float* out_scores);

/* ---- least-squares fold-in: exact rows for new users or items, implicit feedback too, and ALS ------------------------
 * With the other side fixed, the row that minimises the model's objective solves a k x k positive-definite system
 *     (sum_j a_j f_j f_j^T + alpha * F^T F + delta * I) x = sum_j b_j f_j
 * so it needs no learning rate, no epochs and no start row.  alpha = 0, a = 1, b = r, delta = lambda * len is the fixed
 * point of mfsgd_fold_in_users' chain; alpha > 0 is implicit-feedback fold-in (a = c - alpha, b = c, delta = lambda); run
 * over all users and then all items it is ALS.  The rule, bit for bit: everything fp32, round to
 * nearest even, subnormals kept, nothing contracted except the fmas written here, sqrtf and / correctly rounded.
 * F is the fixed side (n rows; Q for MFSGD_SIDE_USERS, P for MFSGD_SIDE_ITEMS), f_j = F[ids[j]], pad columns never enter;
 * j runs over row_ptr[x] .. row_ptr[x + 1] in the order given, an id that appears twice contributes two terms.
 * G = gram(F), lower triangle p >= q: tiles of T = 256 * ceil(n / 65536) rows, tile t owning rows [tT, min(n, (t+1)T));
 *     g_t[p][q] = +0.0f;  for r in the tile, ascending: g_t[p][q] = fmaf(F[r][p], F[r][q], g_t[p][q])
 *     G[p][q] = g_0[p][q];  then G[p][q] = G[p][q] + g_t[p][q] for t = 1, 2, ...;  the upper triangle a copy of the lower
 * The system of a row, lower triangle p >= q:
 *     A[p][q] = +0.0f;  rhs[p] = +0.0f
 *     for j in list order:  t = (a given ? a[j] * f_j[p] : f_j[p])        (one rounding, on the ROW index p)
 *                           A[p][q] = fmaf(t, f_j[q], A[p][q]);   rhs[p] = fmaf(b[j], f_j[p], rhs[p])
 *     if alpha != 0:        A[p][q] = fmaf(alpha, G[p][q], A[p][q])       (G is not computed when alpha == 0)
 *     dg = fmaf(ridge_per_entry, (float)len, ridge);   A[p][p] = A[p][p] + dg
 * The solve, Cholesky by columns, every inner sum a chain in ascending index:
 *     for j = 0 .. k-1:  s = A[j][j];  for t = 0 .. j-1: s = fmaf(-L[j][t], L[j][t], s)
 *                        if !(s > 0.0f): status = j + 1, the row's k floats are 0x7FC00000, stop
 *                        d = sqrtf(s);  inv[j] = 1.0f / d
 *                        for i = j+1 .. k-1:  v = A[i][j];  for t = 0 .. j-1: v = fmaf(-L[i][t], L[j][t], v);  L[i][j] = v * inv[j]
 *     forward:   for i = 0 .. k-1:  s = rhs[i];  for t = 0 .. i-1:         s = fmaf(-L[i][t], y[t], s);  y[i] = s * inv[i]
 *     backward:  for i = k-1 .. 0:  s = y[i];    for t = k-1 down to i+1:  s = fmaf(-L[t][i], x[t], s);  x[i] = s * inv[i]
 * A row with an empty list is +0.0f in all k columns with status 0, and no solve is run.  NaN and Inf propagate as the
 * arithmetic says; a NaN pivot fails the s > 0 test, so such a row is reported and never silently wrong.  A row that
 * fails its pivot is not an error of the call: the call returns MFSGD_OK and out_status (nullable, n_new) says which
 * rows failed (0, or the 1-based pivot).  The chain over a list is sequential: a very long row costs len / 4 dependent
 * matrix instructions (four rank-1 updates each) and is not split across workgroups -- orders of magnitude fewer
 * dependent steps than the SGD chain's len x epochs all the same.
 * Checked before any device work, in this order.  MFSGD_ERR_INVALID_ARG ("fold_in_solve: ..." / "gram: ..."): a side
 * other than MFSGD_SIDE_USERS / MFSGD_SIDE_ITEMS, a negative n_new, a null array that is needed (row_ptr and out_rows
 * with n_new > 0, ids and b with entries; out of mfsgd_gram), row_ptr[0] != 0, a decreasing row_ptr, an id outside the
 * fixed side under the current counts (the message names the entry), a non-finite alpha, ridge or ridge_per_entry.
 * MFSGD_ERR_STATE as mfsgd_fold_in_users reports it.  n_new == 0 is MFSGD_OK and touches nothing.
 * MFSGD_ERR_NO_DEVICE: a valid call with work to do and no usable GPU.  Nothing is written to the outputs of a call
 * that is refused.  The handle is not modified, nothing is cached between calls (G is computed per call when
 * alpha != 0) and all staging is freed on every path.  Lists go up in batches of whole rows, as in mfsgd_fold_in_users. */
/* gram(F) of P (side 0) or Q (side 1): k x k floats, row-major, symmetric. */
int mfsgd_gram(mfsgd_handle* h, int32_t side, float* out);
/* side: the side the NEW rows belong to (MFSGD_SIDE_USERS: new users, against Q).  a nullable: all 1.  out_rows n_new x k. */
int mfsgd_fold_in_solve(mfsgd_handle* h, int32_t side, int32_t n_new, const int64_t* row_ptr, const int32_t* ids,
                        const float* a, const float* b, float alpha, float ridge, float ridge_per_entry,
                        float* out_rows, int32_t* out_status);

/* ---- lr and lambda on a live model; learning-rate schedules --------------------------------------------------------
 * mfsgd_set_hyper gives the handle another lr and lambda without rebuilding anything: the two numbers sit in the
 * schedules' step entries (lr * r and the decay factor 1 - lr * lambda) and nowhere else in them, so the entries are
 * re-baked in place, on the device where they live there (csrc/rehyper.hip) and on the host where they live there.
 * Afterwards every schedule is byte for byte what mfsgd_set_ratings would have built on a handle created with the new
 * values, and everything that reads the handle's lr / lambda (training, mfsgd_fold_in_users, a later rebuild) uses
 * them.  The factors are not touched; the identity of the rating set is kept (the same triples again are still
 * recognised).  The call waits for the handle's stream first, and allocates no device memory that it does not free.
 * Before any ratings it only changes the configuration.  n_parts > 1: all partitions are rewritten; no
 * mfsgd_part_train on a caller's stream may be in flight, and every rank of a ring must make the same call (the
 * update of a rating must not depend on the rank that applies it).
 * MFSGD_ERR_INVALID_ARG ("set_hyper: ..."): a NaN.  Should the rewrite itself fail (a HIP error), the schedules are
 * dropped and mfsgd_set_ratings has to be called again.                                                              */
int mfsgd_set_hyper(mfsgd_handle* h, float lr, float lambda);
int mfsgd_get_hyper(const mfsgd_handle* h, float* lr, float* lambda);   /* either may be NULL */
/* epochs passes, epoch e at lr[e] and lambda[e] (lambda == NULL: the handle's current one throughout).
 * rmse_per_epoch nullable as in mfsgd_train.  Afterwards the handle holds the last epoch's values.  Nothing is re-baked
 * between two epochs whose pair of values is bit-identical.  Checked before any device work (MFSGD_ERR_INVALID_ARG,
 * "train_schedule: ..."): negative epochs, a null lr with epochs > 0, a NaN anywhere in the arrays.  epochs == 0 is
 * MFSGD_OK; otherwise MFSGD_ERR_STATE / MFSGD_ERR_NO_DEVICE as mfsgd_train.  A change of values inside the call is
 * mfsgd_set_hyper: should its rewrite fail, the call returns that error, the epochs before it stay applied, and the
 * handle holds the new values but no schedules (mfsgd_set_ratings again). */
int mfsgd_train_schedule(mfsgd_handle* h, int32_t epochs, const float* lr, const float* lambda, double* rmse_per_epoch);
/* Bold driver.  prev = RMSE before the first epoch (one read-only pass).  Epoch e runs at the handle's current lr,
 * reported in lr_used[e]; rmse[e] is the RMSE after it.  Then, in fp32: lr = lr * up if rmse[e] < prev (strictly),
 * else lr = lr * down (a NaN RMSE therefore shrinks).  prev = rmse[e].  Nothing is rolled back.
 * The handle keeps the lr the next epoch would use.  lr_used and rmse_per_epoch: `epochs` entries, both required.
 * MFSGD_ERR_INVALID_ARG ("bold_driver: ..."): negative epochs, up or down NaN or not above zero, a null array with
 * epochs > 0.  epochs == 0 is MFSGD_OK; otherwise MFSGD_ERR_STATE / MFSGD_ERR_NO_DEVICE as mfsgd_train.  A failed
 * rewrite between two epochs ends the call as it ends mfsgd_train_schedule: the epochs so far stay applied (lr_used
 * and rmse_per_epoch are valid up to there), the handle holds the next rate but no schedules. */
int mfsgd_train_bold_driver(mfsgd_handle* h, int32_t epochs, float up, float down, float* lr_used, double* rmse_per_epoch);

/* ---- a held-out set on the device; early stopping on its RMSE -------------------------------------------------------
 * Every RMSE above is over the ratings the model is trained on.  These calls measure pairs it is NOT trained on: the
 * error of a pair is e = r - dot(P[u], Q[i]) in fp32, the dot being the bits mfsgd_predict() returns, and the SSE is
 * the sum of (double)e * (double)e (csrc/validate.hip).  The result is a pure function of the factor bits, the pair
 * list in the order given and k: pair j is added to partial j mod 16384, each partial in ascending j, and the partials
 * are folded in one fixed order -- nothing depends on the device's size, on blocks / waves / flags or on the launch
 * path, and the same call twice gives the same 64 bits.  A NaN or Inf in a rating or a factor propagates.  Duplicate
 * pairs are allowed.  The model is not modified by the three measuring calls.
 * MFSGD_ERR_INVALID_ARG (messages "set_validation: ...", "validation_rmse: ...", "rmse_pairs: ...", "early_stop: ..."),
 * checked before any device work: negative n or max_epochs, a null array that is needed, a user or item out of range,
 * patience < 1, min_delta NaN or negative, a NaN in lr / lambda, null epochs_run / best_epoch.  MFSGD_ERR_STATE:
 * n_parts != 1; factors never initialised, set or loaded (for the calls that read them); no ratings, or an empty
 * validation set, for mfsgd_train_early_stop with max_epochs > 0.  MFSGD_ERR_NO_DEVICE: a valid compute call without a
 * usable GPU; there is never a CPU result.  max_epochs == 0 and mfsgd_rmse_pairs with n == 0 are MFSGD_OK and touch
 * nothing.
 *
 * The held-out set of a handle: n pairs, copied; replaces an earlier one; n == 0 (pointers may be NULL) clears it and
 * frees its device memory.  Host-only: works without a GPU, touches no schedule and no factor, survives
 * mfsgd_set_ratings / mfsgd_set_hyper / mfsgd_load_factors.  The pairs go to the device at the first call that needs
 * them there and the host copy is dropped then. */
int mfsgd_set_validation(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, int64_t n);
int mfsgd_validation_size(const mfsgd_handle* h, int64_t* n);
/* RMSE (and, nullable, the SSE) of the held-out set under the current factors; an empty set gives 0.0 like mfsgd_rmse. */
int mfsgd_validation_rmse(mfsgd_handle* h, double* rmse, double* sse);
/* The same for pairs of the caller's, nothing kept: uploaded in pieces of bounded size (2^20 pairs), freed before
 * return.  The SSE is the fp64 sum of the pieces' SSEs in order.  For a list that fits in one piece this is bit for bit
 * what mfsgd_validation_rmse gives after mfsgd_set_validation of the same arrays. */
int mfsgd_rmse_pairs(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, int64_t n, double* rmse, double* sse);
/* Train until the held-out RMSE stops improving.  The rule, in full:
 *     best = +inf, best_epoch = -1, bad = 0
 *     for e = 0 .. max_epochs - 1:
 *         train one epoch, at lr[e] / lambda[e] where given (re-baked as by mfsgd_set_hyper only when the pair of values
 *             changes, as in mfsgd_train_schedule; a null array: the handle's current value throughout)
 *         train_rmse[e] = RMSE over the training ratings, if asked for
 *         v = val_rmse[e] = RMSE of the held-out set
 *         if v < best - min_delta:   (a NaN compares false; the first finite v always improves on +inf)
 *             best = v, best_epoch = e, bad = 0; with restore_best, P and Q are copied to a snapshot on the device
 *         else: bad = bad + 1; stop when bad >= patience
 * *epochs_run = epochs trained; entries of val_rmse / train_rmse beyond that are untouched.  Afterwards, if
 * restore_best, best_epoch >= 0 and best_epoch != epochs_run - 1, the snapshot is copied back: the factors are exactly
 * those after epoch best_epoch.  With best_epoch == -1 (no finite improvement) they stay as trained.  The handle keeps
 * the lr / lambda of the last epoch run.  The snapshot (device to device, on the handle's stream; allocated only with
 * restore_best) is freed before the call returns, on every path.  A failed re-bake ends the call as it ends
 * mfsgd_train_schedule: the epochs so far stay applied (*epochs_run, val_rmse and train_rmse are valid up to there),
 * nothing is restored, the handle holds the new values but no schedules. */
int mfsgd_train_early_stop(mfsgd_handle* h, int32_t max_epochs, int32_t patience, double min_delta, int32_t restore_best,
                           const float* lr, const float* lambda,          /* nullable, max_epochs entries: as mfsgd_train_schedule */
                           double* val_rmse,                              /* required when max_epochs > 0 */
                           double* train_rmse,                            /* nullable: one extra training-set pass per epoch */
                           int32_t* epochs_run, int32_t* best_epoch);     /* both required */

/* ---- online updates: fresh ratings of users and items the model already has, applied in the order given --------------
 * mfsgd_apply_ratings applies (u[j], i[j], r[j]), j = 0 .. n - 1, to the live P and Q on the device, each with the whole
 * canonical update at the handle's current lr and lambda:
 *     p = P[u[j]], q = Q[i[j]];  d = dot(p, q);  e = r[j] - d;  s = fma(-lr, d, lr * r[j]);  c = 1 - lr * lambda
 *     P[u[j]][f] = fma(s, q[f], c * p[f]);  Q[i[j]][f] = fma(s, p[f], c * q[f])        (both from the old p and q)
 * Afterwards P and Q are bit for bit what the CPU oracle's sequential loop over the list gives, and err (nullable, n
 * floats) holds e of every rating: its error under the rows as they were just before it -- "test, then train".
 * Duplicate pairs are allowed and give two steps.  A NaN or Inf in a rating or a factor propagates as the arithmetic says.
 * How it runs in parallel ("Online updates"): the list is cut into consecutive pieces of at most 2^20 ratings,
 * applied one after the other.  Within a piece, level[j] = 0 if no earlier rating of the piece has u[j] or i[j], else
 * 1 + the larger level of the latest earlier rating with the same user and of the latest with the same item.  The
 * ratings of one level share no row and run at once; the levels run in ascending order.  mfsgd_online_levels returns
 * those levels (host only: it works without a GPU, without ratings and without factors; `level` nullable, n entries,
 * each relative to its rating's piece).
 * What a call costs: one pass over the list on the host (levels, a counting sort), 16 bytes per rating up and 4 down,
 * and one kernel launch per level that holds more ratings than one workgroup takes in a pass (256 / group_lanes) plus one
 * per run of consecutive levels that do not; a piece has at least as many levels as its most frequent user or item has
 * ratings in it, and those launches, about 5 us each, dominate: at the MovieLens-20M shape and k = 64 a batch of 2^10
 * ratings takes 0.10 ms, 2^16 ratings 1.0 ms and 2^20 ratings (3 568 levels, 3 475 launches) 22 ms ("Online
 * updates").
 * Arguments are checked before any device work (MFSGD_ERR_INVALID_ARG, message "apply_ratings: ..." / "online_levels:
 * ..."): a negative n, a null array that is needed, a user or item out of range (the message names the rating); a
 * failed check leaves the factors untouched.  MFSGD_ERR_STATE (mfsgd_apply_ratings, whatever n is): n_parts != 1,
 * factors never initialised, set or loaded, or no Q (after mfsgd_init_p_offset).  MFSGD_ERR_NO_DEVICE: a valid call with
 * n > 0 and no usable GPU; there is never a CPU result.  n == 0 is MFSGD_OK and touches nothing.
 * The call needs no stored rating set (a model loaded from a factor file can be updated), runs on the handle's stream
 * and blocks until the device is idle.  Its device buffers are sized by the largest piece and freed before it returns,
 * on every path.  It leaves as they were: the stored ratings and their identity (the same triples again are still
 * recognised), every schedule and cached training graph, the held-out set.  Everything that reads the factors
 * afterwards (training, RMSE, predict, recommend, mfsgd_validation_rmse, ...) sees the updated rows.  Should a HIP call
 * fail between two pieces, the pieces before it stay applied.                                                         */
typedef struct mfsgd_online_info {
    int64_t n, pieces;
    int64_t levels;      /* sum of the pieces' level counts                   */
    int64_t max_width;   /* ratings in the widest level                       */
    int64_t launches;    /* kernel launches made (0 from mfsgd_online_levels) */
} mfsgd_online_info;
int mfsgd_online_levels(mfsgd_handle* h, const int32_t* u, const int32_t* i, int64_t n,
                        int32_t* level /* nullable */, mfsgd_online_info* info /* nullable */);
int mfsgd_apply_ratings(mfsgd_handle* h, const int32_t* u, const int32_t* i, const float* r, int64_t n,
                        float* err /* nullable */, mfsgd_online_info* info /* nullable */);

/* ---- pairwise ranking (BPR): (user, positive item, negative item) triples applied in the order given ------------------
 * mfsgd_apply_triples applies (u[x], i[x], j[x]), x = 0 .. n - 1, to the live P and Q on the device, each with one step
 * of Bayesian personalised ranking at the handle's current lr and lambda.  Everything is fp32,
 * round to nearest even, subnormals kept, nothing contracted except the fmas written here; dot is the canonical dot, the
 * bits mfsgd_predict returns.  With p = P[u[x]], qi = Q[i[x]], qj = Q[j[x]], all three read before anything is written:
 *     x  = dot(p, qi) - dot(p, qj)                    the margin before the update
 *     g  = lsig(x)                                    = 1 / (1 + e^x) = sigma(-x)
 *     s  = lr * g;   c = 1 - lr * lambda
 *     P[u][f] = fma( s, qi[f] - qj[f], c * p[f])
 *     Q[i][f] = fma( s, p[f],          c * qi[f])
 *     Q[j][f] = fma(-s, p[f],          c * qj[f])
 * lsig is a pure function of the bits of x:
 *     x is NaN:  g = 0x7FC00000
 *     t  = x > 80 ? 80 : (x < -80 ? -80 : x)
 *     n  = rintf(t * 0x3FB8AA3B)                      1.44269502f, ties to even
 *     r  = fma(n, -0.693359375f, t);  r = fma(n, 2.12194440e-4f, r)
 *     q  = 1.9875691500e-4f
 *     q  = fma(q, r, 1.3981999507e-3f); q = fma(q, r, 8.3334519073e-3f); q = fma(q, r, 4.1665795894e-2f)
 *     q  = fma(q, r, 1.6666665459e-1f); q = fma(q, r, 5.0000001201e-1f)
 *     e  = fma(q, r * r, r) + 1.0f
 *     y  = e * (the float whose bits are (int(n) + 127) << 23)      exact: |n| <= 116
 *     g  = 1.0f / (1.0f + y)                          addition and division each correctly rounded
 * (within 2.48 ulp of 1 / (1 + exp(t)) and never increasing in x: DESIGN.md.)  mfsgd_bpr_weights computes g[a] =
 * lsig(x[a]) on the host with the function the kernel compiles: it has no handle and needs no GPU (messages through
 * mfsgd_last_error(NULL), "bpr_weights: ...": a negative n, a null array with n > 0).
 * Afterwards P and Q are bit for bit the sequential loop above over the list, and margin (nullable, n floats) holds x of
 * every triple: its margin under the rows as they were just before it.  Duplicate triples are allowed and give two steps.
 * A NaN or Inf in a factor propagates as the arithmetic says.
 * How it runs in parallel is mfsgd_apply_ratings' way with three rows per step: pieces of at most 2^20 consecutive
 * triples, one after the other; within a piece level[x] = 0 if no earlier triple of the piece has user u[x], or has i[x]
 * or j[x] in EITHER item position, else 1 + the largest level among the latest earlier triple with that user, the latest
 * with i[x] as either item and the latest with j[x] as either item.  mfsgd_triple_levels returns those levels (host
 * only: no GPU, no ratings, no factors; `level` nullable, n entries, each relative to its triple's piece).  Launches are
 * counted as for ratings: one per level wider than a workgroup pass, one per run of narrower ones.  Per piece 16 bytes
 * per triple and 4 per level go up (at most 20 per triple), and 4 per triple come down if margins are asked for.
 * Checks, all before any device work, in this order.  MFSGD_ERR_INVALID_ARG ("apply_triples: ..." / "triple_levels:
 * ..."): a negative n; a null array with n > 0; a user or item out of range under the current counts (the message names
 * the triple); i[x] == j[x] (the message names the triple).  Then, mfsgd_apply_triples whatever n is, MFSGD_ERR_STATE as
 * mfsgd_apply_ratings reports it: n_parts != 1, factors never initialised, no Q.  n == 0 is MFSGD_OK and touches
 * nothing.  MFSGD_ERR_NO_DEVICE: a valid call with n > 0 and no usable GPU; there is never a CPU result.  A failed
 * check leaves the factors untouched.
 * The device buffers are sized by the largest piece and freed before the call returns, on every path.  The call leaves
 * as they were: the stored ratings and their identity, every schedule and cached training graph, the held-out set and
 * the seen-item index.  Should a HIP call fail between two pieces, the pieces before it stay applied.                  */
int mfsgd_triple_levels(mfsgd_handle* h, const int32_t* u, const int32_t* i, const int32_t* j, int64_t n,
                        int32_t* level /* nullable */, mfsgd_online_info* info /* nullable */);
int mfsgd_apply_triples(mfsgd_handle* h, const int32_t* u, const int32_t* i, const int32_t* j, int64_t n,
                        float* margin /* nullable */, mfsgd_online_info* info /* nullable */);
int mfsgd_bpr_weights(const float* x, float* g, int64_t n);
/* mfsgd_apply_triples_weighted is mfsgd_apply_triples with one line of the step replaced: the step size of triple x is
 *     s = lr * w[x]                                   one fp32 multiply, at the handle's current lr
 * and lsig is not evaluated; c, the three fmas, the pad columns (+0.0), the margin x = dot(p, qi) - dot(p, qj) returned in
 * `margin`, the pieces of 2^20, the levels (exactly mfsgd_triple_levels: weights do not enter), the launches, `info`,
 * what the call leaves untouched and the state and device errors are mfsgd_apply_triples' own code.  w[x] =
 * mfsgd_bpr_weights of the margins reproduces mfsgd_apply_triples on triples that share no row; importance weights,
 * LambdaRank-style weights, hinge losses and WARP (below) are host policy on top of it.  Zero, negative and infinite
 * weights are plain arithmetic; a NaN weight becomes 0x7FC00000 at the door (see "factors" above) and makes the k
 * columns of its three rows NaN.  At most 4 more bytes per triple go up.  Checks: mfsgd_apply_triples' in its order
 * ("apply_triples_weighted: ..."), w being one of the arrays that must not be null when n > 0.
 * mfsgd_warp_weights is the weight of a WARP step for the rank mfsgd_sample_unseen_violating estimated: w[a] = L(rank[a]),
 * L(0) = 0 and L(r) = (float)(1.0/1 + 1.0/2 + ... + 1.0/r) for r > 0, the sum in fp64, added in ascending order and
 * rounded to fp32 once (Weston's harmonic weight).  Host only: no handle, no GPU; one prefix table up to the largest rank
 * of the call, not O(rank) per element.  MFSGD_ERR_INVALID_ARG (message through mfsgd_last_error(NULL), "warp_weights:
 * ..."): a negative n, a null array with n > 0, a negative rank (the message names the entry; w is untouched).          */
int mfsgd_apply_triples_weighted(mfsgd_handle* h, const int32_t* u, const int32_t* i, const int32_t* j, const float* w,
                                 int64_t n, float* margin /* nullable */, mfsgd_online_info* info /* nullable */);
int mfsgd_warp_weights(const int32_t* rank, float* w, int64_t n);

/* ---- growing a live model: rows appended to P and Q in place -----------------------------------------------------------
 * mfsgd_append_users / mfsgd_append_items give the model n_new more users / items: the new rows take the indices
 * old_count .. old_count + n_new - 1, and *first (nullable) receives old_count.  rows: n_new x k, dense -- for instance
 * what mfsgd_fold_in_users / mfsgd_fold_in_items returned; every NaN in it becomes 0x7FC00000, as in mfsgd_set_factors.
 * rows == NULL: element f of new row x is draw x * k + f of java.util.Random(seed), nextFloat() * (float)(1/sqrt(k)):
 * the start rows of a fold-in without init_rows.  The pad columns k .. kp - 1 of a new row are zero.
 * Where the rows go: with the factors on host staging (no GPU needed) the staging grows; with the factors on the
 * device everything happens there -- the caller's rows go up through a bounded staging buffer (freed before return)
 * and a kernel pads them into place (csrc/grow.hip), seeded rows are drawn in place, and no old row crosses PCIe.
 * What changes: the counts, for everything that reads them -- mfsgd_get_dims, mfsgd_get_factors, mfsgd_save_factors,
 * the range checks and scan lengths of predict, recommend, rank, similar, fold-in, validation, online updates and
 * mfsgd_set_ratings, the early-stop snapshot.  What does not: the stored ratings and their identity (the same triples
 * again are still recognised, nothing is rebuilt), every schedule and mfsgd_get_order, the held-out set, lr and lambda,
 * the bits of the old rows.  Training afterwards runs the same schedule in the same order -- the order
 * mfsgd_get_order returns -- and does not touch the new rows, which have no ratings.  A fresh handle created at the
 * grown size may cut its blocks differently: the grown handle is NOT byte-equal to such a build, it is equal to the
 * oracle run over its own order.  A later mfsgd_set_ratings with other triples may name the new indices and builds a
 * schedule for the grown sizes as usual.
 * Capacity: a handle has a capacity per side, at least its count and equal to it until mfsgd_reserve_rows asks for
 * more; the device buffers hold capacity x kp floats, and rows from the count on are never read and never observable.
 * Without a reserve call device memory use is exactly what it is without these calls.  mfsgd_reserve_rows raises a
 * capacity to at least the value given and never shrinks it (a value at or below the current capacity, 0 included,
 * leaves that side alone).  It works in every factor state: before the factors are on the device it records the
 * number, and they are allocated with it when they get there; with the factors on the device it reallocates now.
 * Re-seeding or replacing the factors keeps the capacity.
 * An append that fits the capacity writes the new rows in place: P and Q keep their addresses, so the cached training
 * graphs, which hold those addresses (and nothing that derives from the counts), stay valid and the next mfsgd_train
 * replays them.  An append beyond the capacity reallocates that side to exactly max(count + n_new, reserve): it waits
 * for the handle's stream, allocates the new buffer, copies the old rows device to device, writes the new ones,
 * synchronises, drops the training graphs (they hold the dead pointer; the next mfsgd_train captures again) and frees
 * the old buffer.  The new buffer is allocated BEFORE the old one is released: peak device use during a reallocating
 * append (or reserve) is old + new, and a failed allocation is MFSGD_ERR_OOM with the model exactly as it was.  Growth
 * policy beyond the reserve is the caller's: the library never over-allocates on its own.
 * Checks, in this order.  MFSGD_ERR_INVALID_ARG ("append_users: ..." / "append_items: ..." / "reserve_rows: ..."): a
 * negative n_new or capacity, a count that would exceed INT32_MAX.  MFSGD_ERR_STATE: n_parts != 1; for the appends also
 * factors never initialised, set or loaded, or no Q (after mfsgd_init_p_offset).  n_new == 0 is MFSGD_OK and touches
 * nothing; *first is still set.                                                                                      */
int mfsgd_append_users(mfsgd_handle* h, int32_t n_new, const float* rows /* nullable */, int64_t seed, int32_t* first /* nullable */);
int mfsgd_append_items(mfsgd_handle* h, int32_t n_new, const float* rows /* nullable */, int64_t seed, int32_t* first /* nullable */);
int mfsgd_reserve_rows(mfsgd_handle* h, int32_t user_capacity, int32_t item_capacity);
int mfsgd_get_capacity(const mfsgd_handle* h, int32_t* users, int32_t* items);   /* either may be NULL */

/* Timed variant used by bench.py: runs `epochs` training passes bracketed by
 * HIP events on the handle's stream and returns the elapsed device time and
 * the number of sgd-round kernel launches inside it.  No RMSE pass.          */
int mfsgd_train_timed(mfsgd_handle* h, int32_t epochs, double* elapsed_ms, int64_t* launches);

/* ---- data formats either side of the path (host; csrc/io.cpp) ----------------
 * Rating files of the datasets the configs are shaped after.  Ids in the file are
 * arbitrary: they are compacted to dense indices (rank among the distinct ids,
 * ascending); the original ids are returned as tables.  Errors of these functions
 * are reported by mfsgd_io_last_error() (they have no handle).                   */
#define MFSGD_FMT_AUTO 0
#define MFSGD_FMT_ML_TSV 1  /* MovieLens-100K u.data: user \t item \t rating \t timestamp   */
#define MFSGD_FMT_ML_DAT 2  /* MovieLens-1M/10M ratings.dat: user::movie::rating::time   */
#define MFSGD_FMT_ML_CSV 3  /* MovieLens-20M/25M ratings.csv: userId,movieId,rating,time */
#define MFSGD_FMT_NETFLIX 4 /* Netflix Prize: "movieId:" then "customerId,rating,date"   */
typedef struct mfsgd_ratings_file mfsgd_ratings_file;
int mfsgd_ratings_file_open(const char* path, int32_t format, mfsgd_ratings_file** out);
int mfsgd_ratings_file_info(const mfsgd_ratings_file* f, int64_t* nnz, int32_t* n_users, int32_t* n_items);
/* Any pointer may be NULL.  u, i, r: nnz entries; user_ids / item_ids: n_users / n_items. */
int mfsgd_ratings_file_read(const mfsgd_ratings_file* f, int32_t* u, int32_t* i, float* r,
                            int64_t* user_ids, int64_t* item_ids);
void mfsgd_ratings_file_close(mfsgd_ratings_file* f);
const char* mfsgd_io_last_error(void);
/* Factor files: "MFSGDF01", int32 U, I, k, 0, then P (U x k) and Q (I x k), fp32 little endian. */
int mfsgd_get_dims(const mfsgd_handle* h, int32_t* n_users, int32_t* n_items, int32_t* k);
int mfsgd_save_factors(mfsgd_handle* h, const char* path);
int mfsgd_load_factors(mfsgd_handle* h, const char* path);

/* ---- schedule introspection (host) ---------------------------------------- */
int mfsgd_get_schedule_info(const mfsgd_handle* h, int32_t part, mfsgd_schedule_info* out);
/* Canonical sequential order of partition `part`: order[j] is the index (into
 * the arrays given to set_ratings) of the j-th rating; length = info.nnz.
 * cell_ptr has rounds*blocks+1 entries: cell b of round rd covers
 * order[cell_ptr[rd*blocks+b] .. cell_ptr[rd*blocks+b+1]).                    */
int mfsgd_get_order(const mfsgd_handle* h, int32_t part, int64_t* order, int64_t* cell_ptr);

/* Diagnostic (not part of the Java surface): the device-facing schedule arrays of a
 * partition, so that tests can replay the kernel's exact LDS access order on the CPU.
 * cells: n_cells x 8 words {row_off, ent_off, n_steps, nu | ni << 16, next chunk, flags, 2 reserved} (flags bit 0:
 * the cell's tile is ONE item row in every cell -- it is handed on through the tile's mailbox): chunk
 * descriptors -- the first blocks*blocks are the first chunk of each cell, a cell too large for
 * the LDS continues through `next` (0 = last chunk) into the descriptors behind them;
 * subs: n_subs x 2 words {off | solo steps << 16, general steps | run steps << 16};
 * entries: n_entries x 4 words {p addr | q addr << 16 | flag << 31 (16-byte units), rating bits,
 * bits of lr*rating, bits of the slot's decay factor}.  A sub-cell's solo run follows its run steps
 * and two idle steps (padded to whole steps): header {slots_0, 0, 0, 0}, then per step {slots of the NEXT step,
 * 0xFFFFFFFF (mailbox), bits of lr*rating, rating bits}, then a terminator; the slots behind the last step
 * address an all-zero row.                                                                      */
int mfsgd_debug_schedule_sizes(const mfsgd_handle* h, int32_t part, int64_t* n_cells, int64_t* n_rows,
                               int64_t* n_subs, int64_t* n_entries);
int mfsgd_debug_get_schedule(const mfsgd_handle* h, int32_t part, uint32_t* cells, uint32_t* rows,
                             uint32_t* subs, uint32_t* entries);

/* Diagnostic (not part of the Java surface): runs ONE epoch with the persistent kernel and
 * returns, per workgroup, 16 words: shader cycles wave 0 spent in (0) draining its previous
 * stores and issuing prefetch + own-row gather, (1) waiting for the tile, (2) the barrier after
 * it, (3) the tile gather, (4) the ratings, (5) storing + publishing the tile, (6) storing its
 * own rows; (7) the longest single ratings phase (its slowest cell); (8..14) the seven phases of
 * the pass that contained it; (15) unused.  out must hold blocks x 16 words.  It DOES apply the epoch. */
int mfsgd_debug_epoch_profile(mfsgd_handle* h, uint64_t* out, int32_t* n_workgroups);

/* Diagnostic: out4 = {times a persistent launch found its workgroups not co-resident and the library
 * switched that partition to round launches, partitions currently on the persistent kernel, cached
 * training graphs, schedule builds: mfsgd_set_ratings calls that did not find the same triples
 * already in place}.                                                                              */
int mfsgd_debug_counters(const mfsgd_handle* h, int64_t* out4);

/* Diagnostic (not part of the Java surface): *live = bytes of device memory the library holds in this process
 * right now, over all handles (it takes none: the count is process-wide).  Memory a caller owns (the Q blocks
 * handed to mfsgd_part_train) is not in it.  Tests compare it before and after a call, or a handle's whole
 * life, to see that nothing was kept: free-memory readings of a shared GPU cannot tell.                     */
int mfsgd_debug_device_bytes(int64_t* live);

/* Diagnostic (not part of the Java surface): out2 = host seconds the handle's latest recommend call (any of the
 * mfsgd_recommend* calls) spent in its two device halves, each measured up to its synchronise: {building the candidate
 * and exclusion lists (upload, sort, unique), scoring and selecting (output download included)}.  The argument checks
 * and the upload of rows come before both and are in neither.  tools/among_bench.py reports them apart.            */
int mfsgd_debug_serve_seconds(mfsgd_handle* h, double* out2);

/* Diagnostic (not part of the Java surface): occupies the LDS of all but four CUs for `milliseconds` (<= 5000)
 * with a spinning kernel on a side stream, asynchronously -- what a foreign kernel sharing the GPU
 * looks like to the persistent epoch kernel.  Tests use it to force the "workgroups not co-resident"
 * path: the epoch kernel gives up before touching anything and the epoch runs as round launches. */
int mfsgd_debug_occupy(mfsgd_handle* h, int32_t milliseconds);

/* Diagnostic (not part of the Java surface): runs training round `round` once with
 * phase stamps; out receives blocks x 6 values per workgroup: shader-clock at
 * start, after gather, after the rating steps, after scatter, then the 100 MHz
 * constant clock at start and at end; after those blocks x 6 words follow
 * blocks x W x W x 4 words: per (wave, sub-round) cycles in the general loop,
 * cycles in the run loop, general steps, run steps.  It DOES apply
 * that round's updates.  Single-partition handles only.                        */
int mfsgd_debug_round_stamps(mfsgd_handle* h, int32_t part, int32_t round, uint64_t* out);

/* ---- DSGD building blocks (n_parts > 1) ------------------------------------
 * The global partitioner (host, no GPU): ONE rating set over n_users x n_items is cut for
 * n_parts devices -- users into n_parts contiguous ranges balanced by rating count (device g
 * holds the P rows of users [user_begin[g], user_begin[g+1]) and those users' ratings), items
 * into n_parts partitions balanced by rating count (longest-processing-time-first; items nobody
 * rated are dealt out to even the row counts).  A pure function of the two degree arrays, so
 * every rank computes the same plan from the same degrees (a rank that only sees its own ratings
 * all-reduces the item histogram first).  user_begin: n_parts + 1 entries; item_part: n_items.  */
int mfsgd_dsgd_plan(const int64_t* deg_user, const int64_t* deg_item, int32_t n_users, int32_t n_items,
                    int32_t n_parts, int32_t* user_begin, int32_t* item_part);
/* The same for a job of `world` ranks holding `parts_per_rank` item partitions at a time, at rank k: user_begin has
 * world + 1 entries, item_part n_items entries in [0, world * parts_per_rank).
 * chain_crit = 0: items dealt longest-processing-time-first by rating count -- the heaviest items end up one per
 * partition, the partitions take the same time, and the ring's epoch (world x the slowest partition: a Q block is
 * trained by one rank after the other) is as short as the heaviest item's own chain allows.  This is what
 * mfsgd_dsgd_plan does and what a ring of GPUs wants.
 * chain_crit > 0 (e.g. 0.3): CHAIN-AWARE -- the chain-critical items (those whose chain of dependent updates on one
 * rank reaches chain_crit of a work-bound sub-epoch) are packed, heaviest together, into as few partitions as the
 * rating-count balance allows, the rest dealt LPT over the others.  That minimises the SUM over the partitions of
 * their heaviest items' chains -- what ONE device pays when it runs the partitions back to back (virtual devices) --
 * at the price of unequal partition times (measured: DESIGN.md section 6); not for a ring.
 * info4 (nullable): {sum over the partitions of their heaviest item's rating count, chain-critical items,
 * partitions filled sequentially, the threshold}.   Java: MatrixFactorizationSGD.plan(degUser, degItem, nParts). */
int mfsgd_dsgd_plan_ex(const int64_t* deg_user, const int64_t* deg_item, int32_t n_users, int32_t n_items,
                       int32_t world, int32_t parts_per_rank, int32_t k, float chain_crit, int32_t* user_begin,
                       int32_t* item_part, int64_t* info4);
/* Installs an item -> partition map (n_items entries in [0, n_parts)) on a handle with
 * n_parts > 1, before mfsgd_set_ratings; item i is then row (number of smaller item ids in the
 * same partition) of that partition's Q block.  NULL restores the default below.            */
int mfsgd_set_item_partition(mfsgd_handle* h, const int32_t* item_part);
/* The map in force: partition and block row of every item (either pointer may be NULL). */
int mfsgd_get_item_partition(const mfsgd_handle* h, int32_t* item_part, int32_t* item_row);
/* Default map: item i belongs to partition i % n_parts and is row i / n_parts of that
 * partition's Q block.  A Q block is a caller-owned DEVICE buffer of
 * mfsgd_part_rows() x kp floats (kp from schedule_info), so that the host side
 * can move it between GPUs (RCCL send/recv) without this library knowing.
 * `stream` is the hipStream_t the caller orders its use of the block on; it is
 * used as given (NULL = HIP's null stream, which is what torch's default stream
 * is), never replaced by a private stream.                                     */
int mfsgd_part_rows(const mfsgd_handle* h, int32_t part, int32_t* rows);
/* Fill a HOST buffer (rows x kp, zero padded) with the initial values the
 * single-device init would give these items for this seed and this U:
 * the stream position of Q row i is (U_total + i) * k.                        */
int mfsgd_part_init_q(const mfsgd_handle* h, int32_t part, int64_t seed, int64_t u_total,
                      float* q_block_host);
/* One DSGD sub-epoch: every rating of this handle's users whose item is in
 * `part`, against q_block_dev.  Asynchronous on `stream`.  Calls for different
 * partitions of ONE handle must not overlap in time: they update the same P rows.
 * The block is the caller's memory and is used as it is: a NaN in it must not
 * have all of its low 22 mantissa bits set (0x7FFFFFFF, 0xFFFFFFFF, 0x7FBFFFFF,
 * 0xFFBFFFFF: a buffer filled with 0xFF bytes is the usual source).  Such a row
 * in a long chain makes the launch give up ("timed out waiting for a tile
 * hand-off", MFSGD_ERR_HIP at the next check, factors invalid).  Blocks that
 * came from mfsgd_part_init_q, mfsgd_dsgd_set_q or a kernel of this library
 * never hold one: the library's own NaNs are 0x7FC00000 / 0xFFC00000.          */
int mfsgd_part_train(mfsgd_handle* h, int32_t part, float* q_block_dev, void* stream);
/* Sum of squared errors of the same ratings (fp64), synchronous. */
int mfsgd_part_sse(mfsgd_handle* h, int32_t part, const float* q_block_dev, void* stream,
                   double* sse);
/* Seeds P when this handle holds users [u_offset, u_offset + n_users) of a
 * larger problem: stream position of P row u is (u_offset + u) * k.  It seeds
 * P alone: on a single-partition handle the handle's own Q is gone afterwards,
 * and every call that reads it (training, RMSE, predict, recommend, rank,
 * similar items, fold-in, the held-out measures, mfsgd_get_factors with a Q)
 * is MFSGD_ERR_STATE until mfsgd_init_factors, mfsgd_set_factors or
 * mfsgd_load_factors; the mfsgd_part_* calls with a caller-owned block,
 * mfsgd_similar_users and mfsgd_get_factors(P, NULL) go on working.           */
int mfsgd_init_p_offset(mfsgd_handle* h, int64_t seed, int64_t u_offset);
/* The recovery point of an asynchronous sub-epoch: waits for `stream`; if the LAST mfsgd_part_train of this
 * partition found its persistent launch not co-resident (another kernel held CUs; the launch then changed
 * nothing), the sub-epoch is trained now, as one launch per round on the same stream, and waited for;
 * *rerun (nullable) = 1 then and the partition stays on round launches.  Call it with the same block
 * BEFORE the block is passed on; csrc/dsgd.cpp does so where an exchange may share the GPU with training. */
int mfsgd_part_settle(mfsgd_handle* h, int32_t part, float* q_block_dev, void* stream, int32_t* rerun);
/* Waits for `stream` and reports whether a training launch of this partition gave up on a
 * hand-off since the last check (MFSGD_ERR_HIP then: the factors are invalid).  mfsgd_part_train
 * is asynchronous and cannot report that itself.                                             */
int mfsgd_part_sync(mfsgd_handle* h, int32_t part, void* stream);
/* Partition count, padded row length (floats) and device ordinal of a handle. */
int mfsgd_get_parts(const mfsgd_handle* h, int32_t* n_parts, int32_t* kp, int32_t* device);

/* ---- DSGD driver: the ring under the C-ABI (csrc/dsgd.cpp) -----------------------------------
 * One process per GPU.  Each rank creates a handle with n_parts = world * m (m >= 1 partitions held
 * at a time), installs the item map (mfsgd_set_item_partition) if it uses a plan, gives it ITS
 * users' ratings and seeds P (mfsgd_init_p_offset); then
 *     rank 0: mfsgd_dsgd_unique_id(id);  every rank receives the same 128 bytes (any transport)
 *     mfsgd_dsgd_create(h, rank, world, id, &d)   -- collective (ncclCommInitRank)
 *     mfsgd_dsgd_init_q(d, seed, u_total)         -- seeds the Q blocks this rank holds first
 *     mfsgd_dsgd_train(d, epochs, rmse)           -- collective
 * An epoch is `world` sub-epochs: train the m partitions of the group held (one after another:
 * they share this rank's users), pass each block to rank - 1 as soon as ITS training has finished
 * and receive the next one from rank + 1: ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on
 * a communication stream, ordered against the compute stream with events, no host
 * synchronisation inside an epoch.  RCCL is bound at run time (librccl.so.1, or
 * MFSGD_RCCL_LIBRARY); without it these calls return MFSGD_ERR_UNSUPPORTED.
 * Rehearsal on one GPU: if MFSGD_DSGD_TRANSPORT=shm is set when mfsgd_dsgd_unique_id runs, the id
 * names a POSIX shared-memory segment and the ranks (processes of one host) move the blocks
 * through it instead of RCCL -- same results, host-copy speed, for testing a host's multi-process
 * logic where RCCL cannot run (two ranks on one GPU).
 * Java: MatrixFactorizationSGD.trainDistributed(...).               */
typedef struct mfsgd_dsgd mfsgd_dsgd;
#define MFSGD_DSGD_ID_BYTES 128
int mfsgd_dsgd_unique_id(void* id_out /* MFSGD_DSGD_ID_BYTES */);
int mfsgd_dsgd_create(mfsgd_handle* h, int32_t rank, int32_t world, const void* id, mfsgd_dsgd** out);
void mfsgd_dsgd_destroy(mfsgd_dsgd* d);
/* d == NULL: message of the last failed mfsgd_dsgd_create / mfsgd_dsgd_unique_id on this thread. */
const char* mfsgd_dsgd_last_error(const mfsgd_dsgd* d);
/* Seeds the blocks of the group this rank holds first (partitions rank*m .. rank*m + m - 1) as
 * the single-device init would: stream position of Q row i is (u_total + i) * k.             */
int mfsgd_dsgd_init_q(mfsgd_dsgd* d, int64_t seed, int64_t u_total);
/* Slot j (0 <= j < m) of the group currently held -- between epochs that is the home group:
 * dense rows x k host arrays, rows = mfsgd_part_rows of that partition.                      */
int mfsgd_dsgd_set_q(mfsgd_dsgd* d, int32_t j, const float* block_host);
int mfsgd_dsgd_get_q(mfsgd_dsgd* d, int32_t j, int32_t* part, int32_t* rows, float* block_host);
/* `epochs` DSGD epochs; rmse_per_epoch (nullable) receives the global RMSE after each (one
 * read-only rotation and a 2-double all-reduce).  Blocks until the device is idle.           */
int mfsgd_dsgd_train(mfsgd_dsgd* d, int32_t epochs, double* rmse_per_epoch);
int mfsgd_dsgd_rmse(mfsgd_dsgd* d, double* out);
/* bench.py: `epochs` epochs bracketed by HIP events on the compute stream (the last blocks'
 * arrival included); no RMSE pass.                                                            */
int mfsgd_dsgd_train_timed(mfsgd_dsgd* d, int32_t epochs, double* elapsed_ms);
/* All-reduce of two doubles over the ranks (op 0 = sum, 1 = max): what a host needs for global
 * counts and max-over-ranks timings without a second communication library.                  */
int mfsgd_dsgd_allreduce(mfsgd_dsgd* d, double* values2, int32_t op);
/* Counters of this rank's ring since mfsgd_dsgd_create: out4 = {sub-epoch trainings enqueued, of those run with
 * the recovery point (mfsgd_part_settle before the block leaves), of those re-run as round launches because the
 * persistent launch was not co-resident, bytes sent}.                                                         */
int mfsgd_dsgd_stats(const mfsgd_dsgd* d, int64_t* out4);

#ifdef __cplusplus
}
#endif
#endif
