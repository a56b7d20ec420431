"""Inputs and references shared by the edge tests (tests/test_contract_edges_*.py, tests/test_serving_edges_gpu.py):
factor / rating families that sit on the edges of fp32 (subnormals, signed zeros), the rating sets that make the training
kernel take each of its loop forms, the oracle replay that starts from given factors, the conditions that keep those
tests from being vacuous (checked on the oracle's results only), and the sorted-prediction reference of recommend()."""
import numpy as np

LR = LAM = 0.05  # of every training case here
TINY = np.float32(1.17549435e-38)  # the smallest normal fp32
FAMILIES = ("p_subnormal", "q_subnormal", "tiny_products", "signed_zero")


def kp_of(k):
    """Row width on the device: 4 floats per lane, a power-of-two number of lanes."""
    need, L = (k + 3) // 4, 1
    while L < need:
        L <<= 1
    return 4 * L


def is_subnormal(a):
    """Non-zero and below the smallest normal, elementwise."""
    a = np.abs(np.asarray(a, np.float32))
    return (a > 0) & (a < TINY)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host_keeps_subnormals():
    """False if something switched this process's fp32 arithmetic to flush-to-zero: then the oracle is no reference."""
    return float(np.float32(3e-40) * np.float32(0.5)) != 0.0


# ---- A1: input families ---------------------------------------------------------------------------------------------
def family(name, U, I, k, n, seed=0):
    """(P0, Q0, r) for a U x I model of rank k and n ratings.  The scales shrink with k (rows of norm about 1, products
    summed over k still subnormal), so that lr = 0.05 stays stable and the dots stay where the family wants them."""
    rng = np.random.default_rng([seed, U, I, k, n, FAMILIES.index(name)])
    unit = lambda rows: (rng.uniform(0.5, 1.5, (rows, k)) / np.sqrt(k)).astype(np.float32)  # noqa: E731
    sub = lambda rows: (rng.uniform(1.0, 5.0, (rows, k)) * 1e-40).astype(np.float32)  # noqa: E731
    if name == "p_subnormal":  # lr * r, the dot and the P update are subnormal arithmetic
        return sub(U), unit(I), rng.uniform(1e-41, 4e-39, n).astype(np.float32)
    if name == "q_subnormal":
        return unit(U), sub(I), rng.uniform(1e-41, 4e-39, n).astype(np.float32)
    if name == "tiny_products":  # normal inputs; every product and every dot is subnormal
        s = 1e-20 * k ** -0.25
        P = (rng.uniform(0.5, 1.5, (U, k)) * s).astype(np.float32)
        Q = (rng.uniform(0.5, 1.5, (I, k)) * s).astype(np.float32)
        return P, Q, rng.uniform(0.2e-39, 2e-39, n).astype(np.float32)
    if name == "signed_zero":
        assert k == kp_of(k), "a pad column is +0.0: a -0.0 dot needs k == kp"
        P = (rng.standard_normal((U, k)) / np.sqrt(k)).astype(np.float32)
        Q = (rng.standard_normal((I, k)) / np.sqrt(k)).astype(np.float32)
        P[::2] = np.abs(P[::2]) + np.float32(0.01)  # all-positive rows: their dot with a -0.0 row is -0.0
        Q[0::3] = np.float32(-0.0)
        Q[1::3] = np.float32(0.0)
        r = rng.uniform(1.0, 5.0, n).astype(np.float32)
        r[0::5] = np.float32(0.0)
        r[1::10] = np.float32(-0.0)
        return P, Q, r
    raise ValueError(name)


def flushed(name, P0, Q0, r):
    """The same problem with the subnormal inputs replaced by 0: what a flush-to-zero reader would see."""
    z = lambda a: np.where(is_subnormal(a), np.float32(0), a).astype(np.float32)  # noqa: E731
    return z(P0), z(Q0), z(r)


# ---- A2: rating sets, one per loop form of the training kernel (the shapes of tests/test_gpu_parity.py) -----------------
def general_set(k):
    """test_every_k's: general steps."""
    rng = np.random.default_rng(k)
    U, I, n = 300, 200, 12000
    key = rng.choice(U * I, n, replace=False)
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), {}


def hot_item_set(k, W):
    """test_solo_runs_every_geometry's: item 7 rated by everybody -- run loops and solo runs."""
    rng = np.random.default_rng(k * 10 + W)
    U, I = 3000, 80
    u = list(range(U)) + list(rng.integers(0, U, 9000))
    i = [7] * U + list(rng.integers(0, I, 9000))
    key = rng.permutation(np.unique(np.array(u) * I + np.array(i)))
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), dict(blocks=24 if k == 256 else 5, waves=W)


def chunked_set(k, B, W, n):
    """test_chunked_cells': cells larger than the LDS image."""
    rng = np.random.default_rng(k + B)
    U, I = 900, 800
    key = rng.choice(U * I, n, replace=False)
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), dict(blocks=B, waves=W)


def hot_user_set():
    """test_hot_user_chain_swapped_roles': user 7 rates everything -- the roles of P and Q are swapped."""
    rng = np.random.default_rng(19)
    U, I = 60, 3000
    u = [7] * I + list(rng.integers(0, U, 6000))
    i = list(range(I)) + list(rng.integers(0, I, 6000))
    key = np.unique(np.array(u) * I + np.array(i))
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), {}


GENERAL_K = (1, 4, 5, 8, 64, 100, 128, 256)
SOLO_KW = ((64, 2), (128, 4), (256, 2))
CHUNKED = ((256, 1, 2, 900), (128, 2, 4, 4000))
SIGNED_ZERO_K = (4, 8, 64, 128, 256)


def training_cases():
    """(id, family, set builder, its arguments, k) of every parametrisation of the training tests."""
    out = []
    for fam in FAMILIES:
        for k in GENERAL_K:
            if fam != "signed_zero" or k in SIGNED_ZERO_K:
                out.append((f"general-{fam}-k{k}", fam, general_set, (k,), k))
        for k, W in SOLO_KW:
            out.append((f"solo-{fam}-k{k}-w{W}", fam, hot_item_set, (k, W), k))
        for k, B, W, n in CHUNKED:
            out.append((f"chunked-{fam}-k{k}-b{B}", fam, chunked_set, (k, B, W, n), k))
        out.append((f"swapped-{fam}-k64", fam, hot_user_set, (), 64))
    return out


def oracle_train_from(oracle, P0, Q0, u, i, r, order, epochs, lr=LR, lam=LAM):
    """The oracle replaying `order` (None: the natural order) from the given factors: (P, Q, RMSE after each epoch)."""
    P, Q = P0.copy(), Q0.copy()
    order = np.arange(len(r), dtype=np.int64) if order is None else order
    rm = []
    for _ in range(epochs):
        oracle.sgd_pass_ordered(P, Q, u, i, r, order, lr, lam)
        rm.append(oracle.rmse(P, Q, u, i, r))
    return P, Q, np.array(rm)


# ---- A6: what keeps the comparisons from being vacuous; on the oracle's results only ------------------------------------
def check_inputs(fam, P0, Q0, r):
    if fam == "p_subnormal":
        assert is_subnormal(P0).all() and is_subnormal(r).all()
    if fam == "q_subnormal":
        assert is_subnormal(Q0).all() and is_subnormal(r).all()
    if fam == "tiny_products":
        assert not is_subnormal(P0).any() and not is_subnormal(Q0).any() and (P0 != 0).all() and (Q0 != 0).all()
    if fam == "signed_zero":
        assert (bits(Q0) == 0x80000000).all(axis=1).sum() >= 20 and (bits(Q0) == 0).all(axis=1).sum() >= 20
        assert (P0 > 0).all(axis=1).sum() >= 20


def check_predictions(fam, want):
    """`want`: the oracle's predictions of the pairs a test uses."""
    assert np.isfinite(want).all()
    if fam == "tiny_products":
        assert is_subnormal(want).mean() >= 0.9
    if fam == "signed_zero":
        assert (bits(want) == 0x80000000).sum() >= 20 and (bits(want) == 0).sum() >= 20


def check_training(oracle, fam, P0, Q0, u, i, r, order, epochs, trained):
    """trained = (P, Q, rmse) of the oracle over `order`.  The subnormal side moved, and moved differently from a run whose
    subnormal inputs were flushed; the RMSE is not zero; the predictions at the start are what the family is about."""
    Po, Qo, rmo = trained
    assert np.isfinite(Po).all() and np.isfinite(Qo).all() and np.isfinite(rmo).all() and (rmo != 0).all()
    check_inputs(fam, P0, Q0, r)
    check_predictions(fam, oracle.predict(P0, Q0, u, i))
    if fam in ("p_subnormal", "q_subnormal"):
        Pz, Qz, rz = flushed(fam, P0, Q0, r)
        Pf, Qf, _ = oracle_train_from(oracle, Pz, Qz, u, i, rz, order, epochs)
        got, start, flush = (Po, P0, Pf) if fam == "p_subnormal" else (Qo, Q0, Qf)
        assert (bits(got) != bits(start)).mean() >= 0.5
        assert (bits(got) != bits(flush)).mean() >= 0.5


# ---- serving: recommend() by sorting the oracle's predictions -----------------------------------------------------------
def all_scores(oracle, P, Q, user):
    I = Q.shape[0]
    return oracle.predict(P, Q, np.full(I, user, np.int32), np.arange(I, dtype=np.int32))


def top_of(sc, topn, excluded=None):
    """Items of the topn largest scores, ties by the smaller item: np.lexsort((items, -scores)) of the eligible items,
    pre-selected with np.partition where the row is long (everything that ties with the topn-th stays in)."""
    keep = np.ones(sc.size, bool)
    if excluded is not None:
        keep[excluded] = False
    it = np.flatnonzero(keep).astype(np.int32)
    s = sc[it].astype(np.float64)
    if it.size > 4 * topn:
        kth = np.partition(s, it.size - topn)[it.size - topn]
        sel = s >= kth
        it, s = it[sel], s[sel]
    return it[np.lexsort((it, -s))][:topn]


def recommend_ref(oracle, P, Q, users, topn, eu=None, ei=None, score_rows=None):
    """(items, scores) of recommend(users, topn, exclude=(eu, ei)): rows padded with -1 / NaN.  score_rows: {user: the
    oracle's scores of every item}, filled here and shared between the calls of one test."""
    items = np.full((len(users), topn), -1, np.int32)
    scores = np.full((len(users), topn), np.nan, np.float32)
    score_rows = {} if score_rows is None else score_rows
    for row, user in enumerate(users):
        user = int(user)
        if user not in score_rows:
            score_rows[user] = all_scores(oracle, P, Q, user)
        sc = score_rows[user]
        assert not np.isnan(sc).any()  # (include/mfsgd.h leaves the place of a NaN score unspecified)
        top = top_of(sc, topn, None if eu is None else ei[eu == user])
        items[row, :top.size] = top
        scores[row, :top.size] = sc[top]
    return items, scores


def assert_recommend(got, want, what=""):
    """Items equal, scores bit for bit (the sign of a zero counts; the NaN of a padded place is any NaN)."""
    (gi, gs), (wi, ws) = got, want
    np.testing.assert_array_equal(gi, wi, err_msg=what)
    pad = wi < 0
    assert np.isnan(gs[pad]).all(), what
    assert gs[~pad].tobytes() == ws[~pad].tobytes(), what


def tied_factors(U, I, k, seed):
    """Ordinary factors with a third of the catalogue scoring exactly alike (the existing serving tests' construction)."""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[rng.integers(0, I, I // 3)] = Q[3 % I]
    return rng, P, Q


def exclusions_like_the_exclude_test(rng, oracle, P, Q, users, topn, plain):
    """The pairs of test_recommend_excluding_matches_sorted_predictions for users = [0, 7, 7, U - 1, 13, 21]: every
    row's top-1, half of the tie group at user 0's threshold, a tenth of the catalogue (13), a few of 7's list, all of
    21's items, all but topn // 2 of U - 1's, users nobody asked for; a quarter given twice; shuffled."""
    U, I = P.shape[0], Q.shape[0]
    allitems = np.arange(I, dtype=np.int32)
    pu, pi = [], []

    def add(user, items):
        items = np.asarray(items, np.int32).ravel()
        pu.append(np.full(items.size, user, np.int32))
        pi.append(items)

    for row, user in enumerate(users):
        add(user, plain[row, :1])
    s0 = all_scores(oracle, P, Q, 0)
    add(0, allitems[s0 == s0[plain[0, -1]]][::2])
    add(13, rng.choice(I, max(1, I // 10), replace=False))
    add(7, plain[1, 1:topn:3])
    add(21, allitems)
    add(U - 1, rng.permutation(I)[topn // 2:])
    add(5, rng.integers(0, I, 300))
    add(U - 2, allitems)
    eu, ei = np.concatenate(pu), np.concatenate(pi)
    dup = rng.integers(0, eu.size, eu.size // 4)
    eu, ei = np.concatenate([eu, eu[dup]]), np.concatenate([ei, ei[dup]])
    perm = rng.permutation(eu.size)
    return eu[perm], ei[perm]


# ---- A4: predict and fold-in ---------------------------------------------------------------------------------------------
PREDICT_K = (1, 4, 8, 16, 32, 40, 64, 100, 128, 129, 256)  # every lane-group width, 1 .. 64


def predict_cases():
    return [(k, fam) for k in PREDICT_K for fam in ("ordinary",) + FAMILIES if fam != "signed_zero" or k == kp_of(k)]


def predict_inputs(k, fam):
    """(P, Q, u, i, r): 5000 random pairs of a 120 x 90 model (test_predict_and_set_factors' shape) and a rating each."""
    U, I, n = 120, 90, 5000
    rng = np.random.default_rng(1000 + k)
    uu = rng.integers(0, U, n).astype(np.int32)
    ii = rng.integers(0, I, n).astype(np.int32)
    if fam == "ordinary":
        P = rng.standard_normal((U, k)).astype(np.float32)
        Q = rng.standard_normal((I, k)).astype(np.float32)
        return P, Q, uu, ii, rng.uniform(1.0, 5.0, n).astype(np.float32)
    P, Q, r = family(fam, U, I, k, n)
    return P, Q, uu, ii, r


FOLD_IN_K = (8, 64, 256)
FOLD_IN_FAMILIES = ("p_subnormal", "q_subnormal", "tiny_products")


def fold_in_inputs(k, fam):
    """(Q, row_ptr, items, ratings, init): 50 new users with 0 .. 59 ratings each against 300 items; the start rows are
    the family's P."""
    n_new, I = 50, 300
    rng = np.random.default_rng(2000 + k)
    lens = rng.integers(0, 60, n_new)
    lens[0] = lens[17] = 0
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = rng.integers(0, I, int(row_ptr[-1])).astype(np.int32)
    init, Q, ratings = family(fam, n_new, I, k, items.size)
    return Q, row_ptr, items, ratings, init


# ---- C5: scores at the edges of fp32 -------------------------------------------------------------------------------------
SCORE_KINDS = ("negative_zero", "infinite", "subnormal")
EDGE_I, EDGE_USER = 700, 7
ZERO_ITEMS = np.arange(100, 140)  # even: rows of -0.0, odd: rows of +0.0 -- all tie
POS_INF_ITEMS, NEG_INF_ITEMS = np.array([650, 13, 300, 299]), np.array([5, 699, 301, 42])


def edge_score_factors(kind, k):
    """(P, Q, user): 700 items whose scores for `user` (an all-positive row) hold real -0.0 and +0.0 scores in the
    middle of the ranking / +inf and -inf scores / nothing but distinct subnormals."""
    assert k == kp_of(k)
    rng = np.random.default_rng([k, SCORE_KINDS.index(kind)])
    U, I = 12, EDGE_I
    if kind == "subnormal":
        s = 1e-20 * k ** -0.25
        return ((rng.uniform(0.5, 1.5, (U, k)) * s).astype(np.float32),
                (rng.uniform(0.5, 1.5, (I, k)) * s).astype(np.float32), EDGE_USER)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    P[EDGE_USER] = np.abs(P[EDGE_USER]) + np.float32(1.0)
    if kind == "negative_zero":
        Q = -np.abs(Q)               # negative scores for the user ...
        Q[::11] = np.abs(Q[::11])    # ... but for 64 items: the zeros are places 64 .. 103 or so, inside a top 128
        Q[ZERO_ITEMS[0::2]] = np.float32(-0.0)
        Q[ZERO_ITEMS[1::2]] = np.float32(0.0)
    if kind == "infinite":
        Q[POS_INF_ITEMS] = np.float32(3e38)   # one sign per row and an all-positive user row: no NaN arises
        Q[NEG_INF_ITEMS] = np.float32(-3e38)
    return P, Q, EDGE_USER


def check_edge_scores(kind, sc):
    """sc: the oracle's scores of every item for the user."""
    assert not np.isnan(sc).any()
    if kind == "negative_zero":
        assert (bits(sc[ZERO_ITEMS[0::2]]) == 0x80000000).all() and (bits(sc[ZERO_ITEMS[1::2]]) == 0).all()
        assert 20 <= (sc > 0).sum() <= 128 - ZERO_ITEMS.size  # the zeros lie inside the first 128 places, not at the top
    if kind == "infinite":
        assert np.isposinf(sc[POS_INF_ITEMS]).all() and np.isneginf(sc[NEG_INF_ITEMS]).all()
        assert np.isinf(sc).sum() == POS_INF_ITEMS.size + NEG_INF_ITEMS.size
    if kind == "subnormal":
        assert is_subnormal(sc).all() and np.unique(sc).size >= 600


# ---- NaN and Inf through the solo runs (tests/test_chain_specials_gpu.py, tests/test_contract_edges_cpu.py) -----------
ALL_ONES_NAN = np.array([0xFFFFFFFF], np.uint32).view(np.float32)[0]  # the NaN whose bits are a solo record's empty mailbox
HOT_ITEM = 7  # hot_item_set's


def solo_runs(mf, U, I, k, u, i, **kw):
    """The solo runs of the schedule a handle of this geometry builds (host packer; no GPU needed): one array of rating
    indices per run, in step order, runs in schedule order.  Read off the records themselves: with the ratings 1, 2, 3 ...
    a record {next slots, mailbox = all ones, lr * r, r} names its rating in its last word; the header in front of a
    run's records has mailbox 0, the terminator behind them r = 0, and no step entry holds all ones in its second word."""
    assert u.size < (1 << 24)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1, **kw) as m:
        m.set_ratings(u, i, np.arange(1, u.size + 1, dtype=np.float32))
        ent = m.debug_schedule()[3]
        order = m.order()[0]
        n_solo = int((m.debug_schedule()[2][:, 0] >> 16).sum())
    rec = (ent[:, 1] == 0xFFFFFFFF) & (ent[:, 3] != 0)
    at = np.flatnonzero(rec)
    runs = [ent[x, 3].view(np.float32).astype(np.int64) - 1 for x in np.split(at, np.flatnonzero(np.diff(at) != 1) + 1)] if at.size else []
    assert sum(x.size for x in runs) == n_solo
    place = np.empty(u.size, np.int64)
    place[order] = np.arange(u.size)
    for x in runs:  # the steps of a run follow the exported order, and are one item's
        assert (np.diff(place[x]) == 1).all() and np.unique(i[x]).size == 1
    runs.sort(key=lambda x: place[x[0]])
    return runs, place


def odd_run_set(mf, k, W):
    """hot_item_set(k, W) if a solo run of item 7 has an odd number of steps (k = 256: 125); else the same set with ONE
    rating of item 7 moved to an item its user has not rated -- every user keeps its degree, and with it its block -- so
    that one run of 300 / 150 steps becomes one of 299 / 149 (asserted by whoever uses it: runs_of_the_hot_item)."""
    U, I, u, i, kw = hot_item_set(k, W)
    runs, _ = solo_runs(mf, U, I, k, u, i, **kw)
    if any(x.size % 2 == 1 and i[x[0]] == HOT_ITEM for x in runs):
        return U, I, u, i, kw
    last = [x for x in runs if i[x[0]] == HOT_ITEM][-1]
    j = last[last.size // 2]
    mine = set(i[u == u[j]].tolist())
    i = i.copy()
    i[j] = next(t for t in range(I - 1, -1, -1) if t not in mine)
    return U, I, u, i, kw


def runs_of_the_hot_item(mf, U, I, k, u, i, item=HOT_ITEM, **kw):
    runs, place = solo_runs(mf, U, I, k, u, i, **kw)
    return [x for x in runs if i[x[0]] == item], place


NAN_PLACES = ("rating_first_step", "rating_even_step", "rating_odd_step", "rating_last_step_of_an_odd_run", "p_row_mid_run", "q_hot_item")


def place_nan(where, mf, k, U, I, u, i, kw, P0, Q0, r, item=HOT_ITEM):
    """One all-ones NaN at `where` (NAN_PLACES), as late in the exported order as that place exists, so that one epoch leaves
    NaN and finite entries side by side: the rating places in the LAST solo run of the item (of the last odd-length one);
    the P row of that user in the middle half of a run whose FIRST rating comes latest in the order (a NaN row spreads
    from the first rating of its user on).  Q[item] cannot be late: everybody who rated the item -- in hot_item_set every
    user -- is NaN after one epoch.  Returns (P0, Q0, r, run length, step)."""
    runs, place = runs_of_the_hot_item(mf, U, I, k, u, i, item, **kw)
    assert runs and all(x.size >= 12 for x in runs)
    P0, Q0, r = P0.copy(), Q0.copy(), r.copy()
    run, step = runs[-1], -1
    if where == "rating_first_step":
        step = 0
    elif where == "rating_even_step":
        step = (run.size // 2) & ~1
    elif where == "rating_odd_step":
        step = (run.size // 2) | 1
    elif where == "rating_last_step_of_an_odd_run":
        run = [x for x in runs if x.size % 2 == 1][-1]
        step = run.size - 1
    elif where == "p_row_mid_run":
        first = np.full(U, u.size, np.int64)
        np.minimum.at(first, u, place)
        mid = [(first[u[x[t]]], n, t) for n, x in enumerate(runs) for t in range(x.size // 4, x.size - x.size // 4)]
        _, n, step = max(mid)
        run = runs[n]
        P0[u[run[step]], (3 * k) // 4] = ALL_ONES_NAN
        return P0, Q0, r, run.size, step
    elif where == "q_hot_item":
        Q0[item, k // 3] = ALL_ONES_NAN
        return P0, Q0, r, run.size, step
    else:
        raise ValueError(where)
    r[run[step]] = ALL_ONES_NAN
    return P0, Q0, r, run.size, step


def ordinary_factors(U, I, k, seed=3):
    rng = np.random.default_rng([seed, U, I, k])
    return ((rng.standard_normal((U, k)) / np.sqrt(k)).astype(np.float32),
            (rng.standard_normal((I, k)) / np.sqrt(k)).astype(np.float32))


def ordinary_ratings(n, seed=4):
    return (np.random.default_rng([seed, n]).random(n) * 4 + 1).astype(np.float32)


def assert_same_but_for_the_nans(name, got, want):
    """The NaN masks are equal and every other entry is equal bit for bit, infinities included."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{name}: {(np.isnan(got) != nan).sum()} entries are NaN on one side only"
    assert got[~nan].tobytes() == want[~nan].tobytes(), f"{name}: entries that are not NaN differ"


def assert_rmse_same_but_for_the_nans(rm, rmo):
    assert np.isfinite(rm) == np.isfinite(rmo), (rm, rmo)
    if np.isfinite(rmo):
        np.testing.assert_allclose(rm, rmo, rtol=1e-9, atol=0)


def nan_share(P, Q):
    return float(np.isnan(np.concatenate([P.ravel(), Q.ravel()])).mean())


def classes(P, Q):
    """(finite, infinite, NaN entries present) of a state."""
    both = np.concatenate([P.ravel(), Q.ravel()])
    return bool(np.isfinite(both).any()), bool(np.isinf(both).any()), bool(np.isnan(both).any())


LONE_CELLS = {64: 0, 128: 0, 256: 24}  # lone-tile cells of hot_item_set(k, W) at SOLO_KW (k = 256: B = 24, all of item 7's)
LONE_ITEM, LONE_PROBLEM_CELLS = 9, 24  # lone_problem: items 9 and 17 have a tile each, 12 cells per tile


def lone_problem():
    """test_lone_hop_gpu.test_row_widths' problem at k = 64: B = 12, item 9 rated by all 1800 users -- 150 per cell, one solo
    run each, every cell a lone-tile cell of the fast lane.  (U, I, k, u, i, r, constructor keywords)"""
    from tests.test_lone_hop_gpu import _problem

    U, I, u, i, r = _problem(150 * 12, 90, 6, 64 + 12)
    return U, I, 64, u, i, r, dict(blocks=12, waves=2)


def check_nan_case(where, states):
    """states: the oracle's [(P, Q, rmse)] after each epoch of a NaN case.  After the first epoch NaN and finite entries
    stand side by side, between 0.05 % and 60 % NaN -- but for the NaN in Q[hot item]: every user rated that item, so all
    of P is NaN after one epoch wherever the item's ratings come in the order, and so is most or all of Q."""
    share = nan_share(*states[0][:2])
    assert np.isnan(states[0][2]) and np.isnan(states[-1][2])
    if where == "q_hot_item":
        assert share > 0.6 and np.isnan(states[0][0]).all()
    else:
        assert 0.0005 <= share <= 0.6, share
        assert not np.isinf(states[0][0]).any() and not np.isinf(states[0][1]).any()
    assert nan_share(*states[-1][:2]) >= share


# ---- overflow through every loop form (B) ------------------------------------------------------------------------------
def _without_k_and_r(U, I, k, u, i, r, kw):
    return U, I, u, i, kw


OVERFLOW_SETS = {  # name -> (set builder, k, hot item or None)
    "hot_item_k64_w2": (lambda: hot_item_set(64, 2), 64, HOT_ITEM),
    "hot_item_k128_w4": (lambda: hot_item_set(128, 4), 128, HOT_ITEM),
    "hot_item_k256_w2": (lambda: hot_item_set(256, 2), 256, HOT_ITEM),
    "chunked_k256_b1": (lambda: chunked_set(256, 1, 2, 900), 256, None),
    "swapped_k64": (hot_user_set, 64, None),
    "lone_k64_b12": (lambda: _without_k_and_r(*lone_problem()), 64, LONE_ITEM),
}
OVERFLOW_PLACES = ("anywhere", "last_in_the_order", "on_the_hot_item")


def overflow_cases():
    return [(name, where) for name in sorted(OVERFLOW_SETS) for where in OVERFLOW_PLACES
            if where != "on_the_hot_item" or OVERFLOW_SETS[name][2] is not None]


def overflow_ratings(where, u, i, order, hot):
    """Ratings 1 .. 5 with +-3e38 on 1 % of them, anywhere or at the end of `order`; or on the hot item's last 20 ratings
    in `order`."""
    rng = np.random.default_rng(5)
    r = (rng.random(u.size) * 4 + 1).astype(np.float32)
    n_big = 20 if where == "on_the_hot_item" else u.size // 100
    huge = np.where(rng.random(n_big) < 0.5, np.float32(3e38), np.float32(-3e38))
    if where == "anywhere":
        r[rng.choice(u.size, n_big, replace=False)] = huge
    elif where == "last_in_the_order":
        r[order[-n_big:]] = huge
    else:
        r[order[i[order] == hot][-n_big:]] = huge
    return r


def check_overflow_set(name, info, sched):
    """The schedule holds the loop form the set is there for."""
    solo, lone = int(((sched[2][:, 0] >> 16) > 0).sum()), int((sched[0][:, 5] & 1).sum())
    if name.startswith("hot_item"):
        run_steps = int((sched[2][:, 1] >> 16).sum())  # (at k = 64 the light items' chains stay general steps)
        assert solo >= 10 and (run_steps > 0 or OVERFLOW_SETS[name][1] == 64), (solo, run_steps)
        assert lone == LONE_CELLS[OVERFLOW_SETS[name][1]]
    if name.startswith("chunked"):
        assert info["split_cells"] >= 1
    if name.startswith("swapped"):
        assert info["swapped"] == 1
    if name.startswith("lone"):
        assert lone == LONE_PROBLEM_CELLS and solo >= 12


def check_overflow_case(where, states):
    """The rule of test_overflow_goes_to_infinity_and_nan_where_the_oracle_does, on the oracle's states after each epoch:
    NaN has been seen and the last RMSE is not finite; and, unless the large ratings are anywhere (then everything may be
    NaN within the first epoch), finite, infinite and NaN entries have each been seen and one state holds at least two of
    the classes side by side."""
    seen = np.array([classes(P, Q) for P, Q, _ in states])
    assert seen[:, 2].any() and not np.isfinite(states[-1][2])
    if where != "anywhere":
        assert seen.any(axis=0).all(), seen
        assert (seen.sum(axis=1) >= 2).any(), seen


# ---- NaN and overflow through apply_ratings and fold-in (B) -----------------------------------------------------------
ONLINE_SPECIALS = [(batch, kind, k) for batch in ("one_item", "wide") for kind in ("nan", "huge") for k in (64, 5)]


def online_special_batch(batch, kind):
    """online_common's one_item_batch (a chain of 600 levels) or hot_item_batch (wide levels, every 40th rating of item 7)
    with ONE special rating half-way, on the hot item: an all-ones NaN, or 3e38 (the item's row grows, overflows and
    turns NaN over the next few of its ratings)."""
    from tests import online_common as oc

    U, I, u, i, r = oc.one_item_batch() if batch == "one_item" else oc.hot_item_batch()
    at = (u.size // 2) // 40 * 40
    assert i[at] == (3 if batch == "one_item" else 7)
    r = r.copy()
    r[at] = ALL_ONES_NAN if kind == "nan" else np.float32(3e38)
    return U, I, u, i, r, at


def check_online_special(kind, at, err, P, Q):
    """On the oracle's results: the errors before the special rating are finite; a NaN rating's own error and later ones
    are NaN, and NaN and finite rows stand side by side in P and in Q; a rating of 3e38 leaves infinite entries in P (in
    the chain of one item every user comes once: the rows overflow and stay infinite, no NaN arises) beside finite ones."""
    assert np.isfinite(err[:at]).all()
    if kind == "nan":
        assert np.isnan(err[at]) and np.isnan(err[at + 1:]).any()
        for a in (P, Q):
            assert np.isnan(a).any() and np.isfinite(a).any()
    else:
        assert err[at] > 1e38 and np.isinf(P).any() and np.isfinite(P).any() and np.isfinite(Q).any()


FOLD_IN_SPECIAL_USERS = {1: ((25, "nan"),), 2: ((10, "huge"),), 4: ((10, "huge"), (30, "nan"))}


def fold_in_specials(k):
    """(Q, row_ptr, items, ratings, init): six new users of 40 ratings each against 300 items; user 1 has an all-ones NaN
    rating, user 2 one of 3e38, user 4 both; users 0, 3 and 5 are ordinary."""
    rng = np.random.default_rng(3000 + k)
    n_new, I, n = 6, 300, 40
    row_ptr = (np.arange(n_new + 1) * n).astype(np.int64)
    items = np.concatenate([rng.choice(I, n, replace=False) for _ in range(n_new)]).astype(np.int32)
    ratings = rng.uniform(1.0, 5.0, items.size).astype(np.float32)
    for user, specials in FOLD_IN_SPECIAL_USERS.items():
        for at, kind in specials:
            ratings[user * n + at] = ALL_ONES_NAN if kind == "nan" else np.float32(3e38)
    init, Q = ordinary_factors(n_new, I, k, seed=9)
    return Q, row_ptr, items, ratings, init


def check_fold_in_specials(want):
    assert np.isfinite(want[[0, 3, 5]]).all() and np.isnan(want[1]).all() and np.isnan(want[4]).all()
    # (3e38 alone: against fixed item rows the row stays finite, at the top of fp32's range)
    assert np.isfinite(want[2]).all() and np.abs(want[2]).max() > 1e30


# ---- hot rows on the user side and on both sides (D) --------------------------------------------------------------------
def hot_user_lone_set(B):
    """The lone-tile problem transposed: user 9 rates all 150 * B items, user 17 every other one, 4 * 150 * B random
    ratings on top -- the roles are swapped, users 9 and 17 have a tile each (2 B lone-tile cells, 2 B solo runs)."""
    from tests.test_lone_hop_gpu import _problem

    I, U, i, u, r = _problem(150 * B, 90, 4, 500 + B)
    return U, I, u, i, r


def two_sided_set(U, I, seed=1):
    """User 3 rates every item AND item 9 is rated by every user, 3 * max(U, I) random ratings on top: the longer side's
    hot row gets the lone tile and the solo runs (U < I: roles swapped), the other side's is a chain of dependent steps
    in every cell it meets."""
    rng = np.random.default_rng(seed)
    n = 3 * max(U, I)
    u = list(range(U)) + [3] * I + list(rng.integers(0, U, n))
    i = [9] * U + list(range(I)) + list(rng.integers(0, I, n))
    key = rng.permutation(np.unique(np.array(u, np.int64) * I + np.array(i)))
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(key.size) * 4 + 1).astype(np.float32)
