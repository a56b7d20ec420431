"""Python mirror of the Java surface ``MatrixFactorizationSGD`` (train/predict).

The reference repository contains no source (/root/reference/README.md:1-2), so
the surface is the one SURVEY.md section 8b derives from BASELINE.json:
``new MatrixFactorizationSGD(users, items, k, lr, lambda, seed)``,
``double[] train(int[] u, int[] i, float[] r, int epochs)``,
``float predict(int u, int i)`` / ``float[] predict(int[] u, int[] i)``,
``close()``.  Every method is a thin call into the C-ABI (include/mfsgd.h).
"""
import ctypes as C

import numpy as np

from . import _lib


class MfsgdError(RuntimeError):
    """A C-ABI call returned a non-zero status (the JNI shim throws
    RuntimeException in the same place)."""

    def __init__(self, code, message):
        super().__init__(f"mfsgd error {code}: {message}")
        self.code = code


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def _candidates(cand, n_rows):
    """The `candidates` argument of recommend / recommend_rows as the C-ABI takes it: (ptr int64[n_rows + 1] or None,
    items int32[n]).  A 1-d integer array (or list of integers): one list shared by every row.  A tuple (ptr, items): CSR
    over the request rows.  Any other sequence: one 1-d integer array per request row."""
    def ints(a, what):
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError(f"{what} must be a 1-d integer array")
        return a
    if isinstance(cand, tuple):
        if len(cand) != 2:
            raise ValueError("candidates as a tuple must be (ptr, items)")
        ptr, items = ints(cand[0], "candidates' ptr"), ints(cand[1], "candidates' items")
        if ptr.size != n_rows + 1:
            raise ValueError("candidates' ptr must have one entry per requested row, and one more")
        return np.ascontiguousarray(ptr, dtype=np.int64), _i32(items)
    if isinstance(cand, np.ndarray) or len(cand) == 0 or np.isscalar(cand[0]):
        return None, _i32(ints(cand, "candidates"))
    lists = [ints(c, "each row's candidates") for c in cand]
    if len(lists) != n_rows:
        raise ValueError("candidates must hold one list per requested row")
    ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum([c.size for c in lists], out=ptr[1:])
    return ptr, _i32(np.concatenate(lists)) if lists else np.empty(0, np.int32)


def debug_device_bytes():
    """mfsgd_debug_device_bytes: bytes of device memory the library holds in this process right now, over all handles."""
    live = C.c_int64(-1)
    rc = _lib.load_library().mfsgd_debug_device_bytes(C.byref(live))
    if rc != 0:
        raise MfsgdError(rc, "mfsgd_debug_device_bytes: bad argument")
    return live.value


def dsgd_plan(deg_user, deg_item, n_parts):
    """The global DSGD partitioner (mfsgd_dsgd_plan): (user_begin[n_parts + 1], item_part[n_items])."""
    du = np.ascontiguousarray(deg_user, np.int64)
    di = np.ascontiguousarray(deg_item, np.int64)
    ub = np.empty(int(n_parts) + 1, np.int32)
    ip = np.empty(di.size, np.int32)
    rc = _lib.load_library().mfsgd_dsgd_plan(_p(du, C.c_int64), _p(di, C.c_int64), du.size, di.size, int(n_parts),
                                             _p(ub, C.c_int32), _p(ip, C.c_int32))
    if rc != 0:
        raise MfsgdError(rc, "mfsgd_dsgd_plan: bad argument")
    return ub, ip


def dsgd_plan_ex(deg_user, deg_item, world, parts_per_rank=1, k=64, chain_crit=0.0):
    """mfsgd_dsgd_plan_ex: (user_begin[world + 1], item_part[n_items] over world * parts_per_rank partitions, info);
    chain_crit = 0: plain LPT (what a ring wants), > 0: chain-aware packing (include/mfsgd.h);
    info = dict(sum_max_chain, critical_items, sequential_parts, threshold)."""
    du = np.ascontiguousarray(deg_user, np.int64)
    di = np.ascontiguousarray(deg_item, np.int64)
    ub = np.empty(int(world) + 1, np.int32)
    ip = np.empty(di.size, np.int32)
    info = np.zeros(4, np.int64)
    rc = _lib.load_library().mfsgd_dsgd_plan_ex(_p(du, C.c_int64), _p(di, C.c_int64), du.size, di.size, int(world),
                                                int(parts_per_rank), int(k), float(chain_crit), _p(ub, C.c_int32), _p(ip, C.c_int32),
                                                _p(info, C.c_int64))
    if rc != 0:
        raise MfsgdError(rc, "mfsgd_dsgd_plan_ex: bad argument")
    return ub, ip, dict(sum_max_chain=int(info[0]), critical_items=int(info[1]), sequential_parts=int(info[2]),
                        threshold=int(info[3]))


def ranking_metrics(users, ranks, topn):
    """mfsgd_ranking_metrics_from_ranks (host only, needs no model and no GPU): dict(n_pairs, n_users, hit_rate,
    precision, recall, ndcg, mrr) of held-out pairs given as (user, rank of the item) at cut-off topn -- means over the
    users that have a pair.  The pairs must be distinct for the figures to mean anything."""
    uu, rr = _i32(users), _i32(ranks)
    if uu.shape != rr.shape or uu.ndim != 1:
        raise ValueError("users and ranks must have the same 1-d shape")
    lib = _lib.load_library()
    out = _lib.RankingMetrics()
    rc = lib.mfsgd_ranking_metrics_from_ranks(_p(uu, C.c_int32), _p(rr, C.c_int32), uu.size, int(topn), C.byref(out))
    if rc != 0:
        raise MfsgdError(rc, lib.mfsgd_last_error(None).decode())
    return out.as_dict()


def bpr_weights(x):
    """mfsgd_bpr_weights (host only, needs no model and no GPU): float32 g = lsig(x) = 1 / (1 + e^x) for every margin in
    x, by the function the pairwise kernel compiles (include/mfsgd.h, "pairwise ranking"): the weight of a BPR step."""
    xx = _f32(x)
    g = np.empty(xx.shape, np.float32)
    lib = _lib.load_library()
    rc = lib.mfsgd_bpr_weights(_p(xx, C.c_float), _p(g, C.c_float), xx.size)
    if rc != 0:
        raise MfsgdError(rc, lib.mfsgd_last_error(None).decode())
    return g


def warp_weights(rank):
    """mfsgd_warp_weights (host only, needs no model and no GPU): float32 w = L(rank), L(0) = 0 and L(r) = 1/1 + 1/2 + ...
    + 1/r summed in float64 in ascending order and rounded once, for every rank sample_unseen_violating estimated
    (include/mfsgd.h): the weight of a WARP step.  A negative rank is refused."""
    rr = _i32(rank)
    w = np.empty(rr.shape, np.float32)
    lib = _lib.load_library()
    rc = lib.mfsgd_warp_weights(_p(rr, C.c_int32), _p(w, C.c_float), rr.size)
    if rc != 0:
        raise MfsgdError(rc, lib.mfsgd_last_error(None).decode())
    return w


def popularity_weights(counts, alpha=0.75, resolution=16, least=1):
    """uint32 item weights for set_item_weights from popularity counts (seen_item_counts):
    max(least, rint(resolution * counts ** alpha)), computed in float64.  alpha=0.75 is word2vec's exponent, alpha=0 the
    uniform draw, alpha=1 popularity itself; `resolution` is how finely the integer weights resolve small counts.
    least=1 keeps items nobody has seen drawable, least=0 never draws them (word2vec's behaviour).  Python only: the
    C-ABI takes the integers, so no pow decides a bit of a draw.  ValueError for a negative count, a non-finite alpha or
    a weight above 2^32 - 1."""
    cc = np.asarray(counts)
    if cc.ndim != 1:
        raise ValueError("counts must be a 1-d array")
    cc = cc.astype(np.float64)
    if not np.isfinite(alpha):
        raise ValueError("alpha must be finite")
    if cc.size and not (cc >= 0).all():
        raise ValueError("counts must not be negative")
    if int(least) < 0 or not float(resolution) >= 0:
        raise ValueError("least and resolution must not be negative")
    with np.errstate(divide="ignore"):  # (0 ** a negative alpha is inf, and refused below)
        w = np.maximum(float(int(least)), np.rint(float(resolution) * cc ** float(alpha)))
    if int(least) > 0xFFFFFFFF or (w.size and not (w <= 0xFFFFFFFF).all()):
        raise ValueError("a weight exceeds 2^32 - 1")
    return w.astype(np.uint32)


def _pairs(a, b, what):
    """Two int32 1-d arrays of one length (None: no pairs)."""
    aa, bb = (np.empty(0, np.int32),) * 2 if a is None else (_i32(a), _i32(b))
    if aa.shape != bb.shape or aa.ndim != 1:
        raise ValueError(f"{what} must be two 1-d arrays of the same length")
    return aa, bb


def _users(users):
    """The `users` argument of the calls that take one user per row: a 1-d int32 array, or ValueError."""
    uu = _i32(np.atleast_1d(users))
    if uu.ndim != 1:
        raise ValueError("users must be a 1-d array")
    return uu


def _asked(*outputs):
    """(array, asked for) pairs -> the arrays that were asked for: None, the one, or a tuple of them."""
    res = tuple(a for a, on in outputs if on)
    return None if not res else res[0] if len(res) == 1 else res


def _exclusions(exclude):
    """The `exclude` argument of the serving calls: (seen, u, i).  None: no pairs; (u, i): those pairs; the string "seen":
    what the handle's seen-item index holds (the _unseen calls of the C-ABI), and then u and i are empty."""
    if isinstance(exclude, str):
        if exclude != "seen":
            raise ValueError('exclude must be None, (u, i) or "seen"')
        return (True,) + _pairs(None, None, "exclude")
    return (False,) + _pairs(*((None, None) if exclude is None else exclude), "exclude")


class MatrixFactorizationSGD:
    def __init__(self, users, items, k, lr, lam, seed, *, device=0, blocks=0, waves=0,
                 n_parts=0, host_threads=0, flags=0):
        self._lib = _lib.load_library()
        self._h = C.c_void_p()
        self.users, self.items, self.k = int(users), int(items), int(k)
        self.lr, self.lam, self.seed = float(lr), float(lam), int(seed)
        cfg = _lib.Config(n_users=self.users, n_items=self.items, k=self.k, lr=self.lr,
                          lambda_=self.lam, device=device, blocks=blocks, waves=waves,
                          n_parts=n_parts, host_threads=host_threads, flags=flags)
        rc = self._lib.mfsgd_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            raise MfsgdError(rc, self._lib.mfsgd_last_error(None).decode())
        self.n_parts = max(1, int(n_parts))
        self._initialised = False

    # -- plumbing ---------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise MfsgdError(rc, self._lib.mfsgd_last_error(self._h).decode())

    def _handle(self):
        if not self._h:
            raise MfsgdError(-5, "handle is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mfsgd_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ratings / factors ------------------------------------------------------
    def set_ratings(self, u, i, r):
        u, i, r = _i32(u), _i32(i), _f32(r)
        if not (u.shape == i.shape == r.shape and u.ndim == 1):
            raise ValueError("u, i, r must be 1-d arrays of equal length")
        # the library itself recognises the same triples again (exact: every byte is hashed) and keeps the
        # schedules, so there is nothing to remember here
        self._check(self._lib.mfsgd_set_ratings(self._handle(), _p(u, C.c_int32), _p(i, C.c_int32),
                                                _p(r, C.c_float), u.size))

    def init_factors(self, seed=None):
        self._check(self._lib.mfsgd_init_factors(self._handle(), self.seed if seed is None else int(seed)))
        self._initialised = True

    def set_factors(self, P, Q=None):
        P = _f32(P)
        if P.shape != (self.users, self.k):
            raise ValueError("P must be users x k")
        qp = None
        if Q is not None:
            Q = _f32(Q)
            if Q.shape != (self.items, self.k):
                raise ValueError("Q must be items x k")
            qp = _p(Q, C.c_float)
        self._check(self._lib.mfsgd_set_factors(self._handle(), _p(P, C.c_float), qp))
        self._initialised = True

    def get_factors(self):
        P = np.empty((self.users, self.k), np.float32)
        if self.n_parts > 1:
            self._check(self._lib.mfsgd_get_factors(self._handle(), _p(P, C.c_float), None))
            return P, None
        Q = np.empty((self.items, self.k), np.float32)
        self._check(self._lib.mfsgd_get_factors(self._handle(), _p(P, C.c_float), _p(Q, C.c_float)))
        return P, Q

    def save_factors(self, path):
        rc = self._lib.mfsgd_save_factors(self._handle(), str(path).encode())
        if rc != 0:
            raise MfsgdError(rc, self._lib.mfsgd_io_last_error().decode() or self._lib.mfsgd_last_error(self._h).decode())

    def load_factors(self, path):
        rc = self._lib.mfsgd_load_factors(self._handle(), str(path).encode())
        if rc != 0:
            raise MfsgdError(rc, self._lib.mfsgd_io_last_error().decode() or self._lib.mfsgd_last_error(self._h).decode())
        self._initialised = True

    # -- the Java surface -------------------------------------------------------
    def train(self, u, i, r, epochs, *, rmse=True):
        """Runs `epochs` SGD passes over the ratings; returns the RMSE after each
        epoch (float64 array), as the Java ``double[] train(...)`` does."""
        self.set_ratings(u, i, r)
        if not self._initialised:
            self.init_factors()
        return self.fit(epochs, rmse=rmse)

    def fit(self, epochs, *, rmse=True):
        out = np.zeros(int(epochs), np.float64)
        self._check(self._lib.mfsgd_train(self._handle(), int(epochs),
                                          _p(out, C.c_double) if rmse else None))
        return out if rmse else None

    def set_hyper(self, lr, lam):
        """Another lr and lambda for the live model (mfsgd_set_hyper): the schedules are re-baked in place -- nothing
        is rebuilt, the factors stay where they are."""
        self._check(self._lib.mfsgd_set_hyper(self._handle(), float(lr), float(lam)))
        self.lr, self.lam = self.hyper()

    def hyper(self):
        """(lr, lambda) the handle holds now, as Python floats of the fp32 values."""
        lr, lam = C.c_float(), C.c_float()
        self._check(self._lib.mfsgd_get_hyper(self._handle(), C.byref(lr), C.byref(lam)))
        return lr.value, lam.value

    def fit_schedule(self, lr, lam=None, *, rmse=True):
        """One epoch per entry of lr, epoch e at lr[e] and lam[e] (lam None: the current lambda throughout); returns
        the RMSE after each epoch like fit().  The model keeps the last epoch's values."""
        lrs = _f32(np.atleast_1d(lr))
        lams = None if lam is None else _f32(np.atleast_1d(lam))
        if lrs.ndim != 1 or (lams is not None and lams.shape != lrs.shape):
            raise ValueError("lr and lam must be 1-d arrays of the same length")
        out = np.zeros(lrs.size, np.float64)
        try:
            self._check(self._lib.mfsgd_train_schedule(self._handle(), lrs.size, _p(lrs, C.c_float),
                                                       None if lams is None else _p(lams, C.c_float),
                                                       _p(out, C.c_double) if rmse else None))
        finally:
            if self._h:
                self.lr, self.lam = self.hyper()
        return out if rmse else None

    def fit_bold_driver(self, epochs, up=1.05, down=0.5):
        """`epochs` passes under the bold driver: after an epoch that lowered the RMSE the rate grows by `up`,
        otherwise it shrinks by `down`.  Returns (lr_used float32[epochs], rmse float64[epochs]); the model keeps
        the rate the next epoch would use."""
        used = np.zeros(int(epochs), np.float32)
        out = np.zeros(int(epochs), np.float64)
        try:
            self._check(self._lib.mfsgd_train_bold_driver(self._handle(), int(epochs), float(up), float(down),
                                                          _p(used, C.c_float), _p(out, C.c_double)))
        finally:
            if self._h:
                self.lr, self.lam = self.hyper()
        return used, out

    # -- held-out validation ------------------------------------------------------
    @staticmethod
    def _triples(u, i, r):
        uu, ii = _pairs(np.atleast_1d(u), np.atleast_1d(i), "u and i")
        rr = _f32(np.atleast_1d(r))
        if rr.shape != uu.shape:
            raise ValueError("u, i, r must be 1-d arrays of equal length")
        return uu, ii, rr

    def set_validation(self, u, i, r):
        """The held-out set of the model (mfsgd_set_validation): copied, kept on the device from the first call that
        measures it; empty arrays clear it.  Needs no GPU; survives set_ratings, set_hyper and load_factors."""
        uu, ii, rr = self._triples(u, i, r)
        self._check(self._lib.mfsgd_set_validation(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), _p(rr, C.c_float),
                                                   uu.size))

    def validation_size(self):
        n = C.c_int64(-1)
        self._check(self._lib.mfsgd_validation_size(self._handle(), C.byref(n)))
        return n.value

    def validation_rmse(self, *, sse=False):
        """RMSE of the held-out set under the current factors (sse=True: (rmse, sse)); 0.0 for an empty set."""
        rm, s = C.c_double(), C.c_double()
        self._check(self._lib.mfsgd_validation_rmse(self._handle(), C.byref(rm), C.byref(s)))
        return (rm.value, s.value) if sse else rm.value

    def rmse_on(self, u, i, r, *, sse=False):
        """RMSE of the given pairs under the current factors (mfsgd_rmse_pairs): nothing is kept."""
        uu, ii, rr = self._triples(u, i, r)
        rm, s = C.c_double(), C.c_double()
        self._check(self._lib.mfsgd_rmse_pairs(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), _p(rr, C.c_float),
                                               uu.size, C.byref(rm), C.byref(s)))
        return (rm.value, s.value) if sse else rm.value

    def fit_early_stopping(self, max_epochs, patience=3, min_delta=0.0, restore_best=True, lr=None, lam=None,
                           train_rmse=False):
        """Trains until the held-out RMSE has not improved by more than min_delta for `patience` epochs in a row, at
        most max_epochs epochs (mfsgd_train_early_stop states the rule); with restore_best the model ends with the
        factors of the best epoch.  lr / lam: per-epoch values as in fit_schedule (None: the current one throughout).
        Returns dict(val_rmse float64[epochs_run], train_rmse the same or None, epochs_run, best_epoch)."""
        n = int(max_epochs)
        lrs = None if lr is None else _f32(np.atleast_1d(lr))
        lams = None if lam is None else _f32(np.atleast_1d(lam))
        for a in (lrs, lams):
            if a is not None and a.shape != (max(n, 0),):
                raise ValueError("lr and lam must be 1-d arrays of max_epochs entries")
        val = np.zeros(max(n, 0), np.float64)
        trn = np.zeros(max(n, 0), np.float64) if train_rmse else None
        ran, best = C.c_int32(0), C.c_int32(-1)
        try:
            self._check(self._lib.mfsgd_train_early_stop(
                self._handle(), n, int(patience), float(min_delta), 1 if restore_best else 0,
                None if lrs is None else _p(lrs, C.c_float), None if lams is None else _p(lams, C.c_float),
                _p(val, C.c_double), None if trn is None else _p(trn, C.c_double), C.byref(ran), C.byref(best)))
        finally:
            if self._h:
                self.lr, self.lam = self.hyper()
        return dict(val_rmse=val[:ran.value], train_rmse=None if trn is None else trn[:ran.value],
                    epochs_run=ran.value, best_epoch=best.value)

    # -- online updates (include/mfsgd.h, "online updates") -------------------------
    def partial_fit(self, u, i, r, *, errors=False, info=False, seen=False):
        """Applies the ratings (u[j], i[j], r[j]) to the live model in the order given (mfsgd_apply_ratings): bit for bit
        the sequential per-rating SGD loop, at the current lr and lambda.  The stored ratings, their schedules and the
        held-out set are not touched, and none is needed.  errors=True returns float32[n], each rating's error just
        before its own update ("test, then train"); info=True returns dict(n, pieces, levels, max_width, launches);
        both: (errors, info); neither: None.  seen=True: the applied pairs are then marked in the seen-item index
        (mark_seen), which the update by itself leaves alone."""
        uu, ii, rr = self._triples(u, i, r)
        err = np.empty(uu.size, np.float32) if errors else None
        out = _lib.OnlineInfo()
        self._check(self._lib.mfsgd_apply_ratings(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), _p(rr, C.c_float),
                                                  uu.size, None if err is None else _p(err, C.c_float), C.byref(out)))
        if seen:
            self.mark_seen(uu, ii)
        res = tuple(x for x, on in ((err, errors), (out.as_dict(), info)) if on)
        return None if not res else res[0] if len(res) == 1 else res

    def online_levels(self, u, i):
        """(levels int32[n], dict(n, pieces, levels, max_width, launches = 0)): the dependency level of every rating
        inside its piece of 2^20, as partial_fit would run the list (mfsgd_online_levels).  Host only: needs no GPU, no
        ratings and no factors."""
        uu, ii = _pairs(np.atleast_1d(u), np.atleast_1d(i), "u and i")
        levels = np.empty(uu.size, np.int32)
        out = _lib.OnlineInfo()
        self._check(self._lib.mfsgd_online_levels(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), uu.size,
                                                  _p(levels, C.c_int32), C.byref(out)))
        return levels, out.as_dict()

    # -- pairwise ranking, BPR (include/mfsgd.h, "pairwise ranking") ----------------
    @staticmethod
    def _index_triples(u, i, j):
        uu, ii, jj = _i32(np.atleast_1d(u)), _i32(np.atleast_1d(i)), _i32(np.atleast_1d(j))
        if uu.ndim != 1 or uu.shape != ii.shape or uu.shape != jj.shape:
            raise ValueError("u, i and j must be three 1-d arrays of the same length")
        return uu, ii, jj

    def triple_levels(self, u, i, j):
        """(levels int32[n], dict(n, pieces, levels, max_width, launches = 0)): the dependency level of every triple
        inside its piece of 2^20, as partial_fit_pairwise would run the list (mfsgd_triple_levels).  Host only: needs no
        GPU, no ratings and no factors."""
        uu, ii, jj = self._index_triples(u, i, j)
        levels = np.empty(uu.size, np.int32)
        out = _lib.OnlineInfo()
        self._check(self._lib.mfsgd_triple_levels(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), _p(jj, C.c_int32),
                                                  uu.size, _p(levels, C.c_int32), C.byref(out)))
        return levels, out.as_dict()

    def partial_fit_pairwise(self, u, i, j, *, weights=None, margins=False, info=False):
        """Applies the triples (u[x], i[x], j[x]) -- user, an item the user prefers, an item the user does not -- to the
        live model in the order given, one BPR step each (mfsgd_apply_triples): bit for bit the sequential loop, at the
        current lr and lambda.  i[x] == j[x] is refused.  The stored ratings, their schedules, the held-out set and the
        seen-item index are not touched.  margins=True returns float32[n], each triple's margin dot(p, qi) - dot(p, qj)
        just before its own update; info=True returns dict(n, pieces, levels, max_width, launches); both: (margins,
        info); neither: None.
        weights (float32[n]) gives every step its size instead: s = lr * weights[x] in place of lr * lsig(margin), the
        rest of the step alike (mfsgd_apply_triples_weighted) -- hinge, importance and WARP weights (warp_weights) are the
        caller's policy.  A NaN weight makes its three rows NaN."""
        uu, ii, jj = self._index_triples(u, i, j)
        x = np.empty(uu.size, np.float32) if margins else None
        out = _lib.OnlineInfo()
        if weights is None:
            self._check(self._lib.mfsgd_apply_triples(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), _p(jj, C.c_int32),
                                                      uu.size, None if x is None else _p(x, C.c_float), C.byref(out)))
        else:
            ww = _f32(np.atleast_1d(weights))
            if ww.shape != uu.shape:
                raise ValueError("weights must be a 1-d array as long as u")
            self._check(self._lib.mfsgd_apply_triples_weighted(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32),
                                                               _p(jj, C.c_int32), _p(ww, C.c_float), uu.size,
                                                               None if x is None else _p(x, C.c_float), C.byref(out)))
        return _asked((x, margins), (out.as_dict(), info))

    def _index_and_factors(self, uu, ii):
        """What fit_implicit, fit_bpr and fit_warp start from: a handle without a seen-item index gets set_seen(uu, ii),
        and factors that were never initialised are seeded."""
        if self.seen_size() < 0:
            self.set_seen(uu, ii)
        if not self._initialised:
            self.init_factors()

    def fit_bpr(self, u, i, epochs, *, seed=0, first_epoch=0, stats=True, candidates=1, refresh=None, sampling="uniform",
                candidate_sampling="uniform"):
        """Trains on one-class data with Bayesian personalised ranking: (u[x], i[x]) are the positives, duplicates
        allowed, and every epoch pairs each of them with one freshly drawn item its user has not seen and takes one
        pairwise step per positive, in the order given -- pass the positives shuffled: the order is the caller's, and a
        list sorted by user or item makes long dependency chains and a poor SGD order alike.
        Unseen means unseen by the seen-item index, not by (u, i).  A handle without an index gets set_seen(u, i), and
        keeps it; an index the handle already has is used as it is, so held-out positives put there first are never
        drawn.  Factors that were never initialised are seeded, as in train().
        Epoch e, counted from first_epoch: J = sample_unseen(u, 1, seed, first=e * n); the rows whose draw is -1 (users
        who have seen everything) are dropped for that epoch; partial_fit_pairwise(u, i, J) of the rest.  Seed and epoch
        number alone decide the draws: epochs=a followed by epochs=b, first_epoch=a is epochs=a + b bit for bit.  The
        stored rating set is not touched.
        candidates=m > 1 trains against hard negatives instead (dynamic negative sampling): each positive's negative is
        the best-scoring of m unseen draws under the current factors (sample_unseen_hard), which keeps the steps from
        dying out once most uniform negatives already rank below their positive.  Epoch e walks the positives in blocks
        of `refresh` rows (None: n, one block per epoch); for each block [a, b): J = sample_unseen_hard(u[a:b], m, seed,
        first=e * n * m + a * m) under the factors as the blocks before it left them, rows with -1 dropped,
        partial_fit_pairwise of the rest.  The candidates do not depend on refresh, the picks do; a smaller refresh
        picks against fresher factors and costs a call per block.  Splitting the epochs with first_epoch gives the same
        bits here too.  candidates=1 is the uniform draw above and does not read the factors to draw.
        sampling="weighted" draws every epoch's J with sample_unseen_weighted instead, same counters, in proportion to
        the item weights the handle has (set_item_weights, set_popularity_weights); everything else is as above.  It is
        the spelling for candidates=1 only: with candidates > 1 it is a ValueError.
        candidate_sampling="weighted", with candidates > 1, draws each block's picks with
        sample_unseen_hard(..., sampling="weighted") instead: hard negatives among candidates drawn in proportion to the
        item weights, same counters, rows with -1 (users whose unseen items all weigh nothing) dropped; everything else
        is as above.  It is the spelling for candidates > 1 only: with candidates=1 anything but "uniform" is a
        ValueError, sampling="weighted" being the weighted draw there.  A handle without weights for the items it has
        now is a ValueError too, before the index or the factors are touched.
        Returns, with stats, dict(loss, auc), float64[epochs] each, from the margins x every triple had just before its
        own step: the mean of log1p(exp(-x)), and the share of triples with x > 0.  Without stats: None."""
        uu, ii = _pairs(np.atleast_1d(u), np.atleast_1d(i), "u and i")
        epochs, n, m = int(epochs), uu.size, int(candidates)
        if epochs < 0:
            raise ValueError("epochs must not be negative")
        if m < 1 or (refresh is not None and int(refresh) < 1):
            raise ValueError("candidates and refresh must be at least 1")
        weighted = self._sampling(sampling)
        if weighted and m > 1:
            raise ValueError('sampling="weighted" needs candidates=1')
        if self._sampling(candidate_sampling, "candidate_sampling"):
            if m == 1:
                raise ValueError('candidate_sampling="weighted" needs candidates > 1: with candidates=1 it is sampling="weighted"')
            self._need_item_weights("candidate_sampling")
        draw_into = self._sample_weighted_into if weighted else self._sample_unseen_into
        self._index_and_factors(uu, ii)
        loss, auc = np.zeros(epochs, np.float64), np.zeros(epochs, np.float64)
        if m > 1:
            step = max(n, 1) if refresh is None else int(refresh)
            for e in range(epochs):
                xs = []
                for a in range(0, n, step):
                    bu, bi = uu[a:a + step], ii[a:a + step]
                    J = self.sample_unseen_hard(bu, m, seed, ((int(first_epoch) + e) * n + a) * m, sampling=candidate_sampling)
                    if J.min() < 0:  # users who have seen everything have no negatives
                        keep = J >= 0
                        bu, bi, J = bu[keep], bi[keep], J[keep]
                    xs.append(self.partial_fit_pairwise(bu, bi, J, margins=stats))
                x = np.concatenate(xs).astype(np.float64) if stats and xs else np.empty(0)
                if x.size:
                    loss[e], auc[e] = np.logaddexp(0.0, -x).mean(), (x > 0).mean()
            return dict(loss=loss, auc=auc) if stats else None
        jj = np.empty((n, 1), np.int32)
        for e in range(epochs):
            draw_into(uu, 1, seed, (int(first_epoch) + e) * n, jj)
            J = jj[:, 0]
            if n and J.min() < 0:  # users who have seen everything have no negatives
                keep = J >= 0
                x = self.partial_fit_pairwise(uu[keep], ii[keep], J[keep], margins=stats)
            else:
                x = self.partial_fit_pairwise(uu, ii, J, margins=stats)
            if stats and x.size:
                x = x.astype(np.float64)
                loss[e], auc[e] = np.logaddexp(0.0, -x).mean(), (x > 0).mean()
        return dict(loss=loss, auc=auc) if stats else None

    def fit_warp(self, u, i, epochs, *, candidates=10, margin=1.0, refresh=None, seed=0, first_epoch=0, stats=True,
                 sampling="uniform"):
        """Trains on one-class data with WARP, Weston's weighted approximate-rank pairwise loss: (u[x], i[x]) are the
        positives, in the order given (pass them shuffled, as for fit_bpr).  Each positive's negative is the first of
        m = candidates unseen draws that violates the margin, dot(p, qi) - dot(p, qj) < margin, under the current
        factors (sample_unseen_violating); the number of draws that took estimates the positive's rank, and the step is
        a hinge step of size lr * warp_weights(rank): large where a violator turns up at once, small where it takes
        many draws, none where none of the m violates.  The index and the factors are handled as in fit_bpr: a handle
        without an index gets set_seen(u, i), factors that were never initialised are seeded.
        Epoch e, counted from first_epoch, walks the positives in blocks of `refresh` rows (None: n, one block per
        epoch); for each block [a, b): J, d, rk = sample_unseen_violating(u[a:b], i[a:b], m, margin, seed,
        first=((first_epoch + e) * n + a) * m, draws=True, ranks=True) under the factors as the blocks before it left
        them; the rows with J < 0 (no violator, or nothing unseen) are dropped;
        partial_fit_pairwise(..., weights=warp_weights(rk)) of the rest.  Splitting the epochs with first_epoch gives
        the same bits as one run.  The stored rating set is not touched.
        sampling="weighted" draws every block with sample_unseen_violating(..., sampling="weighted") instead: the
        candidates come in proportion to the item weights the handle has (set_item_weights, set_popularity_weights),
        same counters; everything else is as above.  A handle without weights for the items it has now is a
        ValueError, before the index or the factors are touched.
        Returns, with stats, dict(violating, trials), float64[epochs] each: the share of positives that had a violator,
        and the mean of d + 1 over those positives (0 where there were none).  Without stats: None."""
        uu, ii = _pairs(np.atleast_1d(u), np.atleast_1d(i), "u and i")
        epochs, n, m = int(epochs), uu.size, int(candidates)
        if epochs < 0:
            raise ValueError("epochs must not be negative")
        if m < 1 or (refresh is not None and int(refresh) < 1):
            raise ValueError("candidates and refresh must be at least 1")
        if np.isnan(margin):
            raise ValueError("margin must not be NaN")
        if self._sampling(sampling):
            self._need_item_weights("sampling")
        self._index_and_factors(uu, ii)
        violating, trials = np.zeros(epochs, np.float64), np.zeros(epochs, np.float64)
        step = max(n, 1) if refresh is None else int(refresh)
        for e in range(epochs):
            hits = draws = 0
            for a in range(0, n, step):
                bu, bi = uu[a:a + step], ii[a:a + step]
                J, d, rk = self.sample_unseen_violating(bu, bi, m, margin, seed, ((int(first_epoch) + e) * n + a) * m,
                                                        draws=True, ranks=True, sampling=sampling)
                keep = J >= 0
                self.partial_fit_pairwise(bu[keep], bi[keep], J[keep], weights=warp_weights(rk[keep]))
                hits += int(keep.sum())
                draws += int(d[keep].astype(np.int64).sum()) + int(keep.sum())
            if n:
                violating[e] = hits / n
            if hits:
                trials[e] = draws / hits
        return dict(violating=violating, trials=trials) if stats else None

    def train_timed(self, epochs):
        """(elapsed device milliseconds, kernel launches) for `epochs` passes."""
        ms = C.c_double()
        launches = C.c_int64()
        self._check(self._lib.mfsgd_train_timed(self._handle(), int(epochs), C.byref(ms), C.byref(launches)))
        return ms.value, launches.value

    def rmse(self):
        out = C.c_double()
        self._check(self._lib.mfsgd_rmse(self._handle(), C.byref(out)))
        return out.value

    def predict(self, u, i):
        scalar = np.isscalar(u) and np.isscalar(i)
        uu, ii = _i32(np.atleast_1d(u)), _i32(np.atleast_1d(i))
        if uu.shape != ii.shape or uu.ndim != 1:
            raise ValueError("u and i must have the same 1-d shape")
        out = np.empty(uu.size, np.float32)
        self._check(self._lib.mfsgd_predict(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32),
                                            _p(out, C.c_float), uu.size))
        return float(out[0]) if scalar else out

    def recommend(self, users, topn, exclude=None, candidates=None):
        """(items, scores), each [len(users), topn]: best items per user, best first.  exclude = (u, i):
        pairs never returned (for instance the training ratings, so that only unrated items come back);
        a row with fewer than topn eligible items is padded with item -1 and score NaN.  exclude = "seen": the pairs of
        the seen-item index (set_seen / mark_seen), read on the device where they lie -- the same rows, without the list.
        candidates: the items a row may return at all (mfsgd_recommend_among) -- a 1-d integer array, one list for every
        row; a tuple (ptr, items), CSR over the rows of `users` (row b is the position in users, not the user); or a
        sequence of one 1-d array per row.  Lists may be unsorted, repeat items and be empty.  None: every item."""
        lib = self._lib
        return self._top_n((lib.mfsgd_recommend_excluding, lib.mfsgd_recommend_among, lib.mfsgd_recommend_unseen,
                            lib.mfsgd_recommend_unseen_among), _i32(np.atleast_1d(users)), _exclusions(exclude), candidates, topn)

    def _top_n(self, family, request, exclusions, candidates, topn):
        """The one call behind recommend, recommend_users and their _rows forms: (ids, scores), each [n, topn].  family: the
        C functions (plain, among, unseen, unseen among) -- the _rows families have no unseen forms; request: the ids asked
        for (int32; n is their number) or dense rows (float32, n x k); exclusions: (seen, a, b) as _exclusions returns it,
        the pairs in the order the family takes them; candidates: the caller's, in any of the three forms, or None."""
        rows = request.dtype == np.float32
        n = request.shape[0] if rows else request.size
        seen, ea, eb = exclusions
        cp, cc = (None, None) if candidates is None else _candidates(candidates, n)
        ids = np.empty((n, int(topn)), np.int32)
        scores = np.empty((n, int(topn)), np.float32)
        args = [self._handle(), _p(request, C.c_float if rows else C.c_int32), n, int(topn)]
        if candidates is not None:
            args += [None if cp is None else _p(cp, C.c_int64), _p(cc, C.c_int32), cc.size]
        if not seen:
            args += [_p(ea, C.c_int32), _p(eb, C.c_int32), ea.size]
        self._check(family[2 * seen + (candidates is not None)](*args, _p(ids, C.c_int32), _p(scores, C.c_float)))
        return ids, scores

    def recommend_users(self, items, topn, exclude=None, candidates=None):
        """(users, scores), each [len(items), topn]: the best audience of each item, best first -- recommend() with the
        two sides exchanged (mfsgd_recommend_users); the scores are the bits predict(user, item) returns, equal scores go
        to the smaller user.  exclude = (u, i): the same (user, item) pairs recommend() takes; user u[x] is never
        returned for item i[x], and a row with fewer than topn eligible users is padded with user -1 and score NaN.
        exclude = "seen": the pairs of the seen-item index -- the same rows, without the list; the index is by user, so
        each call reads all of it once on the device to find the requested items' users.
        candidates: the users a row may return at all ("the best 100 of this segment", mfsgd_recommend_users_among), in
        the three forms recommend() takes, the per-row forms indexing `items`.  None: every user."""
        lib = self._lib
        return self._top_n((lib.mfsgd_recommend_users, lib.mfsgd_recommend_users_among, lib.mfsgd_recommend_users_unseen,
                            lib.mfsgd_recommend_users_unseen_among), _i32(np.atleast_1d(items)), _exclusions(exclude), candidates,
                           topn)

    # -- the seen-item index (include/mfsgd.h, "the seen-item index") ---------------
    def set_seen(self, u, i):
        """The seen-item index becomes the distinct pairs (u[x], i[x]) (mfsgd_set_seen): built once on the device and kept
        there, so that exclude="seen" serves "items this user has not seen" without the list.  Empty arrays leave an
        empty index (no GPU needed)."""
        uu, ii = _pairs(np.atleast_1d(u), np.atleast_1d(i), "u and i")
        self._check(self._lib.mfsgd_set_seen(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), uu.size))

    def mark_seen(self, u, i):
        """Adds the pairs to the seen-item index (mfsgd_mark_seen): a merge on the device, the index is not sorted again.
        Without an index it is set_seen."""
        uu, ii = _pairs(np.atleast_1d(u), np.atleast_1d(i), "u and i")
        self._check(self._lib.mfsgd_mark_seen(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), uu.size))

    def clear_seen(self):
        """Drops the seen-item index and frees its device memory: the handle has none afterwards."""
        self._check(self._lib.mfsgd_clear_seen(self._handle()))

    def seen_size(self):
        """Distinct pairs in the seen-item index; -1 when the handle has none."""
        n = C.c_int64(-2)
        self._check(self._lib.mfsgd_seen_size(self._handle(), C.byref(n)))
        return n.value

    def seen(self, users):
        """(row_ptr int64[len(users) + 1], items int32[row_ptr[-1]]): the seen items of the requested users, ascending
        within a user, CSR over `users` as given (mfsgd_get_seen: gathered on the device)."""
        uu = _users(users)
        ptr = np.zeros(uu.size + 1, np.int64)
        self._check(self._lib.mfsgd_get_seen(self._handle(), _p(uu, C.c_int32), uu.size, _p(ptr, C.c_int64), None, 0))
        items = np.empty(int(ptr[-1]), np.int32)
        if items.size:
            self._check(self._lib.mfsgd_get_seen(self._handle(), _p(uu, C.c_int32), uu.size, _p(ptr, C.c_int64),
                                                 _p(items, C.c_int32), items.size))
        return ptr, items

    # -- implicit feedback: negatives sampled off the seen-item index -----------------
    def sample_unseen(self, users, m=1, seed=0, first=0):
        """int32 [len(users), m]: for each row, m items drawn uniformly (with replacement) among those the row's user has
        not seen according to the seen-item index (mfsgd_sample_unseen: one device thread per draw, exact, no rejection);
        -1 throughout a row whose user has seen every item.  Draw d of row x is a pure function of seed, the counter
        first + x * m + d, the user's list and the item count: rows [a:b] of a call are the call on users[a:b] with
        first + a * m."""
        uu = _users(users)
        out = np.empty((uu.size, max(int(m), 0)), np.int32)
        self._sample_unseen_into(uu, m, seed, first, out)
        return out

    def _sample_unseen_into(self, uu, m, seed, first, out):
        """sample_unseen(uu, ...) into `out`, a C-contiguous int32 array of uu.size * m entries."""
        self._check(self._lib.mfsgd_sample_unseen(self._handle(), _p(uu, C.c_int32), uu.size, int(m), int(seed), int(first),
                                                  _p(out, C.c_int32)))

    # -- weighted negatives (include/mfsgd.h, "weighted negatives") ------------------
    def set_item_weights(self, w):
        """The item weights of sample_unseen_weighted become w, one integer in [0, 2^32) per item of the model
        (mfsgd_set_item_weights): an item of weight 0 is never drawn.  They belong to the items and outlive set_seen,
        mark_seen and clear_seen; after add_items they must be set again before the next weighted draw."""
        ww = np.atleast_1d(np.asarray(w))
        if ww.ndim != 1 or (ww.size and ww.dtype.kind not in "iu"):
            raise ValueError("w must be a 1-d integer array")
        if ww.size and (int(ww.min()) < 0 or int(ww.max()) > 0xFFFFFFFF):
            raise ValueError("weights must lie in [0, 2^32)")
        ww = np.ascontiguousarray(ww, dtype=np.uint32)
        self._check(self._lib.mfsgd_set_item_weights(self._handle(), _p(ww, C.c_uint32), ww.size))

    def item_weights(self):
        """uint32 weights as set (for the item count they were set for), or None when the handle has none."""
        n = C.c_int32(-2)
        self._check(self._lib.mfsgd_get_item_weights(self._handle(), None, C.byref(n)))
        if n.value < 0:
            return None
        w = np.empty(n.value, np.uint32)
        self._check(self._lib.mfsgd_get_item_weights(self._handle(), _p(w, C.c_uint32), C.byref(n)))
        return w

    def clear_item_weights(self):
        """Drops the item weights and what the index keeps for them; the handle has none afterwards."""
        self._check(self._lib.mfsgd_clear_item_weights(self._handle()))

    def seen_item_counts(self):
        """int64 [items]: the number of users whose seen list holds each item (mfsgd_seen_item_counts: a histogram on the
        device) -- the popularity that popularity_weights turns into weights."""
        counts = np.empty(self.items, np.int64)
        self._check(self._lib.mfsgd_seen_item_counts(self._handle(), _p(counts, C.c_int64)))
        return counts

    def set_popularity_weights(self, alpha=0.75, resolution=16, least=1):
        """set_item_weights(popularity_weights(seen_item_counts(), alpha, resolution, least))."""
        self.set_item_weights(popularity_weights(self.seen_item_counts(), alpha, resolution, least))

    def sample_unseen_weighted(self, users, m=1, seed=0, first=0, *, mass=False):
        """sample_unseen with every unseen item drawn in proportion to its weight (mfsgd_sample_unseen_weighted: exact,
        integers only, no rejection): int32 [len(users), m], -1 throughout a row whose user has seen every item of
        positive weight.  Draw d of row x is a pure function of seed, the counter first + x * m + d, the user's list, the
        weights and the item count.  mass=True adds int64 [len(users)], each row's unseen weight (written where m > 0)."""
        uu = _users(users)
        out = np.empty((uu.size, max(int(m), 0)), np.int32)
        ms = np.zeros(uu.size, np.int64) if mass else None
        self._sample_weighted_into(uu, m, seed, first, out, ms)
        return (out, ms) if mass else out

    def _sample_weighted_into(self, uu, m, seed, first, out, mass=None):
        """sample_unseen_weighted(uu, ...) into `out`, a C-contiguous int32 array of uu.size * m entries."""
        self._check(self._lib.mfsgd_sample_unseen_weighted(self._handle(), _p(uu, C.c_int32), uu.size, int(m), int(seed),
                                                           int(first), _p(out, C.c_int32),
                                                           None if mass is None else _p(mass, C.c_int64)))

    @staticmethod
    def _sampling(sampling, keyword="sampling"):
        if sampling not in ("uniform", "weighted"):
            raise ValueError(keyword + ' must be "uniform" or "weighted"')
        return sampling == "weighted"

    def _need_item_weights(self, keyword):
        """What fit_bpr and fit_warp ask before they touch anything for a weighted keyword: weights, set for the items
        the model has now (the draw itself would refuse only after the index and the factors were made)."""
        n = C.c_int32(-2)
        self._check(self._lib.mfsgd_get_item_weights(self._handle(), None, C.byref(n)))
        if n.value < 0:
            raise ValueError(keyword + '="weighted" needs item weights: set_item_weights or set_popularity_weights first')
        self._dims()
        if n.value != self.items:
            raise ValueError(keyword + f'="weighted": the item weights cover {n.value} items, the model has {self.items}')

    @classmethod
    def _sampling_mass(cls, sampling, mass):
        """The weighted flag of a pick call, whose mass=True is the weighted call's alone."""
        weighted = cls._sampling(sampling)
        if mass and not weighted:
            raise ValueError('mass=True needs sampling="weighted"')
        return weighted

    def sample_unseen_hard(self, users, m, seed=0, first=0, *, scores=False, draws=False, sampling="uniform", mass=False):
        """int32 [len(users)]: for each row, the best-scoring of the m items sample_unseen(users, m, seed, first) draws for
        it, under the factors as they are now (mfsgd_sample_unseen_hard: drawn, scored and picked on the device, nothing
        per candidate comes down).  The score is predict's; equal scores go to the earlier draw, a NaN score loses to
        every number; -1 for a user who has seen every item.  scores=True adds float32 [len(users)], each pick's score
        (NaN with -1); draws=True adds int32 [len(users)], each pick's position d in its row of draws (-1 with -1); with
        either the result is a tuple (items, scores, draws) without what was not asked for.
        sampling="weighted": the candidates are sample_unseen_weighted(users, m, seed, first)'s instead, drawn in
        proportion to the item weights the handle has (mfsgd_sample_unseen_hard_weighted); -1 for a user whose unseen
        items all weigh nothing.  mass=True (weighted only: a ValueError otherwise) adds int64 [len(users)], each row's
        unseen weight, at the end of the tuple."""
        weighted = self._sampling_mass(sampling, mass)
        uu = _users(users)
        items = np.empty(uu.size, np.int32)
        sc = np.empty(uu.size, np.float32) if scores else None
        dr = np.empty(uu.size, np.int32) if draws else None
        ms = np.zeros(uu.size, np.int64) if mass else None
        args = (self._handle(), _p(uu, C.c_int32), uu.size, int(m), int(seed), int(first), _p(items, C.c_int32),
                None if sc is None else _p(sc, C.c_float), None if dr is None else _p(dr, C.c_int32))
        if weighted:
            self._check(self._lib.mfsgd_sample_unseen_hard_weighted(*args, None if ms is None else _p(ms, C.c_int64)))
        else:
            self._check(self._lib.mfsgd_sample_unseen_hard(*args))
        return _asked((items, True), (sc, scores), (dr, draws), (ms, mass))

    def sample_unseen_violating(self, users, items, m, margin=1.0, seed=0, first=0, *, draws=False, margins=False, ranks=False,
                                sampling="uniform", mass=False):
        """int32 [len(users)]: for each row, the first of the m items sample_unseen(users, m, seed, first) draws for it
        that is not the row's positive items[x] and violates the margin against it, dot(p, q_pos) - dot(p, q_cand) <
        margin, under the factors as they are now (mfsgd_sample_unseen_violating: drawn, scored and picked on the device,
        the draws past the pick skipped); -1 where none of the m does, or the user has seen every item.  A NaN
        difference never violates, one equal to the margin does not.  draws=True adds int32 [len(users)], each pick's
        position d (m where no candidate violates, -1 where nothing is unseen); margins=True adds float32, the pick's
        difference (NaN with -1): what partial_fit_pairwise reports as its margin; ranks=True adds int32, the estimate
        max(1, unseen items // (d + 1)) of how many unseen items violate (0 with -1): what warp_weights takes.  With
        any of them the result is a tuple (items, draws, margins, ranks) without what was not asked for.
        sampling="weighted": the candidates are sample_unseen_weighted(users, m, seed, first)'s instead
        (mfsgd_sample_unseen_violating_weighted); -1, and a draw of -1, for a user whose unseen items all weigh nothing;
        the rank still scales by the number of unseen items.  mass=True (weighted only: a ValueError otherwise) adds
        int64 [len(users)], each row's unseen weight, at the end of the tuple."""
        weighted = self._sampling_mass(sampling, mass)
        uu, ii = _pairs(np.atleast_1d(users), np.atleast_1d(items), "users and items")
        out = np.empty(uu.size, np.int32)
        dr = np.empty(uu.size, np.int32) if draws else None
        mg = np.empty(uu.size, np.float32) if margins else None
        rk = np.empty(uu.size, np.int32) if ranks else None
        ms = np.zeros(uu.size, np.int64) if mass else None
        args = (self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), uu.size, int(m), float(margin), int(seed), int(first),
                _p(out, C.c_int32), None if dr is None else _p(dr, C.c_int32), None if mg is None else _p(mg, C.c_float),
                None if rk is None else _p(rk, C.c_int32))
        if weighted:
            self._check(self._lib.mfsgd_sample_unseen_violating_weighted(*args, None if ms is None else _p(ms, C.c_int64)))
        else:
            self._check(self._lib.mfsgd_sample_unseen_violating(*args))
        return _asked((out, True), (dr, draws), (mg, margins), (rk, ranks), (ms, mass))

    def fit_implicit(self, u, i, epochs, negatives=4, *, seed=0, pos=1.0, neg=0.0, first_epoch=0, rmse=True, sampling="uniform"):
        """Trains on one-class data (clicks, plays, purchases): (u[x], i[x]) are the positives, duplicates allowed, and
        every epoch pairs each of them with `negatives` freshly drawn items its user has not seen, trained towards `neg`.
        Unseen means unseen by the seen-item index, not by (u, i).  A handle without an index gets set_seen(u, i), and
        keeps it (recommend(exclude="seen") wants it afterwards); an index the handle already has is used as it is, so a
        caller who puts held-out positives into it first never trains them as negatives.  Factors that were never
        initialised are seeded, as in train().
        Epoch e, counted from first_epoch: J = sample_unseen(u, negatives, seed, first=e * n * negatives); the rating set
        is the positives in the order given at `pos`, then (u[x], J[x, d], neg) in row-major order without the -1 of
        users who have seen everything; set_ratings of that set, fit(1).  Seed and epoch number alone decide the draws:
        epochs=a followed by epochs=b, first_epoch=a is epochs=a + b bit for bit.  negatives=0: one set_ratings of the
        positives and fit(epochs).  Returns the RMSE of each epoch over that epoch's own set (None with rmse=False);
        the last epoch's set stays the handle's rating set.
        sampling="weighted" draws every epoch's J with sample_unseen_weighted instead, same counters, in proportion to
        the item weights the handle has (set_item_weights, set_popularity_weights); everything else is as above."""
        uu, ii = _pairs(np.atleast_1d(u), np.atleast_1d(i), "u and i")
        epochs, negatives, n = int(epochs), int(negatives), uu.size
        if epochs < 0 or negatives < 0:
            raise ValueError("epochs and negatives must not be negative")
        draw_into = self._sample_weighted_into if self._sampling(sampling) else self._sample_unseen_into
        self._index_and_factors(uu, ii)
        rr = np.full(n, pos, np.float32)
        if negatives == 0:
            self.set_ratings(uu, ii, rr)
            return self.fit(epochs, rmse=rmse)
        # the set of an epoch is laid out once: the draws come down into the items' tail, where set_ratings reads them
        set_u, set_i = np.concatenate([uu, np.repeat(uu, negatives)]), np.concatenate([ii, np.empty(n * negatives, np.int32)])
        set_r = np.concatenate([rr, np.full(n * negatives, neg, np.float32)])
        out = np.zeros(epochs, np.float64)
        for x in range(epochs):
            draw_into(uu, negatives, seed, (int(first_epoch) + x) * n * negatives, set_i[n:])
            if n and set_i[n:].min() < 0:  # users who have seen everything have no negatives
                keep = np.concatenate([np.ones(n, bool), set_i[n:] >= 0])
                self.set_ratings(set_u[keep], set_i[keep], set_r[keep])
            else:
                self.set_ratings(set_u, set_i, set_r)
            got = self.fit(1, rmse=rmse)
            if rmse:
                out[x] = got[0]
        return out if rmse else None

    def serve_seconds(self):
        """(lists, topn): host seconds the latest recommend call spent building its candidate and exclusion lists on the
        device, and scoring and selecting (mfsgd_debug_serve_seconds)."""
        out = np.zeros(2, np.float64)
        self._check(self._lib.mfsgd_debug_serve_seconds(self._handle(), _p(out, C.c_double)))
        return float(out[0]), float(out[1])

    def _fold_in(self, call, row_ptr, ids, ratings, epochs, init, seed, what):
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ii, rr = _i32(ids), _f32(ratings)
        if rp.ndim != 1 or rp.size < 1:
            raise ValueError("row_ptr must be a 1-d array of n_new + 1 offsets")
        n_new = rp.size - 1
        if ii.ndim != 1 or ii.shape != rr.shape or ii.size != rp[-1]:
            raise ValueError(f"{what} and ratings must be 1-d arrays of row_ptr[-1] entries")
        ip = None
        if init is not None:
            init = _f32(init)
            if init.shape != (n_new, self.k):
                raise ValueError("init must be n_new x k")
            ip = _p(init, C.c_float)
        rows = np.empty((n_new, self.k), np.float32)
        self._check(call(self._handle(), n_new, _p(rp, C.c_int64), _p(ii, C.c_int32), _p(rr, C.c_float), int(epochs), ip,
                         self.seed if seed is None else int(seed), _p(rows, C.c_float)))
        return rows

    def fold_in(self, row_ptr, items, ratings, epochs, init=None, seed=None):
        """Rows [n_new, k] for users that are not in the model: new user x owns ratings row_ptr[x] .. row_ptr[x + 1]
        of items / ratings (CSR), and `epochs` passes of the per-rating SGD step run over them against the model's
        item factors, which stay fixed.  init: start rows [n_new, k]; None: seeded rows (seed None: the model's),
        those init_factors(seed) would give a model of n_new users.  The model is not modified."""
        return self._fold_in(self._lib.mfsgd_fold_in_users, row_ptr, items, ratings, epochs, init, seed, "items")

    def fold_in_items(self, row_ptr, users, ratings, epochs, init=None, seed=None):
        """fold_in() for items that are not in the model (mfsgd_fold_in_items): new item x owns ratings row_ptr[x] ..
        row_ptr[x + 1] of users / ratings, and the step runs against the model's user factors, which stay fixed.  The
        seeded start rows are fold_in()'s.  The model is not modified; add_items(rows) puts the rows into it."""
        return self._fold_in(self._lib.mfsgd_fold_in_items, row_ptr, users, ratings, epochs, init, seed, "users")

    # -- least-squares fold-in and ALS (include/mfsgd.h, "least-squares fold-in") -------
    def gram(self, side):
        """float32[k, k]: the Gram matrix P^T P (side "users") or Q^T Q ("items") by the rule of mfsgd_gram -- the
        alpha term of the implicit fold-in's system."""
        code, _ = self._side(side)
        out = np.empty((self.k, self.k), np.float32)
        self._check(self._lib.mfsgd_gram(self._handle(), code, _p(out, C.c_float)))
        return out

    def _fold_in_solve(self, side, row_ptr, ids, a, b, alpha, ridge, ridge_per_entry, status, what):
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ii, bb = _i32(ids), _f32(b)
        if rp.ndim != 1 or rp.size < 1:
            raise ValueError("row_ptr must be a 1-d array of n_new + 1 offsets")
        n_new = rp.size - 1
        if ii.ndim != 1 or ii.shape != bb.shape or ii.size != rp[-1]:
            raise ValueError(f"{what} must be 1-d arrays of row_ptr[-1] entries")
        ap = None
        if a is not None:
            a = _f32(a)
            if a.shape != ii.shape:
                raise ValueError(f"{what} must be 1-d arrays of row_ptr[-1] entries")
            ap = _p(a, C.c_float)
        rows = np.empty((n_new, self.k), np.float32)
        st = np.zeros(n_new, np.int32)
        self._check(self._lib.mfsgd_fold_in_solve(self._handle(), side, n_new, _p(rp, C.c_int64), _p(ii, C.c_int32), ap,
                                                  _p(bb, C.c_float), float(alpha), float(ridge), float(ridge_per_entry),
                                                  _p(rows, C.c_float), _p(st, C.c_int32)))
        return (rows, st) if status else rows

    def _fold_in_exact(self, side, row_ptr, ids, ratings, lam, weights, status, what):
        rr = _f32(ratings)
        a = None
        if weights is not None:
            a = _f32(weights)
            if a.shape != rr.shape:
                raise ValueError(f"{what} must be 1-d arrays of row_ptr[-1] entries")
            rr = a * rr  # one fp32 multiply
        return self._fold_in_solve(side, row_ptr, ids, a, rr, 0.0, 0.0, self.lam if lam is None else lam, status, what)

    def fold_in_exact(self, row_ptr, items, ratings, lam=None, weights=None, status=False):
        """fold_in() without a learning rate, epochs or start rows: row x is the minimiser of
        sum_j w_j (r_j - x . q_j)^2 + lam * len * |x|^2 over the user's list -- the fixed point fold_in()'s chain
        converges to -- found by solving its k x k system on the device (mfsgd_fold_in_solve, bit for bit the rule
        in include/mfsgd.h).  lam None: the handle's lambda; weights None: all 1.  A user without ratings gets zeros.
        status=True: (rows, status), status[x] 0 or the 1-based pivot at which the system of row x turned out not
        positive definite (its row is NaN then).  The model is not modified."""
        return self._fold_in_exact(0, row_ptr, items, ratings, lam, weights, status, "items, ratings and weights")

    def fold_in_items_exact(self, row_ptr, users, ratings, lam=None, weights=None, status=False):
        """fold_in_exact() for items that are not in the model, against the model's user factors."""
        return self._fold_in_exact(1, row_ptr, users, ratings, lam, weights, status, "users, ratings and weights")

    def _fold_in_implicit(self, side, row_ptr, ids, confidence, lam, unobserved, status, what):
        c = _f32(confidence)
        return self._fold_in_solve(side, row_ptr, ids, c - np.float32(unobserved), c, unobserved, lam, 0.0, status, what)

    def fold_in_implicit(self, row_ptr, items, confidence, lam, unobserved=1.0, status=False):
        """Rows for new users of a one-class model (fit_implicit with pos=1, neg=0; fit_ials): the minimiser of
        sum_observed c_j (1 - x . q_j)^2 + unobserved * sum_rest (x . q)^2 + lam * |x|^2, the implicit-feedback
        fold-in of Hu, Koren and Volinsky ("recalculate_user" elsewhere).  confidence: c_j of each named item.  The
        sum over everything unobserved costs one Gram matrix of Q per call.  status as in fold_in_exact()."""
        return self._fold_in_implicit(0, row_ptr, items, confidence, lam, unobserved, status, "items and confidence")

    def fold_in_items_implicit(self, row_ptr, users, confidence, lam, unobserved=1.0, status=False):
        """fold_in_implicit() for items that are not in the model, against the model's user factors."""
        return self._fold_in_implicit(1, row_ptr, users, confidence, lam, unobserved, status, "users and confidence")

    def _als(self, u, i, weights, sweeps, fold_users, fold_items, objective):
        """The alternation fit_als and fit_ials share: CSR by user and by item in the order given (a stable sort), then
        per sweep P from every user's list against Q, Q from every item's list against the new P."""
        uu, ii = _pairs(u, i, "u and i")
        if not self._initialised:
            self.init_factors()
        by_u, by_i = np.argsort(uu, kind="stable"), np.argsort(ii, kind="stable")
        ptr_u = np.concatenate([[0], np.cumsum(np.bincount(uu, minlength=self.users))]).astype(np.int64)
        ptr_i = np.concatenate([[0], np.cumsum(np.bincount(ii, minlength=self.items))]).astype(np.int64)
        P, Q = self.get_factors()
        out = np.zeros(2 * int(sweeps), np.float64)
        for s in range(int(sweeps)):
            for half, (fold, ptr, order, ids) in enumerate(((fold_users, ptr_u, by_u, ii), (fold_items, ptr_i, by_i, uu))):
                rows, st = fold(ptr, ids[order], weights[order])
                if st.any():
                    x = int(np.flatnonzero(st)[0])
                    raise MfsgdError(-1, f"the system of {'item' if half else 'user'} {x} is not positive definite "
                                         f"(pivot {int(st[x])}): raise lam")
                P, Q = (P, rows) if half else (rows, Q)
                self.set_factors(P, Q)
                out[2 * s + half] = objective(P, Q)
        return out

    def fit_als(self, u, i, r, sweeps, lam=None):
        """Alternating least squares on ratings (ALS-WR): each sweep replaces every row of P by fold_in_exact() of that
        user's ratings against Q, then every row of Q by fold_in_items_exact() of that item's ratings against the new
        P.  Inside a list the ratings keep the order given.  Factors that were never initialised are seeded, as in
        train().  Returns float64[2 * sweeps]: after each half-sweep the objective
        sum (r - p . q)^2 + lam * sum_u n_u |p_u|^2 + lam * sum_i n_i |q_i|^2, in fp64 on the host.  A user or item
        without ratings gets a zero row.  MfsgdError when a system is not positive definite."""
        lam = self.lam if lam is None else float(lam)
        uu, ii = _pairs(u, i, "u and i")
        rr = _f32(r)
        if rr.shape != uu.shape:
            raise ValueError("u, i and r must be 1-d arrays of the same length")
        nu, ni = np.bincount(uu, minlength=self.users), np.bincount(ii, minlength=self.items)

        def objective(P, Q):
            P, Q = P.astype(np.float64), Q.astype(np.float64)
            e = rr.astype(np.float64) - np.einsum("ij,ij->i", P[uu], Q[ii])
            return float(e @ e) + lam * float(nu @ (P * P).sum(1)) + lam * float(ni @ (Q * Q).sum(1))

        return self._als(uu, ii, rr, sweeps, lambda ptr, ids, w: self.fold_in_exact(ptr, ids, w, lam, status=True),
                         lambda ptr, ids, w: self.fold_in_items_exact(ptr, ids, w, lam, status=True), objective)

    def fit_ials(self, u, i, sweeps, confidence=41.0, lam=None, unobserved=1.0):
        """Alternating least squares on one-class data (iALS, Hu, Koren and Volinsky): fit_als() with fold_in_implicit()
        and fold_in_items_implicit().  confidence: c of every positive, one number or one per pair.  Returns
        float64[2 * sweeps]: after each half-sweep
        sum_j c_j (1 - s_j)^2 + unobserved * (|P Q^T|_F^2 - sum_j s_j^2) + lam * (|P|_F^2 + |Q|_F^2), s_j = p . q of
        pair j, in fp64 on the host -- what both half-sweeps minimise."""
        lam = self.lam if lam is None else float(lam)
        uu, ii = _pairs(u, i, "u and i")
        cc = np.ascontiguousarray(np.broadcast_to(_f32(confidence), uu.shape))
        un = float(unobserved)

        def objective(P, Q):
            P, Q = P.astype(np.float64), Q.astype(np.float64)
            s = np.einsum("ij,ij->i", P[uu], Q[ii])
            rest = float(((P.T @ P) * (Q.T @ Q)).sum()) - float(s @ s)
            return float(cc.astype(np.float64) @ ((1.0 - s) ** 2)) + un * rest + lam * (float((P * P).sum()) + float((Q * Q).sum()))

        return self._als(uu, ii, cc, sweeps, lambda ptr, ids, c: self.fold_in_implicit(ptr, ids, c, lam, un, status=True),
                         lambda ptr, ids, c: self.fold_in_items_implicit(ptr, ids, c, lam, un, status=True), objective)

    def fold_in_pairwise(self, row_ptr, items, epochs, *, candidates=1, init=None, seed=None, draw_seed=0, first=0,
                         margins=False, negatives=False, sampling="uniform"):
        """Rows [n_new, k] for users that are not in a model trained by fit_bpr or fit_warp, from their positives alone
        (mfsgd_fold_in_users_pairwise): new user x owns the positives items[row_ptr[x] .. row_ptr[x + 1]) (CSR), and
        `epochs` passes of the BPR step run over them against the model's item factors, which stay fixed.  Every step
        draws `candidates` items the user has not named -- sample_unseen's draws for draw_seed and the counters from
        first + row_ptr[x] * epochs * candidates on -- and takes the one the row scores highest (sample_unseen_hard's
        pick; candidates=1: the draw).  init and seed: the start rows, as in fold_in().  margins=True adds float32
        [row_ptr[-1] * epochs], each step's margin before it; negatives=True adds int32 of that shape, each step's
        negative; with either the result is a tuple (rows, margins, negatives) without what was not asked for.  A user
        who names every item takes no step (NaN and -1).  The model is not modified; the rows feed recommend_rows,
        rank_items_rows and add_users.
        sampling="weighted": the draws are sample_unseen_weighted's instead, in proportion to the item weights the
        handle has (mfsgd_fold_in_users_pairwise_weighted) -- the objective of a model trained with weighted negatives;
        a user who names every item of positive weight takes no step."""
        call = (self._lib.mfsgd_fold_in_users_pairwise_weighted if self._sampling(sampling)
                else self._lib.mfsgd_fold_in_users_pairwise)
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        ii = _i32(items)
        if rp.ndim != 1 or rp.size < 1:
            raise ValueError("row_ptr must be a 1-d array of n_new + 1 offsets")
        n_new = rp.size - 1
        if ii.ndim != 1 or ii.size != rp[-1]:
            raise ValueError("items must be a 1-d array of row_ptr[-1] entries")
        ip = None
        if init is not None:
            init = _f32(init)
            if init.shape != (n_new, self.k):
                raise ValueError("init must be n_new x k")
            ip = _p(init, C.c_float)
        steps = int(rp[-1]) * max(int(epochs), 0)
        rows = np.empty((n_new, self.k), np.float32)
        mg = np.empty(steps, np.float32) if margins else None
        ng = np.empty(steps, np.int32) if negatives else None
        self._check(call(self._handle(), n_new, _p(rp, C.c_int64), _p(ii, C.c_int32), int(epochs), int(candidates), ip,
                         self.seed if seed is None else int(seed), int(draw_seed), int(first), _p(rows, C.c_float),
                         None if mg is None else _p(mg, C.c_float), None if ng is None else _p(ng, C.c_int32)))
        return _asked((rows, True), (mg, margins), (ng, negatives))

    # -- growing a live model (include/mfsgd.h, "growing a live model") -------------
    def _dims(self):
        u, i = C.c_int32(), C.c_int32()
        self._check(self._lib.mfsgd_get_dims(self._handle(), C.byref(u), C.byref(i), None))
        self.users, self.items = u.value, i.value

    def _append(self, call, rows, n, seed):
        if (rows is None) == (n is None):
            raise ValueError("give either rows or n")
        rp = None
        if rows is not None:
            rows = _f32(rows)
            if rows.ndim != 2 or rows.shape[1] != self.k:
                raise ValueError("rows must be n_new x k")
            n, rp = rows.shape[0], _p(rows, C.c_float)
        first = C.c_int32(-1)
        try:
            self._check(call(self._handle(), int(n), rp, self.seed if seed is None else int(seed), C.byref(first)))
        finally:
            if self._h:
                self._dims()
        return first.value

    def add_users(self, rows=None, *, n=None, seed=None):
        """Appends users to the live model (mfsgd_append_users) and returns the index of the first: rows [n_new, k] (for
        instance what fold_in returned), or n seeded rows (seed None: the model's) -- fold_in's default start rows.
        Nothing is rebuilt: the stored ratings, their schedules and order, the held-out set and the old rows stay as
        they are, and with the factors on the device no old row leaves it."""
        return self._append(self._lib.mfsgd_append_users, rows, n, seed)

    def add_items(self, rows=None, *, n=None, seed=None):
        """add_users() for items (mfsgd_append_items); rows: for instance what fold_in_items returned."""
        return self._append(self._lib.mfsgd_append_items, rows, n, seed)

    def reserve(self, users=None, items=None):
        """Room for that many users / items in all (mfsgd_reserve_rows; None: leave that side alone): appends up to
        there write in place, P and Q keep their addresses and the cached training graphs stay valid.  Never shrinks."""
        self._check(self._lib.mfsgd_reserve_rows(self._handle(), 0 if users is None else int(users),
                                                 0 if items is None else int(items)))

    def capacity(self):
        """(users, items) the model has room for without reallocating; the counts where nothing was reserved."""
        u, i = C.c_int32(), C.c_int32()
        self._check(self._lib.mfsgd_get_capacity(self._handle(), C.byref(u), C.byref(i)))
        return u.value, i.value

    def recommend_rows(self, rows, topn, exclude=None, candidates=None):
        """recommend() for rows that are not in the model (for instance what fold_in returned): (items, scores), each
        [len(rows), topn].  exclude = (row, item): pairs never returned, row indexing `rows`.  candidates: as in
        recommend(), the per-row forms indexing `rows` (mfsgd_recommend_rows_among)."""
        return self._top_n_rows((self._lib.mfsgd_recommend_rows, self._lib.mfsgd_recommend_rows_among), rows, exclude, candidates,
                                topn)

    def _top_n_rows(self, family, rows, exclude, candidates, topn):
        """_top_n for the _rows calls: family is (plain, among), and exclude None or the two arrays of its pairs."""
        rows = _f32(rows)
        if rows.ndim != 2 or rows.shape[1] != self.k:
            raise ValueError("rows must be n_rows x k")
        pairs = _pairs(None, None, "exclude") if exclude is None else _pairs(exclude[0], exclude[1], "exclude")
        return self._top_n(family, rows, (False,) + pairs, candidates, topn)

    def recommend_users_rows(self, rows, topn, exclude=None, candidates=None):
        """recommend_users() for items that are not in the model (for instance what fold_in_items returned: "who should be
        shown this new item"): (users, scores), each [len(rows), topn].  exclude = (row, user): pairs never returned, row
        indexing `rows`.  candidates: as in recommend_users(), the per-row forms indexing `rows`
        (mfsgd_recommend_users_rows_among)."""
        return self._top_n_rows((self._lib.mfsgd_recommend_users_rows, self._lib.mfsgd_recommend_users_rows_among), rows, exclude,
                                candidates, topn)

    def rank_items(self, u, i, exclude=None):
        """int32[n]: for each held-out pair (u[x], i[x]) the number of items that come before i[x] in u[x]'s
        recommendation order (0 = it would be recommended first) -- its index in recommend(u[x], items, exclude)'s row.
        exclude = (u, i): pairs that do not compete (for instance the training ratings); the held-out item itself is
        ranked even when a pair excludes it.  exclude = "seen": the pairs of the seen-item index.  Nothing is sorted: the
        device counts the items that beat each pair."""
        uu, ii = _pairs(np.atleast_1d(u), np.atleast_1d(i), "u and i")
        seen, eu, ei = _exclusions(exclude)
        ranks = np.empty(uu.size, np.int32)
        if seen:
            self._check(self._lib.mfsgd_rank_items_unseen(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), uu.size,
                                                          _p(ranks, C.c_int32)))
            return ranks
        self._check(self._lib.mfsgd_rank_items(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), uu.size,
                                               _p(eu, C.c_int32), _p(ei, C.c_int32), eu.size, _p(ranks, C.c_int32)))
        return ranks

    def rank_items_rows(self, rows, row, i, exclude=None):
        """rank_items() for rows that are not in the model (for instance what fold_in returned): pair x is
        (rows[row[x]], i[x]); exclude = (row, item), row indexing `rows`."""
        rows = _f32(rows)
        if rows.ndim != 2 or rows.shape[1] != self.k:
            raise ValueError("rows must be n_rows x k")
        rr, ii = _pairs(np.atleast_1d(row), np.atleast_1d(i), "row and i")
        er, ei = _pairs(*((None, None) if exclude is None else exclude), "exclude")
        ranks = np.empty(rr.size, np.int32)
        self._check(self._lib.mfsgd_rank_items_rows(self._handle(), _p(rows, C.c_float), rows.shape[0], _p(rr, C.c_int32),
                                                    _p(ii, C.c_int32), rr.size, _p(er, C.c_int32), _p(ei, C.c_int32),
                                                    er.size, _p(ranks, C.c_int32)))
        return ranks

    def evaluate_ranking(self, u, i, topn, exclude=None):
        """rank_items(u, i, exclude) and ranking_metrics(u, ranks, topn) in one call: the metrics dict, which also
        carries "ranks" (int32[n])."""
        uu, ii = _pairs(np.atleast_1d(u), np.atleast_1d(i), "u and i")
        seen, eu, ei = _exclusions(exclude)
        ranks = np.empty(uu.size, np.int32)
        out = _lib.RankingMetrics()
        if seen:
            self._check(self._lib.mfsgd_evaluate_ranking_unseen(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), uu.size,
                                                                int(topn), C.byref(out), _p(ranks, C.c_int32)))
        else:
            self._check(self._lib.mfsgd_evaluate_ranking(self._handle(), _p(uu, C.c_int32), _p(ii, C.c_int32), uu.size,
                                                         int(topn), _p(eu, C.c_int32), _p(ei, C.c_int32), eu.size,
                                                         C.byref(out), _p(ranks, C.c_int32)))
        res = out.as_dict()
        res["ranks"] = ranks
        return res

    # -- cosine neighbours (include/mfsgd.h, "similar items and users") -----------
    _SIDES = {"users": 0, "items": 1}

    def _side(self, side):
        if side not in self._SIDES:
            raise ValueError('side must be "users" or "items"')
        return self._SIDES[side], self.users if side == "users" else self.items

    def row_inv_norms(self, side):
        """float32[n_users] (side "users") or [n_items] ("items"): 1 / sqrt(dot(row, row)) of every row of P or Q, 0 for a
        zero row -- the factors of the cosine the similar_* calls score with."""
        code, size = self._side(side)
        out = np.empty(size, np.float32)
        self._check(self._lib.mfsgd_row_inv_norms(self._handle(), code, _p(out, C.c_float)))
        return out

    def _similar(self, call, queries, topn):
        qq = _i32(np.atleast_1d(queries))
        if qq.ndim != 1:
            raise ValueError("the queries must be a 1-d array")
        index = np.empty((qq.size, int(topn)), np.int32)
        scores = np.empty((qq.size, int(topn)), np.float32)
        self._check(call(self._handle(), _p(qq, C.c_int32), qq.size, int(topn), _p(index, C.c_int32), _p(scores, C.c_float)))
        return index, scores

    def similar_items(self, items, topn):
        """(index, scores), each [len(items), topn]: for each query item the other items with the largest cosine between
        their rows of Q, best first, ties by the smaller index; the query itself is never returned, and a row that runs
        out of candidates (topn == n_items) is padded with -1 / NaN."""
        return self._similar(self._lib.mfsgd_similar_items, items, topn)

    def similar_users(self, users, topn):
        """similar_items() among users: rows of P against P."""
        return self._similar(self._lib.mfsgd_similar_users, users, topn)

    def similar_rows(self, rows, topn, side="items"):
        """(index, scores), each [len(rows), topn]: the neighbours of query vectors of the caller's (n_rows x k: a folded-in
        user, a cold item's vector) among the rows of Q (side "items") or P ("users").  Nothing is excluded."""
        code, _ = self._side(side)
        rows = _f32(rows)
        if rows.ndim != 2 or rows.shape[1] != self.k:
            raise ValueError("rows must be n_rows x k")
        n = rows.shape[0]
        index = np.empty((n, int(topn)), np.int32)
        scores = np.empty((n, int(topn)), np.float32)
        self._check(self._lib.mfsgd_similar_rows(self._handle(), code, _p(rows, C.c_float), n, int(topn),
                                                 _p(index, C.c_int32), _p(scores, C.c_float)))
        return index, scores

    # -- schedule introspection (tests, bench) -----------------------------------
    def schedule_info(self, part=0):
        info = _lib.ScheduleInfo()
        self._check(self._lib.mfsgd_get_schedule_info(self._handle(), int(part), C.byref(info)))
        return info.as_dict()

    def order(self, part=0):
        """Canonical sequential order of a partition and its cell boundaries."""
        info = self.schedule_info(part)
        order = np.empty(info["nnz"], np.int64)
        cell_ptr = np.empty(info["rounds"] * info["blocks"] + 1, np.int64)
        self._check(self._lib.mfsgd_get_order(self._handle(), int(part), _p(order, C.c_int64),
                                              _p(cell_ptr, C.c_int64)))
        return order, cell_ptr

    def debug_schedule(self, part=0):
        """Device-facing schedule arrays (chunk descriptors, rows, subs, entries) as uint32 arrays."""
        n = [C.c_int64() for _ in range(4)]
        self._check(self._lib.mfsgd_debug_schedule_sizes(self._handle(), int(part), *[C.byref(x) for x in n]))
        cells = np.zeros((n[0].value, 8), np.uint32)
        rows = np.zeros(n[1].value, np.uint32)
        subs = np.zeros((n[2].value, 2), np.uint32)
        entries = np.zeros((n[3].value, 4), np.uint32)
        self._check(self._lib.mfsgd_debug_get_schedule(self._handle(), int(part), _p(cells, C.c_uint32),
                                                       _p(rows, C.c_uint32), _p(subs, C.c_uint32),
                                                       _p(entries, C.c_uint32)))
        return cells, rows, subs, entries

    def debug_epoch_profile(self):
        """[workgroups, 7] shader cycles per phase of one persistent epoch (diagnostic)."""
        info = self.schedule_info()
        out = np.zeros(info["blocks"] * 16, np.uint64)
        n = C.c_int32()
        self._check(self._lib.mfsgd_debug_epoch_profile(self._handle(), _p(out, C.c_uint64), C.byref(n)))
        out = out[: n.value * 16].reshape(n.value, 16)
        self.last_slowest_cell = out[:, 7]  # longest single "ratings" phase per workgroup
        self.last_slowest_pass = out[:, 8:15]  # the seven phases of the pass that contained it
        return out[:, :7]

    def debug_counters(self):
        out = np.zeros(4, np.int64)
        self._check(self._lib.mfsgd_debug_counters(self._handle(), _p(out, C.c_int64)))
        return dict(not_resident=int(out[0]), persistent_parts=int(out[1]), graphs=int(out[2]), schedule_builds=int(out[3]))

    def debug_occupy(self, milliseconds):
        """Holds every CU's LDS for a while on a side stream (diagnostic; asynchronous)."""
        self._check(self._lib.mfsgd_debug_occupy(self._handle(), int(milliseconds)))

    def debug_round_stamps(self, rnd):
        """[blocks, 6] stamps of one training round (diagnostic): 4 shader-clock phase
        stamps, then the 100 MHz constant clock at start and end."""
        info = self.schedule_info()
        B, W = info["blocks"], info["waves"]
        out = np.zeros(B * (6 + W * W * 4), np.uint64)
        self._check(self._lib.mfsgd_debug_round_stamps(self._handle(), 0, int(rnd), _p(out, C.c_uint64)))
        self.last_loop_timers = out[B * 6:].reshape(B, W, W, 4)  # [block, wave, sub-round, (gen cyc, run cyc, gen steps, run steps)]
        return out[:B * 6].reshape(B, 6)

    # -- DSGD building blocks (n_parts > 1); see dsgd.py ---------------------------
    def set_item_partition(self, item_part):
        """Item -> partition map (mfsgd_dsgd_plan's), before set_ratings; None = i % n_parts."""
        if item_part is None:
            self._check(self._lib.mfsgd_set_item_partition(self._handle(), None))
            return
        ip = _i32(item_part)
        if ip.shape != (self.items,):
            raise ValueError("item_part must have one entry per item")
        self._check(self._lib.mfsgd_set_item_partition(self._handle(), _p(ip, C.c_int32)))

    def item_partition(self):
        part = np.empty(self.items, np.int32)
        row = np.empty(self.items, np.int32)
        self._check(self._lib.mfsgd_get_item_partition(self._handle(), _p(part, C.c_int32), _p(row, C.c_int32)))
        return part, row

    def part_rows(self, part):
        rows = C.c_int32()
        self._check(self._lib.mfsgd_part_rows(self._handle(), int(part), C.byref(rows)))
        return rows.value

    def part_init_q(self, part, seed, u_total):
        kp = 4 * self._group_lanes()
        buf = np.zeros((self.part_rows(part), kp), np.float32)
        self._check(self._lib.mfsgd_part_init_q(self._handle(), int(part), int(seed), int(u_total),
                                                _p(buf, C.c_float)))
        return buf

    def init_p_offset(self, seed, u_offset):
        self._check(self._lib.mfsgd_init_p_offset(self._handle(), int(seed), int(u_offset)))
        self._initialised = True

    def part_train(self, part, q_block_ptr, stream_ptr=0):
        self._check(self._lib.mfsgd_part_train(self._handle(), int(part), C.c_void_p(q_block_ptr),
                                               C.c_void_p(stream_ptr)))

    def part_sse(self, part, q_block_ptr, stream_ptr=0):
        out = C.c_double()
        self._check(self._lib.mfsgd_part_sse(self._handle(), int(part), C.c_void_p(q_block_ptr),
                                             C.c_void_p(stream_ptr), C.byref(out)))
        return out.value

    def part_sync(self, part, stream_ptr=0):
        """Waits for what part_train put on the stream and checks that the launches ran (mfsgd_part_sync)."""
        self._check(self._lib.mfsgd_part_sync(self._handle(), int(part), C.c_void_p(stream_ptr)))

    def _group_lanes(self):
        need, L = (self.k + 3) // 4, 1
        while L < need:
            L <<= 1
        return L

    @property
    def kp(self):
        return 4 * self._group_lanes()
