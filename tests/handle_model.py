"""A reference model of one long-lived single-partition handle, and a driver that applies a seeded sequence of calls to
the handle and to the model in lock step (tests/test_handle_sequences_cpu.py, tests/test_handle_sequences_gpu.py).

The model holds what include/mfsgd.h says the handle holds -- P and Q (none, P only, or both), lr and lambda as fp32,
the current triples, the held-out set, the count of schedule builds -- and answers every call with the oracle and numpy
alone.  Training is oracle.sgd_pass_ordered over the canonical order of the current rating set; that order, and the
schedule arrays the getters are compared with, come from a throw-away handle of the same configuration that does nothing
but set_ratings and the getters (reference_order, reference_schedule), never from the handle under test: the sequence
decides when the live handle's getters run.  Calls the handle is in no state for are kept: the model answers with the
code the header gives, and nothing may have changed.

The draw of an op depends on the seed and on the model's abstract state only (which of ratings, factors and held-out set
exist), never on a number the library returned, so the same seed gives the same ops against the library, against a
deliberately wrong model, and in a dry run without any library (dry=True), which is how the op weights are checked."""
import collections
import hashlib
import os
import tempfile
import time

import numpy as np

from tests.test_fold_in_gpu import fold_in_ref
from tests.test_rank_items_gpu import _ranks_ref as ranks_ref
from tests.test_recommend_exclude_gpu import _expected as recommend_ref
from tests.test_similar_gpu import _expected as similar_ref
from tests.test_similar_gpu import _rn as inv_norms_ref
from tests.test_similar_gpu import _same as same_topn
from tests.test_validation_gpu import ATOL, RTOL

OK, INVALID, NO_DEVICE, STATE = 0, -1, -2, -5
NAMES = {OK: "ok", INVALID: "INVALID_ARG", NO_DEVICE: "NO_DEVICE", STATE: "STATE"}

# kind -> weight of the draw (profile "gpu").  Profile "host" scales the kinds that compute down: without a device they
# are all MFSGD_ERR_NO_DEVICE.
WEIGHTS = dict(set_ratings=11, init_factors=3, set_factors=3, save_load=2.5, init_p_offset=1.6, fit=8, train=2,
               fit_schedule=3, fit_bold_driver=3, fit_early_stopping=4, set_hyper=8, set_validation=3, clear_validation=1.6,
               validation_rmse=3, rmse_on=3, rmse=3, predict=3, recommend=2, recommend_excl=2, rank_items=2, similar_items=2,
               similar_users=2, fold_in=2, order=3.5, debug_schedule=3.5, schedule_info=2, hyper=2, debug_counters=2,
               get_factors=2)
COMPUTE = ("fit", "train", "fit_schedule", "fit_bold_driver", "fit_early_stopping", "validation_rmse", "rmse_on", "rmse",
           "predict", "recommend", "recommend_excl", "rank_items", "similar_items", "similar_users", "fold_in")
# the error codes the model can answer with when there is a device, per kind (init_factors, set_factors, init_p_offset,
# set_hyper, set_validation, hyper and debug_counters always succeed)
POSSIBLE_ERRORS = {kind: (STATE,) for kind in
                   ("save_load", "fit", "train", "fit_schedule", "fit_bold_driver", "fit_early_stopping", "validation_rmse",
                    "rmse_on", "rmse", "predict", "recommend", "recommend_excl", "rank_items", "similar_items",
                    "similar_users", "fold_in", "order", "debug_schedule", "schedule_info", "get_factors")}
POSSIBLE_ERRORS["set_ratings"] = (INVALID,)


class SequenceMismatch(AssertionError):
    """The handle and the model disagree; the message carries every op so far."""


def _digest(u, i, r):
    return hashlib.blake2b(u.tobytes() + b"|" + i.tobytes() + b"|" + r.tobytes(), digest_size=16).digest()


def _bits(x):
    return np.float32(x).tobytes()


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} words differ, first at {bad[:4]}, max abs {np.abs(a - b).max()}"


def _close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


# -- the two rating sets -------------------------------------------------------------------------------------------------
def rating_set_a(U, I, seed=1):
    """The shape of test_lone_tile_mailbox_hand_off: item 9 rated by every user, item 17 by every other user, 6 U random
    pairs, deduplicated, shuffled."""
    rng = np.random.default_rng(seed)
    u = list(range(U)) + list(range(0, U, 2)) + list(rng.integers(0, U, 6 * U))
    i = [9] * U + [17] * len(range(0, U, 2)) + list(rng.integers(0, I, 6 * U))
    key = rng.permutation(np.unique(np.array(u, np.int64) * I + np.array(i, np.int64)))
    return (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(key.size) * 4 + 1).astype(np.float32)


def rating_set_b(U, I, seed=2):
    """Uniform random pairs over the same U x I, about half as many as set A has."""
    rng = np.random.default_rng(seed)
    key = rng.choice(U * I, min(U * I // 2, (7 * U) // 2 - 3), replace=False)
    return (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(key.size) * 4 + 1).astype(np.float32)


_sets = {}


def rating_sets(U, I):
    if (U, I) not in _sets:
        _sets[(U, I)] = dict(A=rating_set_a(U, I), B=rating_set_b(U, I))
    return _sets[(U, I)]


# -- the throw-away handle ---------------------------------------------------------------------------------------------
_order_cache, _sched_cache = {}, {}


def _cfg_key(cfg):
    return tuple(cfg[x] for x in ("U", "I", "k", "blocks", "waves", "flags"))


def _throw_away(mf, cfg, triples, lr, lam):
    m = mf.MatrixFactorizationSGD(cfg["U"], cfg["I"], cfg["k"], float(lr), float(lam), cfg["seed"], blocks=cfg["blocks"],
                                  waves=cfg["waves"], flags=cfg["flags"])
    m.set_ratings(*triples)
    return m


def reference_order(mf, oracle, cfg, triples, digest):
    """(order, cell_ptr) of the rating set under the configuration, from a handle of its own; checked once
    (oracle.check_block_schedule) and never modified."""
    key = (digest, _cfg_key(cfg))
    if key not in _order_cache:
        with _throw_away(mf, cfg, triples, cfg["lr"], cfg["lam"]) as m:
            order, cell_ptr = m.order()
            info = m.schedule_info()
        u, i, _ = triples
        assert info["nnz"] == u.size
        if u.size:
            assert oracle.check_block_schedule(u, i, cfg["U"], cfg["I"], order, cell_ptr, info["rounds"], info["blocks"]) == 0
            assert np.array_equal(np.sort(order), np.arange(u.size))
        _order_cache[key] = (order, cell_ptr)
    return _order_cache[key]


def reference_schedule(mf, cfg, triples, digest, lr, lam):
    """What a handle CREATED at (lr, lam) builds for the rating set: dict(info, sched, lone)."""
    key = (digest, _cfg_key(cfg), _bits(lr), _bits(lam))
    if key not in _sched_cache:
        with _throw_away(mf, cfg, triples, lr, lam) as m:
            info = m.schedule_info()
            info.pop("build_seconds")
            sched = m.debug_schedule()
        _sched_cache[key] = dict(info=info, sched=sched, lone=bool((sched[0][:, 5] & 1).any()) if sched[0].size else False)
    return _sched_cache[key]


# -- the calls that read the handle's own Q -----------------------------------------------------------------------------
def q_less_calls(m):
    """(message prefix, call) for every call that reads the handle's own Q, on a model of at least 2 users and 2 items
    that has ratings and a held-out set (tests/test_capi_cpu.py asserts them one by one; op_init_p_offset below makes them an op)."""
    k = m.k
    rows = np.ones((1, k), np.float32)
    es = lambda: m.fit_early_stopping(2, patience=1)
    return (("train", lambda: m.fit(1)), ("train", lambda: m.fit(1, rmse=False)), ("train", lambda: m.fit(0)),
            ("train_timed", lambda: m.train_timed(1)),
            ("train_schedule", lambda: m.fit_schedule([0.01, 0.02])), ("bold_driver", lambda: m.fit_bold_driver(2)),
            ("early_stop", es), ("rmse", m.rmse), ("predict", lambda: m.predict([0], [1])),
            ("recommend", lambda: m.recommend([0], 1)), ("recommend", lambda: m.recommend([0], 1, exclude=([0], [0]))),
            ("recommend_rows", lambda: m.recommend_rows(rows, 1)),
            ("rank_items", lambda: m.rank_items([0], [1])), ("rank_items", lambda: m.rank_items_rows(rows, [0], [1])),
            ("rank_items", lambda: m.evaluate_ranking([0], [1], 1)),
            ("similar_items", lambda: m.similar_items([0], 1)), ("similar_rows", lambda: m.similar_rows(rows, 1, side="items")),
            ("row_inv_norms", lambda: m.row_inv_norms("items")),
            ("fold_in", lambda: m.fold_in([0, 1], [0], [1.0], 1)),
            ("validation_rmse", m.validation_rmse), ("rmse_pairs", lambda: m.rmse_on([0], [0], [1.0])),
            ("debug_round_stamps", lambda: m.debug_round_stamps(0)), ("debug_epoch_profile", m.debug_epoch_profile),
            ("get_factors", m.get_factors))


# -- the model and the driver ---------------------------------------------------------------------------------------------
class Runner:
    """One handle (self.m; None in a dry run) and its model.  Abstract state: R (ratings), F ("none", "ponly", "full"),
    V (a held-out set that is not empty), initialised (the Python wrapper's flag), builds.  Numbers (not in a dry run): P,
    Q, lr, lam, ratings, val."""

    def __init__(self, mf, oracle, cfg, *, device, dry, wrong, tmpdir):
        self.mf, self.oracle, self.cfg, self.device, self.dry, self.wrong, self.tmpdir = mf, oracle, cfg, device, dry, wrong, tmpdir
        self.U, self.I, self.k = cfg["U"], cfg["I"], cfg["k"]
        self.sets = rating_sets(self.U, self.I)
        self.R, self.F, self.V, self.initialised, self.builds = False, "none", False, False, 0
        self.name, self.ratings, self.digest, self.last_valid = None, None, None, None
        self.sched_computed, self.any_compute, self.after_failure = False, False, False
        self.P = self.Q = None
        self.lr, self.lam = np.float32(cfg["lr"]), np.float32(cfg["lam"])
        e = np.empty(0, np.int32)
        self.val = (e, e, np.empty(0, np.float32))
        self.counts, self.facts, self.log, self.n_files = collections.Counter(), collections.Counter(), [], 0
        self.m = None
        if not dry:
            self.m = mf.MatrixFactorizationSGD(self.U, self.I, self.k, cfg["lr"], cfg["lam"], cfg["seed"], blocks=cfg["blocks"],
                                               waves=cfg["waves"], flags=cfg["flags"])

    # .. the draw ......................................................................................................
    def weights(self):
        w = dict(WEIGHTS)
        if self.cfg.get("profile", "gpu") == "host":
            for kind in COMPUTE:
                w[kind] *= 0.2
        if not self.R:
            w["set_ratings"] *= 3
        if self.builds == 0:
            w["set_hyper"] *= 3  # (a change of values before any ratings, and before any compute call)
        if self.F == "none":
            w["init_factors"] *= 3
            w["set_factors"] *= 2
            w["train"] *= 2
        if self.F == "ponly":
            w["init_factors"] *= 6
            w["set_factors"] *= 6
            w["init_p_offset"] = 0.3
            w["train"] *= 4  # (the one state in which the Java surface's train() is an error)
        if not self.V:
            w["set_validation"] *= 3
        return w

    def step(self, rng, kind=None):
        w = self.weights()
        kinds = sorted(w)
        p = np.array([w[x] for x in kinds], np.float64)
        drawn = kinds[int(rng.choice(len(kinds), p=p / p.sum()))]
        seed = int(rng.integers(1 << 31))
        kind = kind or drawn
        self.log.append(f"{len(self.log):3d} {kind}(seed={seed})")
        code = getattr(self, "op_" + kind)(np.random.default_rng(seed))
        self.log[-1] += f" -> {NAMES[code]}"
        self.counts[(kind, NAMES[code])] += 1

    def note(self, text):
        self.log[-1] += " " + text

    # .. plumbing ......................................................................................................
    def call(self, want, fn):
        """Runs fn against the handle: (code, value).  The code must be the model's."""
        if self.dry:
            return want, None
        try:
            value, code, msg = fn(), OK, ""
        except self.mf.MfsgdError as e:
            value, code, msg = None, e.code, str(e)
        assert code == want, f"returned {NAMES.get(code, code)} {msg!r}, the model expects {NAMES[want]}"
        return code, value

    def code_train(self):
        """The calls that go through prepare_compute, after their own Q check."""
        if self.F == "ponly" or not self.R:
            return STATE
        if not self.device:
            return NO_DEVICE
        return STATE if self.F == "none" else OK

    def code_pq(self, none_first):
        """The calls that read P and Q without the ratings; none_first: they ask for the factors before the device."""
        if (none_first and self.F == "none") or self.F == "ponly":
            return STATE
        if not self.device:
            return NO_DEVICE
        return STATE if self.F == "none" else OK

    def computed(self, epochs=0):
        self.sched_computed = self.any_compute = True
        if epochs > 0 and self.lone():
            self.facts["trained_on_a_lone_tile_schedule"] += 1

    def packed(self):
        """The schedule's arrays were packed on the device and (until the first compute call) belong to it."""
        from mfsgd_amd import _lib

        guess = bool(self.cfg["flags"] & _lib.FLAG_DEVICE_INGEST) and self.device and self.ratings[0].size > 0
        if self.dry:
            return guess
        return reference_schedule(self.mf, self.cfg, self.ratings, self.digest, self.cfg["lr"], self.cfg["lam"])["info"]["device_ingest"] == 2

    def lone(self):
        guess = self.cfg["blocks"] > 0 and self.name.startswith("A")
        if self.dry:
            return guess
        got = reference_schedule(self.mf, self.cfg, self.ratings, self.digest, self.cfg["lr"], self.cfg["lam"])["lone"]
        if self.cfg["blocks"] > 0:
            assert got == guess, f"set {self.name}: lone-tile cells {got}, expected {guess}"
        return got

    def order(self):
        return reference_order(self.mf, self.oracle, self.cfg, self.ratings, self.digest)[0]

    def one_pass(self, lr, lam):
        u, i, r = self.ratings
        if u.size:
            self.oracle.sgd_pass_ordered(self.P, self.Q, u, i, r, self.order(), float(lr), float(lam))

    def train_rmse(self):
        return self.oracle.rmse(self.P, self.Q, *self.ratings) if self.ratings[0].size else 0.0

    def check_hyper(self):
        if not self.dry:
            assert self.m.hyper() == (float(self.lr), float(self.lam)), (self.m.hyper(), float(self.lr), float(self.lam))

    def exclusions(self):
        if self.R:
            return self.ratings[0], self.ratings[1]
        return np.empty(0, np.int32), np.empty(0, np.int32)

    # .. ratings .......................................................................................................
    def apply_set(self, name, triples):
        """The model's side of a valid mfsgd_set_ratings: True when the schedule is kept."""
        digest = _digest(*triples)
        reuse = self.R and digest == self.digest
        if not reuse:
            self.builds += 1
            self.sched_computed = False
            if self.after_failure and self.last_valid and digest == _digest(*self.last_valid[1]):
                self.facts["set_ratings_build_of_the_set_a_failed_call_dropped"] += 1
        self.after_failure = False
        self.R, self.name, self.ratings, self.digest, self.last_valid = True, name, triples, digest, (name, triples)
        self.facts["set_ratings_reuse" if reuse else "set_ratings_build"] += 1
        return reuse

    def pick_set(self, g, variants):
        """(variant, name, triples) of a valid rating set."""
        v = variants[int(g.integers(len(variants)))]
        if v == "again":
            if self.R:
                return v, self.name, self.ratings
            if self.last_valid:
                return v, self.last_valid[0], self.last_valid[1]
            v = "A"
        if v == "edit":
            if self.R and self.ratings[0].size:
                u, i, r = self.ratings
                r = r.copy()
                r[int(g.integers(r.size))] += np.float32(1.0)
                return v, self.name.rstrip("'") + "'", (u, i, r)
            v = "A"
        if v == "empty":
            e = np.empty(0, np.int32)
            return v, "empty", (e, e, np.empty(0, np.float32))
        return v, v, self.sets[v]

    def op_set_ratings(self, g):
        variants = ("A", "A", "B", "B", "again", "again", "again", "edit", "edit", "empty", "bad", "bad")
        if variants[int(g.integers(len(variants)))] == "bad":
            _, name, (u, i, r) = self.pick_set(g, ("again", "A", "B"))
            if u.size == 0:
                name, (u, i, r) = "A", self.sets["A"]
            valid = (u, i, r)
            u, i = u.copy(), i.copy()
            j = int(g.integers(u.size))
            if g.integers(2):
                u[j] = self.U
            else:
                i[j] = self.I
            self.note(f"[{name} with pair {j} out of range, n={u.size}]")
            code, _ = self.call(INVALID, lambda: self.m.set_ratings(u, i, r))
            if self.wrong != "failed_set_ratings_keeps":
                self.R = False  # the schedules are gone: nothing trains until a valid set comes
                self.after_failure = True
            self.last_valid = (name, valid)  # "again" sends the same triples, valid as before: they must be built again
            return code
        v, name, triples = self.pick_set(g, ("A", "A", "B", "B", "again", "again", "again", "edit", "edit", "empty"))
        self.note(f"[{v}: {name}, n={triples[0].size}]")
        equal_length = self.R and triples[0].size == self.ratings[0].size
        code, _ = self.call(OK, lambda: self.m.set_ratings(*triples))
        reuse = self.apply_set(name, triples)
        if v == "edit" and equal_length and not reuse:
            self.facts["set_ratings_rebuild_of_equal_length"] += 1
        if not self.dry:
            assert self.m.debug_counters()["schedule_builds"] == self.builds, (self.m.debug_counters(), self.builds, reuse)
        return code

    # .. factors .......................................................................................................
    def op_init_factors(self, g):
        seed = int(g.integers(1, 1000))
        code, _ = self.call(OK, lambda: self.m.init_factors(seed))
        self.F, self.initialised = "full", True
        if not self.dry:
            self.P, self.Q = self.oracle.init_factors(self.U, self.I, self.k, seed)
        return code

    def op_set_factors(self, g):
        P = (g.standard_normal((self.U, self.k)) * 0.1).astype(np.float32)
        Q = (g.standard_normal((self.I, self.k)) * 0.1).astype(np.float32)
        code, _ = self.call(OK, lambda: self.m.set_factors(P, Q))
        self.F, self.initialised, self.P, self.Q = "full", True, P, Q
        return code

    def op_save_load(self, g):
        """save_factors, factors of another seed, load_factors: the model keeps what it had."""
        self.n_files += 1
        path = os.path.join(self.tmpdir, f"factors{self.n_files}.bin")
        code, _ = self.call(OK if self.F == "full" else STATE, lambda: self.m.save_factors(path))
        if code == OK and not self.dry:
            self.m.init_factors(int(g.integers(1000, 2000)))
            self.m.load_factors(path)
        return code

    def op_init_p_offset(self, g):
        """mfsgd_init_p_offset on a single-partition handle: P of the offset, no Q, and every call that reads the
        handle's Q is MFSGD_ERR_STATE before anything is launched (tests/test_capi_cpu.py has the list)."""
        seed, off = int(g.integers(1, 1000)), int(g.integers(0, 50))
        self.note(f"[seed {seed}, offset {off}]")
        code, _ = self.call(OK, lambda: self.m.init_p_offset(seed, off))
        self.F, self.initialised, self.Q = "ponly", True, None
        if not self.dry:
            self.P = np.ascontiguousarray(self.oracle.init_factors(off + self.U, 1, self.k, seed)[0][off:])
            for prefix, fn in q_less_calls(self.m):
                try:
                    fn()
                    raise AssertionError(f"{prefix} succeeded on a handle without Q")
                except self.mf.MfsgdError as e:
                    assert e.code == STATE, (prefix, e)
                    if self.R and self.V:  # (otherwise a few of them are state errors for another reason first)
                        assert f": {prefix}: Q is not initialised" in str(e), (prefix, e)
            import ctypes as C

            P = np.empty((self.U, self.k), np.float32)
            self.m._check(self.m._lib.mfsgd_get_factors(self.m._handle(), P.ctypes.data_as(C.POINTER(C.c_float)), None))
            _same_bits(P, self.P, "P of init_p_offset")
            self.check_hyper()
        return code

    def op_get_factors(self, g):
        code, got = self.call(OK if self.F == "full" else STATE, lambda: self.m.get_factors())
        if code == OK and not self.dry:
            _same_bits(got[0], self.P, "P")
            _same_bits(got[1], self.Q, "Q")
        return code

    # .. training ......................................................................................................
    def op_fit(self, g):
        n, with_rmse = int(g.integers(0, 4)), bool(g.integers(2))
        self.note(f"[{n} epochs, rmse={with_rmse}]")
        return self.fit(n, with_rmse, lambda: self.m.fit(n, rmse=with_rmse))

    def fit(self, n, with_rmse, fn):
        code, got = self.call(self.code_train(), fn)
        if code == OK:
            self.computed(n)
            if not self.dry:
                ref = []
                for _ in range(n):
                    self.one_pass(self.lr, self.lam)
                    ref.append(self.train_rmse())
                if with_rmse:
                    assert len(got) == n
                    _close(got, ref, "RMSE per epoch")
                else:
                    assert got is None
        return code

    def op_train(self, g):
        """The Java surface: set_ratings, init_factors unless something gave factors before, fit."""
        v, name, triples = self.pick_set(g, ("A", "B", "again"))
        n = int(g.integers(1, 3))
        self.note(f"[{v}: {name}, n={triples[0].size}, {n} epochs]")
        self.apply_set(name, triples)
        if not self.initialised:
            self.F, self.initialised = "full", True
            if not self.dry:
                self.P, self.Q = self.oracle.init_factors(self.U, self.I, self.k, self.cfg["seed"])
        code = self.fit(n, True, lambda: self.m.train(*triples, n))
        if not self.dry:
            assert self.m.debug_counters()["schedule_builds"] == self.builds
        return code

    def op_fit_schedule(self, g):
        n = int(g.integers(1, 4))
        lrs = g.uniform(0.004, 0.03, n).astype(np.float32)
        lams = None if g.integers(2) else (g.uniform(0.0, 0.08, n) * g.integers(0, 2, n)).astype(np.float32)
        with_rmse = bool(g.integers(2))
        self.note(f"[{n} epochs, lam given={lams is not None}, rmse={with_rmse}]")
        code, got = self.call(self.code_train(), lambda: self.m.fit_schedule(lrs, lams, rmse=with_rmse))
        if code == OK:
            self.computed(n)
            if not self.dry:
                ref = []
                for e in range(n):
                    self.lr, self.lam = lrs[e], self.lam if lams is None else lams[e]
                    self.one_pass(self.lr, self.lam)
                    ref.append(self.train_rmse())
                if with_rmse:
                    _close(got, ref, "RMSE per epoch of the schedule")
                else:
                    assert got is None
        self.check_hyper()
        return code

    def op_fit_bold_driver(self, g):
        epochs, up, down = 2, 1.05, 0.5
        code, got = self.call(self.code_train(), lambda: self.m.fit_bold_driver(epochs, up, down))
        if code == OK:
            self.computed(epochs)
            if not self.dry:
                used, rm = got
                prev = self.train_rmse()
                for e in range(epochs):
                    assert _bits(used[e]) == _bits(self.lr), (e, used, self.lr)
                    self.one_pass(self.lr, self.lam)
                    _close(rm[e], self.train_rmse(), f"RMSE of bold-driver epoch {e}")
                    # the rule on the figure the call itself reported (it is within 1e-9 of the oracle's)
                    self.lr = np.float32(self.lr * np.float32(up) if rm[e] < prev else self.lr * np.float32(down))
                    prev = rm[e]
        self.check_hyper()
        return code

    def op_fit_early_stopping(self, g):
        max_epochs, patience, restore = int(g.integers(1, 5)), int(g.integers(1, 3)), bool(g.integers(2))
        lrs = g.uniform(0.004, 0.03, max_epochs).astype(np.float32) if g.integers(3) == 0 else None
        with_train = bool(g.integers(2))
        self.note(f"[max {max_epochs}, patience {patience}, restore {restore}, lr given={lrs is not None}, train rmse={with_train}]")
        if not self.R or not self.V or self.F != "full":
            want = STATE
        else:
            want = OK if self.device else NO_DEVICE
        code, res = self.call(want, lambda: self.m.fit_early_stopping(max_epochs, patience=patience, restore_best=restore, lr=lrs,
                                                                      train_rmse=with_train))
        if code == OK:
            self.computed(1)
            if not self.dry:
                best, best_epoch, bad, snap, ran = np.inf, -1, 0, None, 0
                for e in range(max_epochs):
                    if lrs is not None:
                        self.lr = lrs[e]
                    self.one_pass(self.lr, self.lam)
                    ran = e + 1
                    assert res["epochs_run"] >= ran, res
                    _close(res["val_rmse"][e], self.oracle.rmse(self.P, self.Q, *self.val), f"held-out RMSE of epoch {e}")
                    if with_train:
                        _close(res["train_rmse"][e], self.train_rmse(), f"training RMSE of epoch {e}")
                    v = res["val_rmse"][e]  # the rule on the figure the call itself reported
                    if v < best:
                        best, best_epoch, bad, snap = v, e, 0, (self.P.copy(), self.Q.copy())
                    else:
                        bad += 1
                        if bad >= patience:
                            break
                assert (res["epochs_run"], res["best_epoch"], len(res["val_rmse"])) == (ran, best_epoch, ran), (res, ran, best_epoch)
                assert (res["train_rmse"] is None) == (not with_train)
                if restore and best_epoch >= 0 and best_epoch != ran - 1:
                    self.P, self.Q = snap
                    self.note("[restored]")
        self.check_hyper()
        return code

    # .. lr and lambda .................................................................................................
    def note_hyper_state(self):
        """Which kind of schedule a change of values met."""
        if not self.packed():
            self.facts["set_hyper_on_a_host_packed_schedule"] += 1
        elif self.sched_computed:
            self.facts["set_hyper_on_a_device_packed_schedule_after_compute"] += 1
        else:
            self.facts["set_hyper_on_a_device_packed_schedule_before_compute"] += 1

    def op_set_hyper(self, g):
        v = ("new", "new", "new", "same", "lam0")[int(g.integers(5))]
        lr, lam = np.float32(g.uniform(0.004, 0.03)), np.float32(g.uniform(0.01, 0.08))
        if v == "same":
            lr, lam = self.lr, self.lam
        if v == "lam0":
            lam = np.float32(0.0)
        self.note(f"[{v}: {float(lr)!r}, {float(lam)!r}]")
        graphs = None if self.dry else self.m.debug_counters()["graphs"]
        code, _ = self.call(OK, lambda: self.m.set_hyper(lr, lam))
        if v == "same":
            self.facts["set_hyper_same_bits"] += 1
            if not self.dry:
                assert self.m.debug_counters()["graphs"] == graphs, "the same bits are a no-op: the graphs stay"
        else:
            if not self.R:
                self.facts["set_hyper_before_any_ratings" if self.builds == 0 else "set_hyper_without_ratings"] += 1
                if not self.any_compute:
                    self.facts["set_hyper_before_any_compute"] += 1
            else:
                self.note_hyper_state()
                if not self.dry:
                    assert self.m.debug_counters()["graphs"] == 0, "graphs carry lr and c: they are dropped"
            if self.R or self.wrong != "hyper_before_ratings":
                self.lr, self.lam = lr, lam
        self.check_hyper()
        return code

    def op_hyper(self, g):
        code, got = self.call(OK, lambda: self.m.hyper())
        if not self.dry:
            assert got == (float(self.lr), float(self.lam)), (got, float(self.lr), float(self.lam))
        return code

    # .. the held-out set ..............................................................................................
    def pairs(self, g, n):
        u, i = g.integers(0, self.U, n).astype(np.int32), g.integers(0, self.I, n).astype(np.int32)
        return u, i, (g.integers(1, 11, n) * 0.5).astype(np.float32)

    def op_set_validation(self, g):
        self.val = self.pairs(g, int(g.integers(50, 400)))
        self.note(f"[n={self.val[0].size}]")
        code, _ = self.call(OK, lambda: self.m.set_validation(*self.val))
        self.V = True
        if not self.dry:
            assert self.m.validation_size() == self.val[0].size
        return code

    def op_clear_validation(self, g):
        self.val = self.pairs(g, 0)
        code, _ = self.call(OK, lambda: self.m.set_validation(*self.val))
        self.V = False
        if not self.dry:
            assert self.m.validation_size() == 0
        return code

    def op_validation_rmse(self, g):
        if self.F != "full":
            want = STATE
        else:
            want = OK if self.device or not self.V else NO_DEVICE
        code, got = self.call(want, lambda: self.m.validation_rmse(sse=True))
        if code == OK and not self.dry:
            if self.V:
                _close(got[0], self.oracle.rmse(self.P, self.Q, *self.val), "held-out RMSE")
                _close(got[1], self.oracle.sse(self.P, self.Q, *self.val), "held-out SSE")
            else:
                assert got == (0.0, 0.0)
        return code

    def op_rmse_on(self, g):
        u, i, r = self.pairs(g, int(g.integers(1, 400)))
        self.note(f"[n={u.size}]")
        code, got = self.call(self.code_pq(True), lambda: self.m.rmse_on(u, i, r, sse=True))
        if code == OK and not self.dry:
            _close(got[0], self.oracle.rmse(self.P, self.Q, u, i, r), "RMSE of the pairs")
            _close(got[1], self.oracle.sse(self.P, self.Q, u, i, r), "SSE of the pairs")
        return code

    # .. serving .......................................................................................................
    def op_rmse(self, g):
        code, got = self.call(self.code_train(), lambda: self.m.rmse())
        if code == OK:
            self.computed()
            if not self.dry:
                _close(got, self.train_rmse(), "RMSE")
        return code

    def op_predict(self, g):
        u, i, _ = self.pairs(g, 64)
        code, got = self.call(self.code_pq(False), lambda: self.m.predict(u, i))
        if code == OK and not self.dry:
            _same_bits(got, self.oracle.predict(self.P, self.Q, u, i), "predict")
        return code

    def recommend(self, g, excl):
        users = g.integers(0, self.U, 4).astype(np.int32)
        users[3] = users[0]  # one user twice
        eu, ei = self.exclusions() if excl else (np.empty(0, np.int32),) * 2
        code, got = self.call(self.code_pq(False), lambda: self.m.recommend(users, 5, exclude=(eu, ei) if excl else None))
        if code == OK and not self.dry:
            same_topn(got, recommend_ref(self.oracle, self.P, self.Q, users, 5, eu, ei))
        return code

    def op_recommend(self, g):
        return self.recommend(g, False)

    def op_recommend_excl(self, g):
        return self.recommend(g, True)

    def op_rank_items(self, g):
        u, i, _ = self.pairs(g, 12)
        eu, ei = self.exclusions()
        code, got = self.call(self.code_pq(True), lambda: self.m.rank_items(u, i, exclude=(eu, ei)))
        if code == OK and not self.dry:
            assert np.array_equal(got, ranks_ref(self.oracle, self.P, self.Q, u, i, eu, ei)), got
        return code

    def op_similar_items(self, g):
        q = g.integers(0, self.I, 6).astype(np.int32)
        code, got = self.call(self.code_pq(True), lambda: self.m.similar_items(q, 4))
        if code == OK and not self.dry:
            rn = inv_norms_ref(self.oracle, self.Q)
            same_topn(got, similar_ref(self.oracle, self.Q, rn, q, self.Q, rn, 4, True))
        return code

    def op_similar_users(self, g):
        q = g.integers(0, self.U, 8).astype(np.int32)
        if self.F == "none":
            want = STATE
        else:
            want = OK if self.device else NO_DEVICE  # (P alone is enough)
        code, got = self.call(want, lambda: self.m.similar_users(q, 3))
        if code == OK and not self.dry:
            rn = inv_norms_ref(self.oracle, self.P)
            same_topn(got, similar_ref(self.oracle, self.P, rn, q, self.P, rn, 3, True))
        return code

    def op_fold_in(self, g):
        """fold_in of five new users, then recommend_rows for the rows it returned, their own items left out."""
        lens = g.integers(0, 13, 5)
        row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        items = g.integers(0, self.I, int(row_ptr[-1])).astype(np.int32)
        ratings = g.uniform(0.5, 5.0, items.size).astype(np.float32)
        epochs, seeded = int(g.integers(0, 3)), bool(g.integers(2))
        seed = int(g.integers(1, 1000))
        init = None if seeded else g.standard_normal((5, self.k)).astype(np.float32)
        self.note(f"[{epochs} epochs, {items.size} ratings, seeded={seeded}]")
        code, rows = self.call(self.code_pq(True), lambda: self.m.fold_in(row_ptr, items, ratings, epochs, init=init, seed=seed))
        if code == OK and not self.dry:
            R0 = self.oracle.init_factors(5, 0, self.k, seed)[0] if seeded else init
            want = fold_in_ref(self.oracle, self.Q, row_ptr, items, ratings, epochs, R0, float(self.lr), float(self.lam))
            _same_bits(rows, want, "fold_in rows")
            er = np.repeat(np.arange(5, dtype=np.int32), lens).astype(np.int32)
            got = self.m.recommend_rows(rows, 4, exclude=(er, items))
            same_topn(got, recommend_ref(self.oracle, want, self.Q, np.arange(5, dtype=np.int32), 4, er, items))
        return code

    # .. getters .......................................................................................................
    def getter(self):
        self.facts["schedule_getter_after_compute" if self.sched_computed else "schedule_getter_before_compute"] += 1

    def op_order(self, g):
        code, got = self.call(OK if self.R else STATE, lambda: self.m.order())
        if code == OK:
            self.getter()
            if not self.dry:
                want = reference_order(self.mf, self.oracle, self.cfg, self.ratings, self.digest)
                assert np.array_equal(got[0], want[0]), "the canonical order differs from a fresh handle's"
                assert np.array_equal(got[1], want[1]), "the cell boundaries differ from a fresh handle's"
        return code

    def op_debug_schedule(self, g):
        code, got = self.call(OK if self.R else STATE, lambda: self.m.debug_schedule())
        if code == OK:
            self.getter()
            if not self.dry:
                want = reference_schedule(self.mf, self.cfg, self.ratings, self.digest, self.lr, self.lam)["sched"]
                for name, x, y in zip(("cells", "rows", "subs", "entries"), got, want):
                    assert x.shape == y.shape and np.array_equal(x, y), \
                        f"{name} differ from a handle created at ({float(self.lr)!r}, {float(self.lam)!r})"
        return code

    def op_schedule_info(self, g):
        code, got = self.call(OK if self.R else STATE, lambda: self.m.schedule_info())
        if code == OK and not self.dry:
            got.pop("build_seconds")
            want = reference_schedule(self.mf, self.cfg, self.ratings, self.digest, self.lr, self.lam)["info"]
            assert got == want, (got, want)
        return code

    def op_debug_counters(self, g):
        code, got = self.call(OK, lambda: self.m.debug_counters())
        if not self.dry:
            assert got["schedule_builds"] == self.builds, (got, self.builds)
        return code


def run_sequence(mf, oracle, seed, n_ops, config, *, device=True, dry=False, wrong=None):
    """Creates one handle of `config` (dict: U, I, k, blocks, waves, flags, lr, lam, seed, profile), applies n_ops drawn ops
    and a final get_factors to it and to the model in lock step, asserting after each; closes it and checks that the
    library's device-byte count is back where it started.  Raises SequenceMismatch with every op so far.  Returns
    dict(counts {(kind, outcome): n}, facts {name: n}, n_ops, errors, seconds, log).
    device=False: no GPU is expected, and every call that needs one is MFSGD_ERR_NO_DEVICE.  dry=True: no library at all,
    the ops and their outcomes as the model alone gives them.  wrong: a deliberately wrong rule of the model
    ("hyper_before_ratings", "failed_set_ratings_keeps"), for the driver's self-test."""
    cfg = dict(blocks=0, waves=0, flags=0, lr=0.02, lam=0.03, seed=7, profile="gpu")
    cfg.update(config)
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    start = None if dry else mf.debug_device_bytes()
    with tempfile.TemporaryDirectory() as tmpdir:
        run = Runner(mf, oracle, cfg, device=device, dry=dry, wrong=wrong, tmpdir=tmpdir)
        try:
            try:
                for _ in range(n_ops):
                    run.step(rng)
                run.step(rng, kind="get_factors")
            finally:
                if run.m is not None:
                    run.m.close()
            if not dry:
                assert mf.debug_device_bytes() == start, f"{mf.debug_device_bytes() - start} device bytes are left after close()"
        except SequenceMismatch:
            raise
        except Exception as e:
            raise SequenceMismatch(f"{type(e).__name__}: {e}\nconfig {cfg}, seed {seed}, device={device}; ops so far:\n" +
                                   "\n".join(run.log)) from e
    errors = sum(n for (_, outcome), n in run.counts.items() if outcome != "ok")
    return dict(counts=run.counts, facts=run.facts, n_ops=n_ops + 1, errors=errors, seconds=time.perf_counter() - t0, log=run.log)


def check_coverage(results):
    """The conditions of a set of sequences taken together (device present): returns the totals, raises on a miss."""
    counts, facts = collections.Counter(), collections.Counter()
    for res in results:
        counts.update(res["counts"])
        facts.update(res["facts"])
    total = sum(counts.values())
    errors = sum(n for (_, outcome), n in counts.items() if outcome != "ok")
    missing = [kind for kind in WEIGHTS if counts[(kind, "ok")] < 10]
    assert not missing, f"fewer than 10 successful runs of {missing}: {dict(counts)}"
    missing = [(kind, NAMES[c]) for kind, codes in POSSIBLE_ERRORS.items() for c in codes if counts[(kind, NAMES[c])] < 1]
    assert not missing, f"error outcomes that never occurred: {missing}"
    for fact in ("set_ratings_reuse", "set_ratings_rebuild_of_equal_length", "set_hyper_on_a_device_packed_schedule_before_compute",
                 "set_hyper_on_a_device_packed_schedule_after_compute", "set_hyper_on_a_host_packed_schedule",
                 "set_hyper_before_any_ratings", "set_hyper_before_any_compute", "set_hyper_same_bits",
                 "trained_on_a_lone_tile_schedule", "schedule_getter_before_compute", "schedule_getter_after_compute"):
        assert facts[fact] >= 1, f"{fact} never happened: {dict(facts)}"
    assert errors <= 0.35 * total, f"{errors} of {total} ops ended in an error code"
    return dict(ops=total, errors=errors, counts=counts, facts=facts)


# -- the cases of tests/test_handle_sequences_gpu.py (its dry run is a CPU test) --------------------------------------------
GEOMETRIES = {
    "k8": dict(k=8, U=600, I=90),                                    # L = 2: the C++ step; automatic blocks
    "k64_b16_w2": dict(k=64, blocks=16, waves=2, U=150 * 16, I=90),  # L = 16: solo runs, a lone-tile mailbox
    "k100_b12_w2": dict(k=100, blocks=12, waves=2, U=150 * 12, I=90),  # L = 32, padded
}
GPU_FLAGS = ("default", "FLAG_ROUND_LAUNCH", "FLAG_NO_GRAPH", "FLAG_DEVICE_INGEST", "FLAG_HOST_INGEST")
GPU_SEEDS = (0, 1)
GPU_OPS = 40


def flag_value(name):
    from mfsgd_amd import _lib

    return 0 if name == "default" else getattr(_lib, name)


def gpu_config(flag, geometry):
    return dict(GEOMETRIES[geometry], flags=flag_value(flag))


def gpu_seed(flag, geometry, seed):
    """Another sequence for every case."""
    return 1000 * GPU_FLAGS.index(flag) + 100 * sorted(GEOMETRIES).index(geometry) + seed
