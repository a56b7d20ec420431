"""A reference model of one long-lived single-partition handle, and a driver that applies a seeded sequence of calls to
the handle and to the model in lock step (tests/test_handle_sequences_cpu.py, tests/test_handle_sequences_gpu.py).

The model holds what include/mfsgd.h says the handle holds -- P and Q (none, P only, or both), the live counts of users
and items and the capacity per side, lr and lambda as fp32, the current triples, the held-out set, the count of schedule
builds, where the factors are (host staging or the device) and how many training graphs are cached -- and answers every
call with the oracle and numpy alone.  Training is oracle.sgd_pass_ordered over the canonical order of the current rating
set; that order, and the schedule arrays the getters are compared with, come from a throw-away handle of the same
configuration, created at the sizes the live handle had when it built the schedule, that does nothing but set_ratings and
the getters (reference_order, reference_schedule), never from the handle under test: the sequence decides when the live
handle's getters run.  Calls the handle is in no state for are kept: the model answers with the code the header gives,
and nothing may have changed.

Growth (add_users, add_items, reserve), online updates (partial_fit) and the cold-start path (fold_in / fold_in_items,
their rows appended) are ops like any other: they change the factors behind the schedule's back, the counts, the device
addresses of P and Q and whether the cached graphs are valid, and every later op is answered for the grown model.

The seen-item index (include/mfsgd.h, "the seen-item index") is part of the model: `seen` is None (the handle has no
index) or the sorted distinct keys u << 32 | i.  set_seen, mark_seen, clear_seen, seen_size, get_seen, the three serving
calls with exclude="seen" and partial_fit(seen=True) are ops; after EVERY op seen_size() is the model's, and after every op
the header says leaves the index as it is, or extends its per-user tables (SEEN_READ_AFTER), the whole index is read back
and compared.  (That read synchronises the stream when the index holds pairs, as get_factors would: the sequences keep
their stretches without an index, before the first set_seen and behind every clear_seen, for the missing-wait check.)

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
from tests.test_fold_in_items_gpu import fold_in_items_ref
from tests.test_rank_items_cpu import _assert_metrics as same_metrics
from tests.test_rank_items_cpu import _metrics_ref as metrics_ref
from tests.test_rank_items_gpu import _ranks_ref as ranks_ref
from tests.test_recommend_among_gpu import _ref_a as among_ref_a
from tests.test_recommend_among_gpu import _ref_b as among_ref_b
from tests.test_recommend_among_gpu import _same as same_among
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
               get_factors=2, add_users=4, add_items=4, reserve=4, partial_fit=4.5, fold_in_items=2, recommend_among=2,
               set_seen=3, mark_seen=4, clear_seen=2, seen_size=1.5, get_seen=2.5, recommend_unseen=2.5, rank_unseen=2,
               evaluate_unseen=2)
COMPUTE = ("fit", "train", "fit_schedule", "fit_bold_driver", "fit_early_stopping", "validation_rmse", "rmse_on", "rmse",
           "predict", "recommend", "recommend_excl", "rank_items", "similar_items", "similar_users", "fold_in",
           "partial_fit", "fold_in_items", "recommend_among", "recommend_unseen", "rank_unseen", "evaluate_unseen")
# ... of which the host profile draws these as often as the gpu profile: what they answer without a device is a rule too
# (an empty batch of online updates; "no seen set", which precedes the factor and device checks)
HOST_TOO = ("partial_fit", "recommend_unseen", "rank_unseen", "evaluate_unseen")
# the ops after which the whole index is read back: the header's "leave the index as it is" list, and the growth calls
SEEN_READ_AFTER = ("add_users", "add_items", "reserve", "set_ratings", "set_factors", "save_load", "init_factors",
                   "init_p_offset", "fit", "train", "fit_schedule", "fit_bold_driver", "fit_early_stopping", "fold_in",
                   "fold_in_items", "partial_fit")
# the error codes the model can answer with when there is a device, per kind (init_factors, set_factors, init_p_offset,
# set_hyper, set_validation, hyper, debug_counters, reserve, clear_seen and seen_size always succeed)
POSSIBLE_ERRORS = {kind: (STATE,) for kind in
                   ("fit", "train", "fit_schedule", "fit_bold_driver", "fit_early_stopping", "validation_rmse",
                    "rmse_on", "rmse", "predict", "recommend", "recommend_excl", "rank_items", "similar_items",
                    "similar_users", "fold_in", "order", "debug_schedule", "schedule_info", "get_factors",
                    "add_users", "add_items", "partial_fit", "fold_in_items", "recommend_among")}
POSSIBLE_ERRORS["set_ratings"] = (INVALID,)
for _kind in ("set_seen", "mark_seen"):
    POSSIBLE_ERRORS[_kind] = (INVALID,)
for _kind in ("get_seen", "recommend_unseen", "rank_unseen", "evaluate_unseen"):
    POSSIBLE_ERRORS[_kind] = (STATE,)
POSSIBLE_ERRORS["save_load"] = (STATE, INVALID)  # (INVALID: the file was saved before an append and no longer loads)
QUIET_NAN = 0x7FC00000
HOT = 9  # the row of set A that every row of the other side rates


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


def online_levels(u, i):
    """include/mfsgd.h, "online updates": (number of levels, ratings per level) of a batch that is one piece."""
    last_u, last_i, count = {}, {}, collections.Counter()
    for a, b in zip(u.tolist(), i.tolist()):
        level = max(last_u.get(a, 0), last_i.get(b, 0))
        count[level] += 1
        last_u[a] = last_i[b] = level + 1
    return len(count), [count[level] for level in range(len(count))]


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


def rating_sets(U, I, swap=False):
    """swap: both sets are drawn for (I, U) and u and i exchanged -- user 9 rates every item, and the schedule is built
    with the roles of P and Q exchanged."""
    if (U, I, swap) not in _sets:
        if swap:
            a, b = rating_set_a(I, U), rating_set_b(I, U)
            _sets[(U, I, swap)] = dict(A=(a[1], a[0], a[2]), B=(b[1], b[0], b[2]))
        else:
            _sets[(U, I, swap)] = dict(A=rating_set_a(U, I), B=rating_set_b(U, I))
    return _sets[(U, I, swap)]


def grown_set(g, base, U0, I0, U, I):
    """Set "C": the base set plus three ratings of every appended user (U0 .. U - 1) and of every appended item (I0 ..
    I - 1), no pair twice, shuffled."""
    bu, bi, br = base
    nu = np.concatenate([np.repeat(np.arange(U0, U), 3), g.integers(0, U, 3 * (I - I0))])
    ni = np.concatenate([g.integers(0, I, 3 * (U - U0)), np.repeat(np.arange(I0, I), 3)])
    key = np.unique(nu.astype(np.int64) * I + ni.astype(np.int64))  # (every new pair names an appended row: none is in the base)
    u = np.concatenate([bu, (key // I).astype(np.int32)])
    i = np.concatenate([bi, (key % I).astype(np.int32)])
    r = np.concatenate([br, (g.random(key.size) * 4 + 1).astype(np.float32)])
    p = g.permutation(u.size)
    return np.ascontiguousarray(u[p]), np.ascontiguousarray(i[p]), np.ascontiguousarray(r[p])


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
            ("get_factors", m.get_factors),
            ("apply_ratings", lambda: m.partial_fit([0], [1], [1.0])), ("apply_ratings", lambda: m.partial_fit([], [], [])),
            ("append_users", lambda: m.add_users(rows)), ("append_users", lambda: m.add_users(n=0)),
            ("append_items", lambda: m.add_items(n=2, seed=3)),
            ("fold_in_items", lambda: m.fold_in_items([0, 1], [0], [1.0], 1)),
            ("recommend_among", lambda: m.recommend([0], 1, candidates=[0, 1])),
            ("recommend_among", lambda: m.recommend([0, 1], 1, candidates=([0, 1, 1], [0]), exclude=([0], [0]))),
            ("recommend_rows_among", lambda: m.recommend_rows(rows, 1, candidates=[0])))


# -- the model and the driver ---------------------------------------------------------------------------------------------
class Runner:
    """One handle (self.m; None in a dry run) and its model.  Abstract state: R (ratings), F ("none", "ponly", "full"),
    V (a held-out set that is not empty), initialised (the Python wrapper's flag), builds, the live counts U and I (U0 and
    I0: what the handle was created with), res (the largest reserve per side), built_at (the counts at the latest schedule
    build), where ("none", "host", "device": csrc/handle.cpp's Where), graphs (cached training graphs), pending (what
    happened to the factors since the latest epoch), seen (None, or the index's sorted distinct keys u << 32 | i: drawn from
    the seed and the counts alone, so a dry run has them too), seen_moved (what happened to the index's per-user tables
    since its latest full read).  Numbers (not in a dry run): P, Q, lr, lam, ratings, val."""

    def __init__(self, mf, oracle, cfg, *, device, dry, wrong, tmpdir):
        self.mf, self.oracle, self.cfg, self.device, self.dry, self.wrong, self.tmpdir = mf, oracle, cfg, device, dry, wrong, tmpdir
        self.U, self.I, self.k = cfg["U"], cfg["I"], cfg["k"]
        self.U0, self.I0, self.res, self.built_at = self.U, self.I, [0, 0], (self.U, self.I)
        self.where, self.graphs, self.pending, self.appended_since_build = "none", 0, set(), False
        self.hyper_after_growth, self.no_upload = False, False
        self.seen, self.seen_moved, self.last_msg = None, set(), ""
        self.swap = bool(cfg.get("swap_roles"))
        self.sets = rating_sets(self.U, self.I, self.swap)
        self.group_lanes = 1
        while self.group_lanes < (self.k + 3) // 4:
            self.group_lanes <<= 1
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
                if kind not in HOST_TOO:
                    w[kind] *= 0.2
        if self.F == "full" and not self.grown():
            w["add_users"] *= 2
            w["add_items"] *= 2
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
        self.no_upload = False
        code = getattr(self, "op_" + kind)(np.random.default_rng(seed))
        if code == OK and kind in COMPUTE and not self.no_upload:
            self.uploaded()
        self.check_seen_size()
        if kind in SEEN_READ_AFTER:
            self.check_seen_lists()
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
        self.last_msg = msg
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
        """A call that went through prepare_compute: the factors and the schedule are on the device; `epochs` epochs ran."""
        from mfsgd_amd import _lib

        self.sched_computed = self.any_compute = True
        self.uploaded()
        if epochs > 0 and self.lone():
            self.facts["trained_on_a_lone_tile_schedule"] += 1
        if epochs > 0 and self.ratings[0].size > 0:
            # csrc/train.cpp, launch_epoch: one graph per (P, Q) pair of addresses, with round launches too; none
            # under FLAG_NO_GRAPH, and none for an empty set, which launches nothing
            self.graphs = 0 if self.cfg["flags"] & _lib.FLAG_NO_GRAPH else 1
            for what in sorted(self.pending):
                self.facts["fit_after_" + what] += 1
            self.pending.clear()
            if self.hyper_after_growth:
                self.facts["set_hyper_after_growth_then_fit"] += 1
            self.hyper_after_growth = False
            if self.grown() and self.swapped():
                self.facts["trained_on_a_swapped_schedule_after_growth"] += 1
            if self.grown():
                self.facts["trained_after_growth"] += 1

    def uploaded(self):
        """A compute call succeeded: csrc/handle.cpp, factors_to_device."""
        if self.device and self.where == "host":
            self.where = "device"

    def seeded_or_replaced(self, seeded):
        """mfsgd_init_factors / mfsgd_init_p_offset (seeded: on the device where there is one) or mfsgd_set_factors /
        mfsgd_load_factors (host staging): the device copies, and every graph captured with their addresses, are gone."""
        self.where = "device" if seeded and self.device else "host"
        self.graphs = 0
        self.pending.clear()

    def grown(self):
        return self.U > self.U0 or self.I > self.I0

    def capacity(self):
        return max(self.U, self.res[0]), max(self.I, self.res[1])

    def check_counts(self):
        """The counts, the capacity and the cached graphs, after every op that can change them."""
        if not self.dry:
            assert (self.m.users, self.m.items) == (self.U, self.I), ((self.m.users, self.m.items), (self.U, self.I))
            assert self.m.capacity() == self.capacity(), (self.m.capacity(), self.capacity())
            got = self.m.debug_counters()
            assert got["graphs"] == self.graphs, f"{got['graphs']} cached training graphs, the model expects {self.graphs}"
            assert got["schedule_builds"] == self.builds, (got, self.builds)

    def ref_cfg(self):
        """The configuration of the throw-away handle: the sizes the live handle had when it built the current schedule
        (include/mfsgd.h: a handle created at the grown size may cut its blocks differently)."""
        return dict(self.cfg, U=self.built_at[0], I=self.built_at[1])

    def ref_schedule(self, lr, lam):
        return reference_schedule(self.mf, self.ref_cfg(), self.ratings, self.digest, lr, lam)

    def base(self):
        """"A" or "B" for those sets, their edits and the sets C made from them; None for the empty set."""
        return self.name[0] if self.R and self.name[0] in "AB" else None

    def packed(self):
        """The schedule's arrays were packed on the device and (until the first compute call) belong to it."""
        from mfsgd_amd import _lib

        guess = bool(self.cfg["flags"] & _lib.FLAG_DEVICE_INGEST) and self.device and self.ratings[0].size > 0
        if self.dry:
            return guess
        return self.ref_schedule(self.cfg["lr"], self.cfg["lam"])["info"]["device_ingest"] == 2

    def lone(self):
        guess = self.cfg["blocks"] > 0 and self.name.startswith("A")
        if self.dry:
            return guess and "+C" not in self.name
        got = self.ref_schedule(self.cfg["lr"], self.cfg["lam"])["lone"]
        if self.cfg["blocks"] > 0 and "+C" not in self.name:  # (a set C is built at grown sizes: its cells are cut anew)
            assert got == guess, f"set {self.name}: lone-tile cells {got}, expected {guess}"
        return got

    def swapped(self):
        """The schedule was built with the roles of P and Q exchanged: the training kernels receive (Q, P)."""
        if self.dry or self.ratings[0].size == 0:
            return self.swap and self.ratings[0].size > 0
        got = self.ref_schedule(self.cfg["lr"], self.cfg["lam"])["info"]["swapped"] == 1
        assert got == self.swap, f"set {self.name}: swapped {got}, expected {self.swap}"
        return got

    def order(self):
        return reference_order(self.mf, self.oracle, self.ref_cfg(), self.ratings, self.digest)[0]

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
        if self.wrong == "append_forgets_the_ratings" and self.appended_since_build:
            reuse = False
        if not reuse:
            self.builds += 1
            self.sched_computed = False
            self.built_at, self.appended_since_build, self.hyper_after_growth = (self.U, self.I), False, False
            self.graphs = 0  # (the partition, and the graphs it cached, are new)
            self.pending.clear()
            if self.after_failure and self.last_valid and digest == _digest(*self.last_valid[1]):
                self.facts["set_ratings_build_of_the_set_a_failed_call_dropped"] += 1
            if "+C" in name:
                self.facts["set_ratings_build_naming_appended_rows"] += 1
        elif self.appended_since_build:
            self.facts["set_ratings_reuse_after_growth"] += 1  # (the reference handle keeps the sizes of the build)
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
        if v == "C":  # only after growth: set A or B and a few ratings of every appended row, drawn anew every time
            if self.grown():
                base = "AB"[int(g.integers(2))]
                return v, f"{base}+C{self.U}x{self.I}", grown_set(g, self.sets[base], self.U0, self.I0, self.U, self.I)
            v = "A"
        return v, v, self.sets[v]

    def op_set_ratings(self, g):
        variants = ("A", "A", "B", "B", "again", "again", "again", "edit", "edit", "empty", "bad", "bad", "C", "C", "C")
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
                self.graphs, self.appended_since_build, self.hyper_after_growth = 0, False, False
                self.pending.clear()
            self.last_valid = (name, valid)  # "again" sends the same triples, valid as before: they must be built again
            return code
        v, name, triples = self.pick_set(g, ("A", "A", "B", "B", "again", "again", "again", "edit", "edit", "empty", "C", "C", "C"))
        self.note(f"[{v}: {name}, n={triples[0].size}]")
        equal_length = self.R and triples[0].size == self.ratings[0].size
        code, _ = self.call(OK, lambda: self.m.set_ratings(*triples))
        reuse = self.apply_set(name, triples)
        if v == "edit" and equal_length and not reuse:
            self.facts["set_ratings_rebuild_of_equal_length"] += 1
        if v == "C" and "+C" in name:
            assert not reuse, "a set C is drawn anew: it is never the set in place"
        if not self.dry:
            assert self.m.debug_counters()["schedule_builds"] == self.builds, (self.m.debug_counters(), self.builds, reuse)
            if self.ratings[0].size:
                self.swapped()  # (asserts the role decision of the reference handle at the build's sizes)
        return code

    # .. factors .......................................................................................................
    def op_init_factors(self, g):
        seed = int(g.integers(1, 1000))
        code, _ = self.call(OK, lambda: self.m.init_factors(seed))
        self.F, self.initialised = "full", True
        self.seeded_or_replaced(True)
        if self.grown():
            self.facts["init_factors_after_growth"] += 1  # at the grown counts; the capacity is kept
        if not self.dry:
            U, I = (self.U0, self.I0) if self.wrong == "reseed_forgets_growth" else (self.U, self.I)
            self.P, self.Q = self.oracle.init_factors(U, I, self.k, seed)
        self.check_counts()
        return code

    def op_set_factors(self, g):
        P = (g.standard_normal((self.U, self.k)) * 0.1).astype(np.float32)
        Q = (g.standard_normal((self.I, self.k)) * 0.1).astype(np.float32)
        code, _ = self.call(OK, lambda: self.m.set_factors(P, Q))
        self.F, self.initialised, self.P, self.Q = "full", True, P, Q
        self.seeded_or_replaced(False)
        if self.wrong == "set_factors_clears_the_index":
            self.seen = None
        self.check_counts()
        return code

    def op_save_load(self, g):
        """save_factors, factors of another seed, load_factors: the model keeps what it had.  Or (stale): save_factors, one
        row appended, load_factors -- the file has the shape of before, MFSGD_ERR_INVALID_ARG, and the model keeps the
        grown factors."""
        self.n_files += 1
        path = os.path.join(self.tmpdir, f"factors{self.n_files}.bin")
        stale, side, seed = int(g.integers(4)) == 0, int(g.integers(2)), int(g.integers(1000, 2000))
        code, _ = self.call(OK if self.F == "full" else STATE, lambda: self.m.save_factors(path))
        if code == OK and stale:
            self.note(f"[stale: one {'item' if side else 'user'} appended behind the save]")
            self.append(side, None, 1, seed)
            code, _ = self.call(INVALID, lambda: self.m.load_factors(path))
            self.facts["stale_factor_file_refused"] += 1
        elif code == OK:
            if not self.dry:
                self.m.init_factors(seed)
                self.m.load_factors(path)
            self.seeded_or_replaced(False)
        self.check_counts()
        return code

    def op_init_p_offset(self, g):
        """mfsgd_init_p_offset on a single-partition handle: P of the offset, no Q, and every call that reads the
        handle's Q is MFSGD_ERR_STATE before anything is launched (tests/test_capi_cpu.py has the list)."""
        seed, off = int(g.integers(1, 1000)), int(g.integers(0, 50))
        self.note(f"[seed {seed}, offset {off}]")
        code, _ = self.call(OK, lambda: self.m.init_p_offset(seed, off))
        self.F, self.initialised, self.Q = "ponly", True, None
        self.seeded_or_replaced(True)
        self.check_counts()
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
            self.seeded_or_replaced(True)
            if not self.dry:
                self.P, self.Q = self.oracle.init_factors(self.U, self.I, self.k, self.cfg["seed"])
        code = self.fit(n, True, lambda: self.m.train(*triples, n))
        self.check_counts()
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
            self.graphs = 0  # (the rate of the NEXT epoch is set behind the last one, as by set_hyper: the graph goes)
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
        min_delta = (0.0, 0.3, 0.3)[int(g.integers(3))]  # (0.3: more than an epoch gains, so an earlier epoch stays the best)
        self.note(f"[max {max_epochs}, patience {patience}, min_delta {min_delta}, restore {restore}, lr given={lrs is not None}, "
                  f"train rmse={with_train}]")
        if not self.R or not self.V or self.F != "full":
            want = STATE
        else:
            want = OK if self.device else NO_DEVICE
        code, res = self.call(want, lambda: self.m.fit_early_stopping(max_epochs, patience=patience, min_delta=min_delta,
                                                                      restore_best=restore, lr=lrs, train_rmse=with_train))
        if code == OK:
            self.computed(1)
            self.measured_validation()
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
                    if v < best - min_delta:
                        best, best_epoch, bad, snap = v, e, 0, (self.P.copy(), self.Q.copy())
                    else:
                        bad += 1
                        if bad >= patience:
                            break
                assert (res["epochs_run"], res["best_epoch"], len(res["val_rmse"])) == (ran, best_epoch, ran), (res, ran, best_epoch)
                assert (res["train_rmse"] is None) == (not with_train)
                if restore and best_epoch >= 0 and best_epoch != ran - 1:
                    self.P, self.Q = snap  # (the snapshot is of the rows the model has now)
                    self.note("[restored]")
                    if self.grown():
                        self.facts["early_stopping_restored_after_growth"] += 1
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
                self.graphs = 0
                if self.appended_since_build:
                    self.hyper_after_growth = True  # (a schedule kept across an append is re-baked)
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
        """n pairs over the current counts; after growth one in eight names an appended row."""
        u, i = g.integers(0, self.U, n).astype(np.int32), g.integers(0, self.I, n).astype(np.int32)
        if self.U > self.U0:
            u[0::8] = g.integers(self.U0, self.U, u[0::8].size)
        if self.I > self.I0:
            i[4::8] = g.integers(self.I0, self.I, i[4::8].size)
        return u, i, (g.integers(1, 11, n) * 0.5).astype(np.float32)

    def appended_rows(self, g, side, n):
        """n indices of one side, an appended row among them where there is one."""
        count, first = ((self.U, self.U0), (self.I, self.I0))[side]
        x = g.integers(0, count, n).astype(np.int32)
        if count > first and n > 1:
            x[1] = g.integers(first, count)
        return x

    def measured_validation(self):
        if self.V and ((self.val[0] >= self.U0).any() or (self.val[1] >= self.I0).any()):
            self.facts["validation_pair_on_an_appended_row"] += 1  # (the set survived the append, or was given after it)

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
        self.no_upload = not self.V  # (an empty set is answered without the device)
        if code == OK:
            self.measured_validation()
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
        users = self.appended_rows(g, 0, 4)
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
        q = self.appended_rows(g, 1, 6)
        code, got = self.call(self.code_pq(True), lambda: self.m.similar_items(q, 4))
        if code == OK and not self.dry:
            rn = inv_norms_ref(self.oracle, self.Q)
            same_topn(got, similar_ref(self.oracle, self.Q, rn, q, self.Q, rn, 4, True))
        return code

    def op_similar_users(self, g):
        q = self.appended_rows(g, 0, 8)
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
        """fold_in of five new users, then recommend_rows for the rows it returned, their own items left out -- over the
        whole catalogue or among a candidate list per row -- and, in a drawn half, the rows appended as users."""
        lens = g.integers(0, 13, 5)
        row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        items = g.integers(0, self.I, int(row_ptr[-1])).astype(np.int32)
        ratings = g.uniform(0.5, 5.0, items.size).astype(np.float32)
        epochs, seeded = int(g.integers(0, 3)), bool(g.integers(2))
        seed = int(g.integers(1, 1000))
        init = None if seeded else g.standard_normal((5, self.k)).astype(np.float32)
        append, among = bool(g.integers(2)), bool(g.integers(2))
        lists = [self.appended_rows(g, 1, int(n)) for n in g.integers(0, 20, 5)]  # (per row; short and empty ones are padded)
        self.note(f"[{epochs} epochs, {items.size} ratings, seeded={seeded}, appended={append}, among candidates={among}]")
        code, rows = self.call(self.code_pq(True), lambda: self.m.fold_in(row_ptr, items, ratings, epochs, init=init, seed=seed))
        if code == OK:
            self.uploaded()
            want = None
            if not self.dry:
                R0 = self.oracle.init_factors(5, 0, self.k, seed)[0] if seeded else init
                want = fold_in_ref(self.oracle, self.Q, row_ptr, items, ratings, epochs, R0, float(self.lr), float(self.lam))
                _same_bits(rows, want, "fold_in rows")
                er = np.repeat(np.arange(5, dtype=np.int32), lens).astype(np.int32)
                if among:
                    got = self.m.recommend_rows(rows, 4, exclude=(er, items), candidates=lists)
                    predict = lambda row, i: self.oracle.predict(want, self.Q, row, i)
                    same_among(got, among_ref_b(predict, np.arange(5, dtype=np.int32), lists, 4, er, items))
                else:
                    got = self.m.recommend_rows(rows, 4, exclude=(er, items))
                    same_topn(got, recommend_ref(self.oracle, want, self.Q, np.arange(5, dtype=np.int32), 4, er, items))
            if append:  # the cold-start path end to end: the folded rows become users of the model
                self.append(0, want, 5, None)
        return code

    def op_fold_in_items(self, g):
        """fold_in_items of five new items against the fixed P, then what serving makes of the rows it returned: the items
        most like them (similar_rows), or the users' scores among candidates once they are appended."""
        lens = g.integers(0, 13, 5)
        row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        users = g.integers(0, self.U, int(row_ptr[-1])).astype(np.int32)
        ratings = g.uniform(0.5, 5.0, users.size).astype(np.float32)
        epochs, seeded = int(g.integers(0, 3)), bool(g.integers(2))
        seed = int(g.integers(1, 1000))
        init = None if seeded else g.standard_normal((5, self.k)).astype(np.float32)
        append = bool(g.integers(2))
        asked = self.appended_rows(g, 0, 3)
        self.note(f"[{epochs} epochs, {users.size} ratings, seeded={seeded}, appended={append}]")
        code, rows = self.call(self.code_pq(True), lambda: self.m.fold_in_items(row_ptr, users, ratings, epochs, init=init, seed=seed))
        if code == OK:
            self.uploaded()
            want = None
            if not self.dry:
                R0 = self.oracle.init_factors(5, 0, self.k, seed)[0] if seeded else init
                want = fold_in_items_ref(self.oracle, self.P, row_ptr, users, ratings, epochs, R0, float(self.lr), float(self.lam))
                _same_bits(rows, want, "fold_in_items rows")
                rn = inv_norms_ref(self.oracle, self.Q)
                got = self.m.similar_rows(rows, 4, side="items")
                same_topn(got, similar_ref(self.oracle, want, inv_norms_ref(self.oracle, want), np.arange(5), self.Q, rn, 4, False))
            if append:  # the cold-start path end to end: the folded rows become items, and candidates
                first = self.I
                self.append(1, want, 5, None)
                cand = np.arange(first - 2, first + 5, dtype=np.int32)
                if not self.dry:
                    got = self.m.recommend(asked, 3, candidates=cand)
                    same_among(got, among_ref_b(lambda u, i: self.oracle.predict(self.P, self.Q, u, i), asked, [cand] * 3, 3))
        return code

    def op_recommend_among(self, g):
        """recommend(users, n, candidates=...): one shared list or a list per request row, with and without exclusions;
        lists that are short (padded), empty, unsorted, with repeats, and with an appended item where there is one --
        against the whole-catalogue order filtered on the host (_ref_a) and against sorted predictions (_ref_b)."""
        users = self.appended_rows(g, 0, 4)
        users[3] = users[0]  # one user twice, with a list of its own in the per-row form
        shared, excl, topn = bool(g.integers(2)), bool(g.integers(2)), int(g.integers(1, 8))
        lists = [self.appended_rows(g, 1, int(n)) for n in g.integers(0, 30, 4)]
        lists[1] = lists[1][:2]                                  # shorter than topn, mostly: padded
        lists[2] = lists[2][:0]                                  # empty: all padding
        lists[0] = np.concatenate([lists[0], lists[0][:3]])      # repeats
        if shared:
            lists = [lists[int(g.integers(4))]] * 4
        eu, ei = self.exclusions() if excl else (np.empty(0, np.int32),) * 2
        self.note(f"[shared={shared}, exclude={excl}, topn {topn}, lists of {[int(c.size) for c in lists]}]")
        cand = lists[0] if shared else ([np.asarray(c) for c in lists] if g.integers(2) else
                                        (np.concatenate([[0], np.cumsum([c.size for c in lists])]).astype(np.int64), np.concatenate(lists)))
        code, got = self.call(self.code_pq(False), lambda: self.m.recommend(users, topn, exclude=(eu, ei) if excl else None,
                                                                            candidates=cand))
        if code == OK and not self.dry:
            full = recommend_ref(self.oracle, self.P, self.Q, users, self.I, eu, ei)
            same_among(got, among_ref_a(full, lists, topn), "against the filtered whole-catalogue order")
            predict = lambda u, i: self.oracle.predict(self.P, self.Q, u, i)
            same_among(got, among_ref_b(predict, users, lists, topn, eu, ei), "against sorted predictions")
        return code

    # .. the seen-item index ...........................................................................................
    def seen_pairs(self):
        """(u, i) int32 of the model's index."""
        keys = np.empty(0, np.int64) if self.seen is None else self.seen
        return (keys >> 32).astype(np.int32), (keys & 0xFFFFFFFF).astype(np.int32)

    def seen_merge(self, u, i):
        keys = np.unique((np.asarray(u, np.int64) << 32) | np.asarray(i, np.int64))
        self.seen = keys if self.seen is None else np.union1d(self.seen, keys)

    def seen_lists(self, users):
        """(row_ptr int64[len(users) + 1], items int32): what seen(users) returns."""
        users = np.asarray(users, np.int64)
        lo, hi = np.searchsorted(self.seen, users << 32), np.searchsorted(self.seen, (users + 1) << 32)
        ptr = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64)
        items = [self.seen[a:b] & 0xFFFFFFFF for a, b in zip(lo, hi)]
        return ptr, (np.concatenate(items) if items else np.empty(0, np.int64)).astype(np.int32)

    def check_seen_size(self):
        """After every op: seen_size() is the model's (-1: no index).  Host only."""
        if not self.dry:
            got, want = self.m.seen_size(), -1 if self.seen is None else int(self.seen.size)
            assert got == want, f"seen_size() is {got}, the model's index holds {want}"

    def check_seen_lists(self):
        """The whole index, read back: seen(arange(U)) equals the model.  (An empty index is read on the host.)"""
        if self.seen is None:
            self.seen_moved.clear()
            return
        if not self.dry:
            got = self.m.seen(np.arange(self.U, dtype=np.int32))
            want = self.seen_lists(np.arange(self.U))
            assert got[0].dtype == np.int64 and got[1].dtype == np.int32
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), \
                f"seen(every user) differs from the model: {got[1].size} items, the model holds {want[1].size}"
        for what in sorted(self.seen_moved):
            self.facts["seen_read_after_" + what] += 1
        self.seen_moved.clear()

    def seen_update(self, g, merge):
        """set_seen (merge False) / mark_seen: a valid batch, an empty one, one wholly inside the index, one with a pair
        out of range at a drawn position.  csrc/seen_index.cpp: the pairs are checked first (MFSGD_ERR_INVALID_ARG, "pair
        N out of range"); n == 0 is answered on the host; n > 0 needs a device; a refused call leaves the index alone."""
        host = self.cfg.get("profile", "gpu") == "host"
        variants = ("some", "inside", "empty", "empty", "empty", "bad") if host else ("some", "some", "some", "empty", "inside", "bad")
        v = variants[int(g.integers(len(variants)))]
        n = int(g.integers(1, 400))
        u, i, _ = self.pairs(g, n)
        pick, j, which = g.integers(0, 1 << 30, n), int(g.integers(n)), int(g.integers(2))
        if v == "inside":
            if self.seen is not None and self.seen.size:
                keys = self.seen[pick % self.seen.size]
                u, i = (keys >> 32).astype(np.int32), (keys & 0xFFFFFFFF).astype(np.int32)
            else:
                v = "some"
        if v == "empty":
            u, i = u[:0], i[:0]
        if v == "bad":
            if which:
                u[j] = self.U
            else:
                i[j] = self.I
        name = "mark_seen" if merge else "set_seen"
        self.note(f"[{v}: n={u.size}" + (f", pair {j} out of range]" if v == "bad" else "]"))
        want = INVALID if v == "bad" else OK if self.device or u.size == 0 else NO_DEVICE
        fn = (lambda: self.m.mark_seen(u, i)) if merge else (lambda: self.m.set_seen(u, i))
        before = None if self.seen is None else self.seen.size
        code, _ = self.call(want, fn)
        if code == INVALID and not self.dry:
            assert f"{name}: pair {j} out of range" in self.last_msg, self.last_msg
        if code == OK:
            if merge:
                if u.size and (u >= self.U0).any():
                    self.facts["mark_seen_of_an_appended_user"] += 1
                if u.size and (i >= self.I0).any():
                    self.facts["mark_seen_of_an_appended_item"] += 1
                self.seen_merge(u, i)  # (of nothing, on a handle without an index: an empty index)
                if v == "inside":
                    assert self.seen.size == before
                    self.facts["mark_seen_wholly_inside_the_index"] += 1
            else:
                if before:
                    self.facts["set_seen_replacing_a_non_empty_index"] += 1
                self.seen = None
                self.seen_merge(u, i)
            if u.size == 0:
                self.facts[name + "_of_no_pairs"] += 1
        else:  # refused: the index is as it was, all of it
            if merge and before:
                self.facts["refused_mark_seen_then_read"] += 1
            self.check_seen_lists()
        return code

    def op_set_seen(self, g):
        return self.seen_update(g, False)

    def op_mark_seen(self, g):
        return self.seen_update(g, True)

    def op_clear_seen(self, g):
        code, _ = self.call(OK, lambda: self.m.clear_seen())
        self.seen = None
        self.seen_moved.clear()
        return code

    def op_seen_size(self, g):
        code, got = self.call(OK, lambda: self.m.seen_size())
        if not self.dry:
            assert got == (-1 if self.seen is None else self.seen.size), (got, self.seen)
        return code

    def op_get_seen(self, g):
        """seen(users) for drawn users, with repeats, or for none.  A handle without an index: MFSGD_ERR_STATE; an empty
        index and zero users are answered on the host."""
        n = int(g.integers(0, 9))
        users = self.appended_rows(g, 0, n)
        if n > 2:
            users[2] = users[0]
        self.note(f"[{n} users]")
        if self.seen is None:
            want = STATE
        else:
            want = OK if self.device or n == 0 or self.seen.size == 0 else NO_DEVICE
        code, got = self.call(want, lambda: self.m.seen(users))
        if code == STATE and not self.dry:
            assert "get_seen: no seen set" in self.last_msg, self.last_msg
        if code == OK:
            if self.seen.size == 0 or n == 0:
                self.facts["get_seen_answered_on_the_host"] += 1
            if not self.dry:
                want_ptr, want_items = self.seen_lists(users)
                assert np.array_equal(got[0], want_ptr) and np.array_equal(got[1], want_items), (got, want_ptr, want_items)
        return code

    def code_unseen(self, none_first):
        """The serving calls against the index: "no seen set" comes before every factor and device check."""
        if self.seen is None:
            if self.F != "full":
                self.facts["unseen_refused_for_no_seen_set_without_factors"] += 1
            return STATE
        return self.code_pq(none_first)

    def unseen_outcome(self, code, name):
        if code == STATE and self.seen is None and not self.dry:
            assert f"{name}: no seen set" in self.last_msg, self.last_msg
        if code == OK and self.seen.size == 0:
            self.facts["unseen_call_on_an_empty_index"] += 1  # (it excludes nothing)

    def op_recommend_unseen(self, g):
        """recommend(users, n, exclude="seen"), over the whole catalogue or among drawn candidates (one shared list or one
        per row; empty, short and repeating ones), against the references of recommend_excl / recommend_among given the
        model's pairs."""
        users = self.appended_rows(g, 0, 4)
        users[3] = users[0]
        among, shared, topn = bool(g.integers(2)), bool(g.integers(2)), int(g.integers(1, 8))
        lists = [self.appended_rows(g, 1, int(n)) for n in g.integers(0, 30, 4)]
        lists[1] = lists[1][:2]
        lists[2] = lists[2][:0]
        lists[0] = np.concatenate([lists[0], lists[0][:3]])
        if shared:
            lists = [lists[int(g.integers(4))]] * 4
        self.note(f"[among={among}, shared={shared}, topn {topn}, lists of {[int(c.size) for c in lists]}]")
        cand = None
        if among:
            cand = lists[0] if shared else (np.concatenate([[0], np.cumsum([c.size for c in lists])]).astype(np.int64),
                                            np.concatenate(lists))
        code, got = self.call(self.code_unseen(False), lambda: self.m.recommend(users, topn, exclude="seen", candidates=cand))
        self.unseen_outcome(code, "recommend_unseen_among" if among else "recommend_unseen")
        if code == OK and not self.dry:
            eu, ei = self.seen_pairs()
            if among:
                predict = lambda u, i: self.oracle.predict(self.P, self.Q, u, i)
                same_among(got, among_ref_b(predict, users, lists, topn, eu, ei), "against sorted predictions")
            else:
                same_topn(got, recommend_ref(self.oracle, self.P, self.Q, users, topn, eu, ei))
        return code

    def op_rank_unseen(self, g):
        u, i, _ = self.pairs(g, 12)
        code, got = self.call(self.code_unseen(True), lambda: self.m.rank_items(u, i, exclude="seen"))
        self.unseen_outcome(code, "rank_items_unseen")
        if code == OK and not self.dry:
            assert np.array_equal(got, ranks_ref(self.oracle, self.P, self.Q, u, i, *self.seen_pairs())), got
        return code

    def op_evaluate_unseen(self, g):
        u, i, _ = self.pairs(g, 12)
        topn = int(g.integers(1, 20))
        code, got = self.call(self.code_unseen(True), lambda: self.m.evaluate_ranking(u, i, topn, exclude="seen"))
        self.unseen_outcome(code, "evaluate_ranking_unseen")
        if code == OK and not self.dry:
            ranks = ranks_ref(self.oracle, self.P, self.Q, u, i, *self.seen_pairs())
            assert np.array_equal(got["ranks"], ranks), got
            same_metrics(got, metrics_ref(u, ranks, topn))
        return code

    # .. growth ........................................................................................................
    def append(self, side, rows, n, seed):
        """add_users (side 0) / add_items (side 1) of `rows`, or of n seeded rows, against the handle and the model; returns
        the code.  csrc/handle.cpp, append_rows: MFSGD_ERR_STATE without factors or without Q, before anything else that
        can happen here; *first is the old count; n_new == 0 touches nothing."""
        old = (self.U, self.I)[side]
        n_new = n if rows is None else rows.shape[0]
        add = None if self.dry else (self.m.add_items if side else self.m.add_users)
        fn = (lambda: add(n=n_new, seed=seed)) if seed is not None else (lambda: add(rows))
        code, first = self.call(OK if self.F == "full" else STATE, fn)
        if code == OK and not self.dry:
            assert first == old, (first, old)
        if code == OK and n_new > 0:
            if self.where == "device":
                if old + n_new > self.capacity()[side]:  # to a new buffer: the graphs hold the dead address
                    self.graphs = 0
                    self.pending.add("reallocating_append")
                else:                                    # in place: P and Q stay where they are, and so do the graphs
                    self.pending.add("append_in_place")
            else:
                self.facts["append_on_host_staging"] += 1
            if self.R:
                self.appended_since_build = True
                if self.packed() and not self.sched_computed:
                    self.facts["append_on_a_device_packed_schedule_before_compute"] += 1
            if side == 0 and self.seen is not None and self.seen.size:
                # the new users have empty lists; beyond the capacity the per-user tables are copied into larger ones
                if old + n_new <= self.capacity()[0]:
                    self.seen_moved.add("an_append_in_place")
                else:
                    self.seen_moved.add("a_reallocating_append_on_" + ("the_device" if self.where == "device" else "host_staging"))
                if self.wrong == "append_users_gives_new_users_the_last_list":
                    last = self.seen[(self.seen >> 32) == old - 1] & 0xFFFFFFFF
                    new = (np.arange(old, old + n_new, dtype=np.int64)[:, None] << 32) | last[None, :]
                    self.seen = np.union1d(self.seen, new.ravel())
            if side:
                self.I += n_new
            else:
                self.U += n_new
            if not self.dry:
                if seed is not None:
                    rows = self.oracle.init_factors(n_new, 0, self.k, seed)[0]
                rows = np.array(rows, np.float32)
                rows.view(np.uint32)[np.isnan(rows)] = QUIET_NAN  # (as mfsgd_set_factors: no payload of the caller's is kept)
                if side:
                    self.Q = np.vstack([self.Q, rows])
                else:
                    self.P = np.vstack([self.P, rows])
        self.check_counts()
        return code

    def add(self, g, side):
        n = 0 if int(g.integers(6)) == 0 else int(g.integers(1, 41))
        given, seed = bool(g.integers(2)), int(g.integers(1, 1000))
        rows = (g.standard_normal((n, self.k)) * 0.1).astype(np.float32)
        nan = given and n > 0 and int(g.integers(4)) == 0
        if nan:
            rows.view(np.uint32)[int(g.integers(n)), int(g.integers(self.k))] = 0x7FFFFFFF
        self.note(f"[{n} rows, {'given' if given else f'seed {seed}'}{', a NaN among them' if nan else ''}]")
        code = self.append(side, rows if given else None, n, None if given else seed)
        if code == OK and nan:
            # The NaN went in as 0x7FC00000: read back at once.  It does not stay: the header leaves ranks, the bold driver
            # and the order of NaN scores unspecified for a model that holds one, so the rows are given again without it.
            self.facts["append_of_a_nan"] += 1
            if not self.dry:
                got = self.m.get_factors()
                _same_bits(got[0], self.P, "P behind an append with a NaN")
                _same_bits(got[1], self.Q, "Q behind an append with a NaN")
                assert np.isnan((self.Q if side else self.P)[-n:]).sum() == 1
                np.nan_to_num(self.P, copy=False, nan=0.25)
                np.nan_to_num(self.Q, copy=False, nan=0.25)
                self.m.set_factors(self.P, self.Q)
            self.seeded_or_replaced(False)
            self.check_counts()
        return code

    def op_add_users(self, g):
        return self.add(g, 0)

    def op_add_items(self, g):
        return self.add(g, 1)

    def op_reserve(self, g):
        """mfsgd_reserve_rows for one side or both: below, at and above the capacity, 0, or None (that side left alone).
        With the factors on the device a larger capacity is a new buffer now, and the graphs go."""
        sides = ((0,), (1,), (0, 1))[int(g.integers(3))]
        want = [None, None]
        for side in sides:
            cap = self.capacity()[side]
            v = ("below", "at", "above", "above", "zero")[int(g.integers(5))]
            want[side] = dict(below=cap - int(g.integers(1, 20)), at=cap, above=cap + int(g.integers(1, 120)), zero=0)[v]
        self.note(f"[users {want[0]}, items {want[1]}; capacity {self.capacity()}]")
        code, _ = self.call(OK, lambda: self.m.reserve(users=want[0], items=want[1]))
        for side in sides:
            if want[side] > self.capacity()[side]:
                if side == 0 and self.seen is not None and self.seen.size:
                    self.seen_moved.add("reserve")  # (the index's per-user tables are as long as the capacity)
                if self.where == "device" and (side == 0 or self.F == "full"):  # (that side has a buffer: it moves)
                    self.graphs = 0
                    self.facts["reserve_that_reallocates"] += 1
                self.res[side] = want[side]
                self.facts["reserve_above_the_capacity"] += 1
        self.check_counts()
        return code

    # .. online updates ................................................................................................
    def op_partial_fit(self, g):
        """partial_fit of 0 .. 300 ratings over the current counts: some on the hot row of set A, some on appended rows,
        pairs repeated (several levels), and in a third of the draws a first level wider than one workgroup pass, so that
        both kernels of csrc/online.hip run.  The model is the sequential loop; the errors compare bit for bit."""
        none = int(g.integers(2 if self.cfg.get("profile", "gpu") == "host" else 8)) == 0
        n = 0 if none else int(g.integers(1, 301))
        u, i = g.integers(0, self.U, n).astype(np.int32), g.integers(0, self.I, n).astype(np.int32)
        r = (g.integers(1, 11, n) * 0.5).astype(np.float32)
        hot = self.base() == "A" and n > 0
        if hot:
            (u if self.swap else i)[g.integers(0, n, n // 4 + 1)] = HOT
        on_new = self.grown() and n > 0
        if self.U > self.U0 and n > 0:
            u[g.integers(0, n, n // 6 + 1)] = g.integers(self.U0, self.U, n // 6 + 1)
        if self.I > self.I0 and n > 0:
            i[g.integers(0, n, n // 6 + 1)] = g.integers(self.I0, self.I, n // 6 + 1)
        if n > 4:  # the same pair three times more
            at = g.integers(0, n, 4)
            u[at[1:]], i[at[1:]] = u[at[0]], i[at[0]]
        per_pass = 256 // self.group_lanes
        wide = n > 0 and int(g.integers(3)) == 0 and min(self.U, self.I) > per_pass + 8
        if wide:  # per_pass + 9 ratings that share no row, in front: level 0 of the batch
            wu, wi = g.choice(self.U, per_pass + 9, replace=False), g.choice(self.I, per_pass + 9, replace=False)
            u, i = np.concatenate([wu, u]).astype(np.int32), np.concatenate([wi, i]).astype(np.int32)
            r = np.concatenate([np.full(per_pass + 9, 3.5, np.float32), r])
            n = u.size
        check_order = bool(g.integers(2))
        mark = int(g.integers(3)) == 0  # partial_fit(seen=True): the applied pairs are marked behind the update
        n_levels, widths = online_levels(u, i)
        width = max(widths, default=0)
        wide = width > per_pass  # (a random batch can have such a level without the rows in front)
        narrow = n > 0 and min(widths) <= per_pass
        self.note(f"[n={n}, hot={hot}, appended rows={on_new}, {n_levels} levels, the widest of {width}, seen={mark}]")
        if self.F != "full":
            want = STATE
        else:
            want = OK if self.device or n == 0 else NO_DEVICE
        code, got = self.call(want, lambda: self.m.partial_fit(u, i, r, errors=True, info=True, seen=mark))
        self.no_upload = n == 0
        if mark:
            # trainer.py: mark_seen runs behind mfsgd_apply_ratings, so a refused update (it raises) marks nothing, and
            # an applied one marks exactly its pairs -- no pairs, on a handle without an index, leave an empty index
            self.facts["partial_fit_seen_" + ("applied" if code == OK else "refused")] += 1
            if code == OK:
                self.seen_merge(u, i)
        if code == OK and n == 0:
            self.facts["partial_fit_of_no_ratings"] += 1
        if code == OK and n > 0:
            self.pending.add("partial_fit")
            if on_new:
                self.facts["partial_fit_on_an_appended_row"] += 1
            if wide:
                self.facts["partial_fit_with_a_wide_level"] += 1
            if narrow:
                self.facts["partial_fit_with_a_narrow_level"] += 1
            if hot:
                self.facts["partial_fit_on_the_hot_row"] += 1
        if code == OK and not self.dry:
            err, info = got
            ref = np.array([self.oracle.sgd_update(self.P[a], self.Q[b], float(c), float(self.lr), float(self.lam))
                            for a, b, c in zip(u, i, r)], np.float32)
            _same_bits(err, ref, "errors of partial_fit")
            assert (info["n"], info["pieces"], info["levels"], info["max_width"]) == (n, min(n, 1), n_levels, width), (info, n_levels, width)
            # the stored set, its identity (a later "again" is a reuse), its order and the cached graphs are as they were
            if self.R and check_order:
                self.getter()
                want_order = reference_order(self.mf, self.oracle, self.ref_cfg(), self.ratings, self.digest)
                assert np.array_equal(self.m.order()[0], want_order[0]), "partial_fit changed the canonical order"
        self.check_counts()
        return code

    # .. getters .......................................................................................................
    def getter(self):
        self.facts["schedule_getter_after_compute" if self.sched_computed else "schedule_getter_before_compute"] += 1

    def op_order(self, g):
        code, got = self.call(OK if self.R else STATE, lambda: self.m.order())
        if code == OK:
            self.getter()
            if not self.dry:
                want = reference_order(self.mf, self.oracle, self.ref_cfg(), self.ratings, self.digest)
                assert np.array_equal(got[0], want[0]), "the canonical order differs from a fresh handle's"
                assert np.array_equal(got[1], want[1]), "the cell boundaries differ from a fresh handle's"
        return code

    def op_debug_schedule(self, g):
        code, got = self.call(OK if self.R else STATE, lambda: self.m.debug_schedule())
        if code == OK:
            self.getter()
            if not self.dry:
                want = self.ref_schedule(self.lr, self.lam)["sched"]
                for name, x, y in zip(("cells", "rows", "subs", "entries"), got, want):
                    assert x.shape == y.shape and np.array_equal(x, y), \
                        f"{name} differ from a handle created at ({float(self.lr)!r}, {float(self.lam)!r})"
        return code

    def op_schedule_info(self, g):
        code, got = self.call(OK if self.R else STATE, lambda: self.m.schedule_info())
        if code == OK and not self.dry:
            got.pop("build_seconds")
            want = self.ref_schedule(self.lr, self.lam)["info"]
            assert got == want, (got, want)
        return code

    def op_debug_counters(self, g):
        """schedule builds, and the training graphs cached now: one per kept (P, Q) pair of addresses once an epoch has
        run, none under FLAG_NO_GRAPH; gone with a rebuilt schedule, other values of lr and lambda, factors seeded or
        replaced, and a reallocating append or reserve; kept by an append or a reserve inside the capacity and by
        partial_fit; back after the next epoch."""
        code, got = self.call(OK, lambda: self.m.debug_counters())
        if not self.dry:
            assert got["schedule_builds"] == self.builds, (got, self.builds)
            assert got["graphs"] == self.graphs, (got, self.graphs)
        return code


def run_sequence(mf, oracle, seed, n_ops, config, *, device=True, dry=False, wrong=None):
    """Creates one handle of `config` (dict: U, I, k, blocks, waves, flags, lr, lam, seed, profile), applies n_ops drawn ops
    and a final get_factors to it and to the model in lock step, asserting after each; closes it and checks that the
    library's device-byte count is back where it started.  Raises SequenceMismatch with every op so far.  Returns
    dict(counts {(kind, outcome): n}, facts {name: n}, n_ops, errors, seconds, log).
    device=False: no GPU is expected, and every call that needs one is MFSGD_ERR_NO_DEVICE.  dry=True: no library at all,
    the ops and their outcomes as the model alone gives them.  wrong: a deliberately wrong rule of the model
    ("hyper_before_ratings", "failed_set_ratings_keeps", "reseed_forgets_growth", "append_forgets_the_ratings",
    "set_factors_clears_the_index", "append_users_gives_new_users_the_last_list"), for the driver's self-test."""
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
    return dict(counts=run.counts, facts=run.facts, n_ops=n_ops + 1, errors=errors, seconds=time.perf_counter() - t0, log=run.log,
                dry=dry)


GROWTH_FACTS = ("fit_after_append_in_place", "fit_after_reallocating_append", "fit_after_partial_fit",
                "partial_fit_on_an_appended_row", "partial_fit_with_a_wide_level", "set_ratings_reuse_after_growth",
                "set_ratings_build_naming_appended_rows", "set_hyper_after_growth_then_fit", "init_factors_after_growth",
                "early_stopping_restored_after_growth", "validation_pair_on_an_appended_row", "stale_factor_file_refused",
                "append_on_a_device_packed_schedule_before_compute", "trained_on_a_swapped_schedule_after_growth")
NUMERIC_FACTS = ("early_stopping_restored_after_growth",)
SEEN_FACTS = ("seen_read_after_an_append_in_place", "seen_read_after_a_reallocating_append_on_the_device",
              "seen_read_after_a_reallocating_append_on_host_staging", "seen_read_after_reserve",
              "mark_seen_of_an_appended_user", "mark_seen_of_an_appended_item",
              "unseen_refused_for_no_seen_set_without_factors", "unseen_call_on_an_empty_index",
              "set_seen_replacing_a_non_empty_index", "refused_mark_seen_then_read", "mark_seen_wholly_inside_the_index",
              "partial_fit_seen_applied", "partial_fit_seen_refused")


def check_coverage(results):
    """The conditions of a set of sequences taken together (device present): returns the totals, raises on a miss."""
    results = list(results)
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
                 "trained_on_a_lone_tile_schedule", "schedule_getter_before_compute", "schedule_getter_after_compute") + GROWTH_FACTS + SEEN_FACTS:
        if fact in NUMERIC_FACTS and any(res.get("dry") for res in results):
            continue  # (whether an early stop restores depends on the numbers: a dry run has none)
        assert facts[fact] >= 1, f"{fact} never happened: {dict(facts)}"
    assert errors <= 0.35 * total, f"{errors} of {total} ops ended in an error code"
    return dict(ops=total, errors=errors, counts=counts, facts=facts)


# -- the cases of tests/test_handle_sequences_gpu.py (its dry run is a CPU test) --------------------------------------------
GEOMETRIES = {
    "k8": dict(k=8, U=600, I=90),                                    # L = 2: the C++ step; automatic blocks
    "k64_b16_w2": dict(k=64, blocks=16, waves=2, U=150 * 16, I=90),  # L = 16: solo runs, a lone-tile mailbox
    "k100_b12_w2": dict(k=100, blocks=12, waves=2, U=150 * 12, I=90),  # L = 32, padded
    # exchanged roles: the sets are drawn for (I, U) and u and i exchanged, user 9 rates every item, the chain and the
    # lone tile belong to a user, and the training kernels receive (Q, P) -- the two pointers that growth moves
    "k64_b12_w2_hot_user": dict(k=64, blocks=12, waves=2, U=90, I=150 * 12, swap_roles=True),
}
GPU_FLAGS = ("default", "FLAG_ROUND_LAUNCH", "FLAG_NO_GRAPH", "FLAG_DEVICE_INGEST", "FLAG_HOST_INGEST")
GPU_SEEDS = (0, 1)
GPU_OPS = 75  # (64 before the ops of the seen-item index: as many draws of every other kind as then, 64 x 132.7 / 113.2)


def flag_value(name):
    from mfsgd_amd import _lib

    return 0 if name == "default" else getattr(_lib, name)


def gpu_config(flag, geometry):
    return dict(GEOMETRIES[geometry], flags=flag_value(flag))


def gpu_seed(flag, geometry, seed):
    """Another sequence for every case."""
    return 1000 * GPU_FLAGS.index(flag) + 100 * sorted(GEOMETRIES).index(geometry) + seed
