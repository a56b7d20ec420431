"""mfsgd_set_hyper on the host path, without a GPU: a schedule re-baked in place is byte for byte the schedule a
fresh handle builds at the new values, for every record kind (general steps, run steps with idle slots, solo records,
chunked cells, swapped roles, DSGD partitions) and for the value pairs at which the old or the new decay factor is
exactly 1; replaying the re-baked arrays reproduces the oracle at the new values; the rating set's identity survives;
and the new calls check their arguments."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import have_gpu
from tests.kernel_emulator import replay_epoch

SEED = 3
# (from, to): ordinary; old c exactly 1; new c exactly 1; c rounds to 1; zero lr
PAIRS = [((0.01, 0.05), (0.007, 0.02)), ((0.01, 0.0), (0.02, 0.1)), ((0.01, 0.05), (0.01, 0.0)),
         ((0.01, 0.05), (1e-9, 0.05)), ((0.01, 0.05), (0.0, 0.05))]


def _dominant_item():
    """Item 7 rated by everyone plus 900 random pairs (tests/test_schedule_cpu.py's solo-run set)."""
    rng = np.random.default_rng(21)
    U, I = 400, 50
    u = list(range(U)) + list(rng.integers(0, U, 900))
    i = [7] * U + list(rng.integers(0, I, 900))
    key = np.unique(np.array(u) * I + np.array(i))
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(key.size) * 4 + 1).astype(np.float32)


def _dominant_item_with_nan_ratings():
    """_dominant_item with the NaN whose bits are all ones -- a solo record's empty mailbox word (csrc/run_asm.hpp) -- on
    every 40th rating of item 7 (solo steps) and every 97th rating of all: whoever writes a schedule writes the quiet
    NaN 0x7FC00000 for such a rating and for its lr * r (csrc/records.hpp, canon_nan)."""
    U, I, u, i, r = _dominant_item()
    r = r.copy()
    r[np.flatnonzero(i == 7)[::40]] = np.array([0xFFFFFFFF], np.uint32).view(np.float32)[0]
    r[::97] = np.array([0xFFFFFFFF], np.uint32).view(np.float32)[0]
    return U, I, u, i, r


def _chunked():
    rng = np.random.default_rng(257)
    U, I, n = 900, 800, 700
    key = rng.choice(U * I, n, replace=False)
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(n) * 4 + 1).astype(np.float32)


def _hot_user():
    rng = np.random.default_rng(10)
    U, I = 50, 300
    u = [7] * I + list(rng.integers(0, U, 600))
    i = list(range(I)) + list(rng.integers(0, I, 600))
    key = np.unique(np.array(u) * I + np.array(i))
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), rng.random(key.size).astype(np.float32)


# name -> (problem, k, constructor keywords, property of the schedule that makes the case what it is)
PROBLEMS = {
    "solo_k64_w2": (_dominant_item, 64, dict(blocks=2, waves=2), "solo"),
    "solo_k128_w4": (_dominant_item, 128, dict(blocks=2, waves=4), "solo"),
    "solo_k64_w1": (_dominant_item, 64, dict(blocks=2, waves=1), "solo"),
    "solo_nan_k64_w2": (_dominant_item_with_nan_ratings, 64, dict(blocks=2, waves=2), "solo_nan"),
    "run_k32_w2": (_dominant_item, 32, dict(blocks=2, waves=2), "run"),
    "chunked_k256": (_chunked, 256, dict(blocks=1, waves=2), "split"),
    "hot_user": (_hot_user, 64, dict(blocks=2, waves=2), "swapped"),
    "dsgd": (_dominant_item, 64, dict(blocks=2, waves=2, n_parts=2), "parts"),
}


def snapshot(m):
    """Everything of a handle's schedules that must not depend on how lr and lambda got there."""
    out = []
    for part in range(m.n_parts):
        info = m.schedule_info(part)
        info.pop("build_seconds")
        out.append((info, m.debug_schedule(part), m.order(part)))
    return out


def assert_same(a, b, what=""):
    assert len(a) == len(b)
    for part, ((ia, sa, oa), (ib, sb, ob)) in enumerate(zip(a, b)):
        assert ia == ib, (what, part)
        for name, x, y in zip(("cells", "rows", "subs", "entries"), sa, sb):
            assert x.shape == y.shape and np.array_equal(x, y), (what, part, name, np.flatnonzero((x != y).any(axis=-1))[:8])
        assert np.array_equal(oa[0], ob[0]) and np.array_equal(oa[1], ob[1]), (what, part, "order")


def check_kind(m, kind):
    """The schedule carries the records the case is there for."""
    for part in range(m.n_parts):
        info = m.schedule_info(part)
        cells, rows, subs, entries = m.debug_schedule(part)
        nsolo, nrun = int((subs[:, 0] >> 16).sum()), int((subs[:, 1] >> 16).sum())
        if kind == "solo":
            assert nsolo > 0, "solo steps must exist"
        if kind == "solo_nan":  # NaN ratings in solo records and in step entries, every one the quiet NaN in both words
            record = (entries[:, 1] == 0xFFFFFFFF) & (entries[:, 3] != 0)
            nan_record = record & ((entries[:, 3] & 0x7FFFFFFF) > 0x7F800000)
            nan_step = ~record & ((entries[:, 1] & 0x7FFFFFFF) > 0x7F800000) & (entries[:, 1] != 0xFFFFFFFF)
            assert nsolo > 0 and nan_record.sum() >= 5 and nan_step.sum() >= 5, (nan_record.sum(), nan_step.sum())
            assert (entries[nan_record][:, 2:] == 0x7FC00000).all() and (entries[nan_step][:, 1:3] == 0x7FC00000).all()
            assert not (entries[:, 2] == 0xFFFFFFFF).any()
        if kind == "run":
            assert nsolo == 0 and nrun > 0
            G = info["slots"]
            idle = 0
            for d in range(cells.shape[0]):
                for x in range(info["waves"] ** 2):
                    off, n = (int(v) for v in subs[d * info["waves"] ** 2 + x])
                    lo = (int(cells[d][1]) + (off & 0xFFFF) + (n & 0xFFFF)) * G
                    idle += int((entries[lo:lo + (n >> 16) * G, 0] >> 31).sum())
            assert idle > 0, "run steps with idle slots must exist"
        if kind == "split":
            assert info["split_cells"] >= 1
        if kind == "swapped":
            assert info["swapped"] == 1
        if kind == "parts":
            assert m.n_parts == 2 and info["nnz"] > 0


def fresh(mf, name, lr, lam, flags=0):
    make, k, kw, kind = PROBLEMS[name]
    U, I, u, i, r = make()
    m = mf.MatrixFactorizationSGD(U, I, k, lr, lam, SEED, flags=flags, **kw)
    m.set_ratings(u, i, r)
    return m


_fresh_cache = {}


def fresh_snapshot(mf, name, lr, lam):
    """What a handle created at (lr, lam) builds for the problem: computed once, never modified."""
    key = (name, lr, lam)
    if key not in _fresh_cache:
        with fresh(mf, name, lr, lam) as m:
            check_kind(m, PROBLEMS[name][3])
            _fresh_cache[key] = snapshot(m)
    return _fresh_cache[key]


@pytest.mark.parametrize("pair", range(len(PAIRS)))
@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_rebaked_schedule_is_the_fresh_schedule_byte_for_byte(mf, name, pair):
    (lr0, lam0), (lr1, lam1) = PAIRS[pair]
    first, want = fresh_snapshot(mf, name, lr0, lam0), fresh_snapshot(mf, name, lr1, lam1)
    with fresh(mf, name, lr0, lam0) as m:
        m.set_hyper(lr1, lam1)
        assert_same(snapshot(m), want, "after set_hyper")
        assert m.hyper() == (float(np.float32(lr1)), float(np.float32(lam1))) == (m.lr, m.lam)
        m.set_hyper(lr0, lam0)
        assert_same(snapshot(m), first, "after the round trip")


def test_threaded_host_pass_writes_the_same_bytes(mf):
    """A schedule large enough for rehyper_schedule to deal its chunks out to several threads."""
    w = mf.synth.workload("cfg1_ml100k", 1.0)
    (lr0, lam0), (lr1, lam1) = PAIRS[0]
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], lr1, lam1, SEED, host_threads=4) as f, \
            mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], lr0, lam0, SEED, host_threads=4) as m:
        for x in (f, m):
            x.set_ratings(w["u"], w["i"], w["r"])
        assert m.debug_schedule()[3].shape[0] >= 1 << 16, "too small for the threaded pass"
        m.set_hyper(lr1, lam1)
        assert_same(snapshot(m), snapshot(f))


def test_replaying_the_rebaked_schedule_gives_the_oracle_at_the_new_values(mf, oracle):
    make, k, kw, _ = PROBLEMS["solo_k64_w2"]
    U, I, u, i, r = make()
    lr1, lam1 = 0.007, 0.02
    with fresh(mf, "solo_k64_w2", 0.01, 0.05) as m:
        m.set_hyper(lr1, lam1)
        info, sched, (order, _) = m.schedule_info(), m.debug_schedule(), m.order()
    assert not info["swapped"]
    P, Q = oracle.init_factors(U, I, k, SEED)
    Pe, Qe = P.copy(), Q.copy()
    oracle.sgd_pass_ordered(P, Q, u, i, r, order, lr1, lam1)
    replay_epoch(oracle, Pe, Qe, k, lr1, lam1, sched, info["blocks"], info["waves"], info["slots"], info["group_lanes"])
    np.testing.assert_array_equal(Pe, P)
    np.testing.assert_array_equal(Qe, Q)


def test_the_rating_set_stays_recognised_and_a_rebuild_uses_the_new_values(mf):
    make, k, kw, _ = PROBLEMS["solo_k64_w2"]
    U, I, u, i, r = make()
    lr1, lam1 = 0.007, 0.02
    with fresh(mf, "solo_k64_w2", 0.01, 0.05) as m:
        assert m.debug_counters()["schedule_builds"] == 1
        m.set_hyper(lr1, lam1)
        assert m.debug_counters()["schedule_builds"] == 1
        m.set_ratings(u.copy(), i.copy(), r.copy())  # the same triples: kept, and still holding the new values
        assert m.debug_counters()["schedule_builds"] == 1
        assert_same(snapshot(m), fresh_snapshot(mf, "solo_k64_w2", lr1, lam1), "same triples")
        r2 = r.copy()
        r2[5] += 1.0
        m.set_ratings(u, i, r2)  # other triples: built, with the new values
        assert m.debug_counters()["schedule_builds"] == 2
        with mf.MatrixFactorizationSGD(U, I, k, lr1, lam1, SEED, **kw) as f:
            f.set_ratings(u, i, r2)
            assert_same(snapshot(m), snapshot(f), "other triples")


def test_set_hyper_before_any_ratings_only_changes_the_configuration(mf):
    with mf.MatrixFactorizationSGD(400, 50, 64, 0.01, 0.05, SEED, blocks=2, waves=2) as m:
        assert m.hyper() == (float(np.float32(0.01)), float(np.float32(0.05)))
        m.set_hyper(0.007, 0.02)
        assert m.hyper() == (float(np.float32(0.007)), float(np.float32(0.02)))
        lib, h = m._lib, m._handle()
        lr = C.c_float()
        assert lib.mfsgd_get_hyper(h, C.byref(lr), None) == 0 and lr.value == float(np.float32(0.007))  # either may be NULL
        assert lib.mfsgd_get_hyper(h, None, None) == 0
        U, I, u, i, r = _dominant_item()
        m.set_ratings(u, i, r)
        assert_same(snapshot(m), fresh_snapshot(mf, "solo_k64_w2", 0.007, 0.02))


def test_argument_checks(mf):
    nan = float("nan")
    f32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_double)
    with fresh(mf, "solo_k64_w2", 0.01, 0.05) as m:
        m.init_factors()
        lib, h = m._lib, m._handle()
        before = snapshot(m)

        def bad(rc, prefix):
            assert rc == -1, rc  # MFSGD_ERR_INVALID_ARG
            assert lib.mfsgd_last_error(h).decode().startswith(prefix), lib.mfsgd_last_error(h)

        bad(lib.mfsgd_set_hyper(h, nan, 0.05), "set_hyper: ")
        bad(lib.mfsgd_set_hyper(h, 0.01, nan), "set_hyper: ")
        lrs = (C.c_float * 3)(0.01, 0.02, 0.03)
        lams = (C.c_float * 3)(0.05, 0.05, 0.05)
        out = (C.c_double * 3)()
        used = (C.c_float * 3)()
        bad(lib.mfsgd_train_schedule(h, -1, lrs, None, None), "train_schedule: ")
        bad(lib.mfsgd_train_schedule(h, 3, None, None, None), "train_schedule: ")
        bad(lib.mfsgd_train_schedule(h, 3, (C.c_float * 3)(0.01, 0.02, nan), None, out), "train_schedule: ")
        bad(lib.mfsgd_train_schedule(h, 3, lrs, (C.c_float * 3)(0.05, nan, 0.05), out), "train_schedule: ")
        bad(lib.mfsgd_train_bold_driver(h, -1, 1.05, 0.5, used, out), "bold_driver: ")
        bad(lib.mfsgd_train_bold_driver(h, 3, 1.05, 0.5, None, out), "bold_driver: ")
        bad(lib.mfsgd_train_bold_driver(h, 3, 1.05, 0.5, used, None), "bold_driver: ")
        for up, down in ((nan, 0.5), (1.05, nan), (0.0, 0.5), (1.05, 0.0), (-1.0, 0.5), (1.05, -0.5)):
            bad(lib.mfsgd_train_bold_driver(h, 3, up, down, used, out), "bold_driver: ")
        # epochs == 0 is fine, with or without a device, and needs no arrays
        assert lib.mfsgd_train_schedule(h, 0, None, None, None) == 0
        assert lib.mfsgd_train_bold_driver(h, 0, 1.05, 0.5, None, None) == 0
        # none of the refused calls changed anything
        assert m.hyper() == (float(np.float32(0.01)), float(np.float32(0.05)))
        assert_same(snapshot(m), before)
        # a valid call computes on the device or fails loudly: there is no CPU training
        rc_s = lib.mfsgd_train_schedule(h, 3, lrs, lams, out)
        rc_b = lib.mfsgd_train_bold_driver(h, 3, 1.05, 0.5, used, out)
        if have_gpu():
            assert (rc_s, rc_b) == (0, 0)
        else:
            assert (rc_s, rc_b) == (-2, -2)  # MFSGD_ERR_NO_DEVICE
            assert m.hyper() == (float(np.float32(0.01)), float(np.float32(0.05)))
    with fresh(mf, "dsgd", 0.01, 0.05) as m:  # as mfsgd_train: partitioned handles are driven with mfsgd_part_train
        m.init_factors()
        assert m._lib.mfsgd_train_schedule(m._handle(), 3, lrs, None, None) == -5
        assert m._lib.mfsgd_train_bold_driver(m._handle(), 3, 1.05, 0.5, used, out) == -5
    with mf.MatrixFactorizationSGD(4, 3, 8, 0.01, 0.05, 1) as m:  # ... and nothing trains before set_ratings
        assert m._lib.mfsgd_train_schedule(m._handle(), 3, lrs, None, None) == -5
