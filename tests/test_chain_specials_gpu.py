"""NaN and Inf through the loops the epoch waits for: the solo chain wave, its helper wave and the lone-tile hop, and with
them every other loop form of the epoch kernel, mfsgd_apply_ratings and fold-in.

A solo record's mailbox word is 0xFFFFFFFF until the chain wave has posted s there; 0xFFFFFFFF is also a NaN, and
s = fma(-lr, dot, lr * r) hands a NaN operand's payload on.  So the library replaces every NaN that enters it by the quiet
NaN 0x7FC00000 (csrc/records.hpp, canon_nan): an all-ones NaN in a rating, in P or in Q ends in NaN exactly where the
oracle has NaN, and the call returns MFSGD_OK -- not in the helper giving up after 2^22 polls ("timed out waiting for a
tile hand-off").  Without canon_nan in the packers a NaN rating of a solo step posts all ones (the rating cases), without
it in set_factors a NaN row does (the P and Q cases); FLAG_ROUND_LAUNCH runs the one-wave form, which has no mailbox.

The reference is the oracle replaying the order the handle exports, compared after EACH epoch: which entries are NaN, and
every bit of the others (infinities included); the RMSE finite on both sides or on neither.  What keeps the comparisons
from being vacuous is asserted on the oracle's results only, and without a GPU in tests/test_contract_edges_cpu.py."""
import numpy as np
import pytest

from tests import edge_inputs as E

pytestmark = pytest.mark.gpu

EPOCHS = 2


def _flag_sets():
    from mfsgd_amd import _lib

    return (("default", 0), ("no_graph", _lib.FLAG_NO_GRAPH), ("round_launch", _lib.FLAG_ROUND_LAUNCH))


def _epoch_by_epoch(mf, U, I, k, u, i, r, P0, Q0, flags, kw, seed=11):
    """[(P, Q, rmse) after each epoch], order, schedule_info, debug_schedule; P0 None: factors from the seed."""
    with mf.MatrixFactorizationSGD(U, I, k, E.LR, E.LAM, seed, flags=flags, **kw) as m:
        m.set_ratings(u, i, r)
        if P0 is None:
            m.init_factors()
        else:
            m.set_factors(P0, Q0)
        got = []
        for _ in range(EPOCHS):
            rm = m.fit(1)  # (an error -- the helper's give-up is one -- raises here)
            got.append(m.get_factors() + (float(rm[0]),))
        return got, m.order()[0], m.schedule_info(), m.debug_schedule()


def _oracle_epochs(oracle, P0, Q0, u, i, r, order):
    P, Q = P0.copy(), Q0.copy()
    out = []
    for _ in range(EPOCHS):
        oracle.sgd_pass_ordered(P, Q, u, i, r, order, E.LR, E.LAM)
        out.append((P.copy(), Q.copy(), oracle.rmse(P, Q, u, i, r)))
    return out


def _compare(got, want, what):
    for epoch, ((P, Q, rm), (Po, Qo, rmo)) in enumerate(zip(got, want)):
        print(f"{what}, epoch {epoch + 1}: NaN P {np.isnan(Po).mean():.4f} Q {np.isnan(Qo).mean():.4f}; inf P "
              f"{np.isinf(Po).mean():.4f} Q {np.isinf(Qo).mean():.4f}; rmse {rm} oracle {rmo}")
        E.assert_same_but_for_the_nans(f"{what}: P after epoch {epoch + 1}", P, Po)
        E.assert_same_but_for_the_nans(f"{what}: Q after epoch {epoch + 1}", Q, Qo)
        E.assert_rmse_same_but_for_the_nans(rm, rmo)


def _solo_and_lone(sched):
    return int(((sched[2][:, 0] >> 16) > 0).sum()), int((sched[0][:, 5] & 1).sum())


def _through_every_path(mf, oracle, U, I, k, u, i, r, P0, Q0, kw, what, check, solo_runs, lone_cells):
    """The three launch paths on one problem; the oracle once per exported order; `check`: the oracle-side conditions."""
    seen = {}
    for name, flags in _flag_sets():
        got, order, info, sched = _epoch_by_epoch(mf, U, I, k, u, i, r, P0, Q0, flags, kw)
        assert _solo_and_lone(sched) == (solo_runs, lone_cells), (name, _solo_and_lone(sched))
        if order.tobytes() not in seen:
            if P0 is None:
                P0, Q0 = oracle.init_factors(U, I, k, 11)
            seen[order.tobytes()] = _oracle_epochs(oracle, P0, Q0, u, i, r, order)
            check(seen[order.tobytes()])
        _compare(got, seen[order.tobytes()], f"{what} {name}")


# ---- A: the all-ones NaN ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", E.NAN_PLACES)
@pytest.mark.parametrize("k,W", E.SOLO_KW)
def test_an_all_ones_nan_passes_through_a_solo_run(mf, oracle, k, W, where):
    """hot_item_set: all ratings of item 7 lie in solo runs of 300 / 150 / 125 steps (10 / 20 / 24 runs; at k = 256 every
    one a lone-tile cell of the fast lane).  One all-ones NaN per case, late in the order (E.place_nan)."""
    U, I, u, i, kw = E.odd_run_set(mf, k, W) if where == "rating_last_step_of_an_odd_run" else E.hot_item_set(k, W)
    P0, Q0 = E.ordinary_factors(U, I, k)
    P0, Q0, r, n, step = E.place_nan(where, mf, k, U, I, u, i, kw, P0, Q0, E.ordinary_ratings(u.size))
    assert (E.bits(P0) == 0xFFFFFFFF).sum() + (E.bits(Q0) == 0xFFFFFFFF).sum() + (E.bits(r) == 0xFFFFFFFF).sum() == 1
    if where == "rating_last_step_of_an_odd_run":
        assert n % 2 == 1 and step == n - 1
    runs, _ = E.solo_runs(mf, U, I, k, u, i, **kw)
    assert sum(x.size for x in runs if i[x[0]] == E.HOT_ITEM) == (i == E.HOT_ITEM).sum()  # item 7 is in solo runs only
    _through_every_path(mf, oracle, U, I, k, u, i, r, P0, Q0, kw, f"k={k} {where} (run of {n}, step {step})",
                        lambda states: E.check_nan_case(where, states), len(runs), E.LONE_CELLS[k])


@pytest.mark.parametrize("where", [w for w in E.NAN_PLACES if w != "rating_last_step_of_an_odd_run"])
def test_an_all_ones_nan_crosses_the_fast_lane(mf, oracle, where):
    """Item 9 of the lone-tile problem at B = 12, k = 64: twelve runs of 150 steps (none odd), each a lone-tile cell, so
    the NaN row travels through the mailbox granules {value, tag} from workgroup to workgroup."""
    U, I, k, u, i, r0, kw = E.lone_problem()
    P0, Q0 = E.ordinary_factors(U, I, k)
    P0, Q0, r, n, step = E.place_nan(where, mf, k, U, I, u, i, kw, P0, Q0, r0, item=E.LONE_ITEM)
    runs, _ = E.solo_runs(mf, U, I, k, u, i, **kw)
    assert n == 150 and sum(x.size == 150 and i[x[0]] == E.LONE_ITEM for x in runs) == 12
    _through_every_path(mf, oracle, U, I, k, u, i, r, P0, Q0, kw, f"lone {where} (step {step})",
                        lambda states: E.check_nan_case(where, states), len(runs), E.LONE_PROBLEM_CELLS)


# ---- B: overflow through every loop form -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,where", E.overflow_cases())
def test_overflow_through_every_loop_form(mf, oracle, name, where):
    """1 % of the ratings at +-3e38 (test_contract_edges_gpu's overflow test, which runs the general steps only) on the
    sets that make the kernel take its other loop forms: run loops and solo pairs (hot_item), the fast lane (lone),
    chunked cells, swapped roles -- anywhere, at the end of the exported order and, with a hot item, on its last 20
    ratings in the order: the helper's re-derived q recurrence and the granules of a lone tile carry Inf and NaN.

    [swapped_k64-last_in_the_order] is the case that found the idle slot of a run step left to the arithmetic: with a
    resident row that held an Inf, 0 * Inf = NaN turned the row NaN and went into the zero row that the idle slots of
    every wave share (one user row NaN against the oracle's finite 2.5e36, depending on which wave read it first).  The run
    loops now mask idle slots (csrc/run_asm.hpp, Cell::apply run_step)."""
    make, k, hot = E.OVERFLOW_SETS[name]
    U, I, u, i, kw = make()
    with mf.MatrixFactorizationSGD(U, I, k, E.LR, E.LAM, 11, **kw) as m:
        m.set_ratings(u, i, np.ones(u.size, np.float32))
        order = m.order()[0]
    r = E.overflow_ratings(where, u, i, order, hot)
    seen = {}
    for path, flags in _flag_sets()[::2] if name.startswith(("chunked", "swapped")) else _flag_sets():
        got, order2, info, sched = _epoch_by_epoch(mf, U, I, k, u, i, r, None, None, flags, kw)
        assert np.array_equal(order2, order)  # (the order depends on (u, i) only)
        E.check_overflow_set(name, info, sched)
        if not seen:
            P0, Q0 = oracle.init_factors(U, I, k, 11)
            seen[0] = _oracle_epochs(oracle, P0, Q0, u, i, r, order)
            E.check_overflow_case(where, seen[0])
        _compare(got, seen[0], f"{name} {where} {path}")


# ---- B: apply_ratings and fold-in ------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,kind,k", E.ONLINE_SPECIALS)
def test_partial_fit_propagates_nan_and_overflow(mf, oracle, batch, kind, k):
    """include/mfsgd.h, mfsgd_apply_ratings: "a NaN or Inf rating propagates".  P, Q and the returned errors against the
    oracle's sequential loop: the same entries NaN, every other bit equal."""
    from tests.test_online_gpu import LAM, LR, SEED, _oracle_apply

    U, I, u, i, r, at = E.online_special_batch(batch, kind)
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    P, Q, err = _oracle_apply(oracle, P0, Q0, u, i, r)
    E.check_online_special(kind, at, err, P, Q)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.init_factors()
        got_err = m.partial_fit(u, i, r, errors=True)
        gP, gQ = m.get_factors()
    print(f"{batch} {kind} k={k}: NaN errors {np.isnan(err).mean():.3f}, NaN P {np.isnan(P).mean():.3f} Q {np.isnan(Q).mean():.3f}")
    E.assert_same_but_for_the_nans("P", gP, P)
    E.assert_same_but_for_the_nans("Q", gQ, Q)
    E.assert_same_but_for_the_nans("errors", got_err, err)


@pytest.mark.parametrize("k", E.FOLD_IN_K)
def test_fold_in_propagates_nan_and_overflow(mf, oracle, k):
    from tests.test_fold_in_gpu import fold_in_ref

    Q, row_ptr, items, ratings, init = E.fold_in_specials(k)
    want = fold_in_ref(oracle, Q, row_ptr, items, ratings, 3, init, E.LR, E.LAM)
    E.check_fold_in_specials(want)
    with mf.MatrixFactorizationSGD(6, Q.shape[0], k, E.LR, E.LAM, 1) as m:
        m.set_factors(np.zeros((6, k), np.float32), Q)
        got = m.fold_in(row_ptr, items, ratings, 3, init=init)
    E.assert_same_but_for_the_nans("fold-in rows", got, want)


# ---- D: hot rows on the user side, and on both sides, at explicit geometry --------------------------------------------
def _forms(mf, U, I, k, u, i, **kw):
    """(swapped, lone-tile cells, lengths of the solo runs in ascending order, run steps) of the schedule a handle builds."""
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 5, **kw) as m:
        m.set_ratings(u, i, np.ones(u.size, np.float32))
        cells, _, subs, _ = m.debug_schedule()
        solo = subs[:, 0] >> 16
        return (m.schedule_info()["swapped"], int((cells[:, 5] & 1).sum()), sorted(int(x) for x in solo[solo > 0]),
                int((subs[:, 1] >> 16).sum()))


@pytest.mark.parametrize("k,B", [(64, 8), (256, 12)])
def test_hot_user_with_a_tile_of_its_own(mf, oracle, k, B):
    """Swapped roles through the fast lane: the chain is a user's, its row hops from workgroup to workgroup."""
    from tests.test_gpu_parity import _run

    U, I, u, i, r = E.hot_user_lone_set(B)
    swapped, lone, solo, _ = _forms(mf, U, I, k, u, i, blocks=B, waves=2)
    print(f"k={k} B={B}: swapped {swapped}, lone cells {lone}, solo runs {solo}")
    assert (swapped, lone, len(solo)) == (1, 2 * B, 2 * B) and solo.count(150) == B  # user 9: 150 items per cell
    _run(mf, oracle, U, I, k, u, i, r, seed=5, epochs=3, blocks=B, waves=2)


@pytest.mark.parametrize("U,I", [(1200, 600), (600, 1200)])
def test_hot_rows_on_both_sides(mf, oracle, U, I):
    from tests.test_gpu_parity import _run

    U, I, u, i, r = E.two_sided_set(U, I)
    swapped, lone, solo, run_steps = _forms(mf, U, I, 64, u, i, blocks=8, waves=2)
    print(f"U={U} I={I}: swapped {swapped}, lone cells {lone}, solo runs {solo}, run steps {run_steps}")
    # the longer side's hot row: every one of its 1200 ratings in ONE solo run per block -- 160 where a block holds 160
    # rows of that side, 159 and 81 in the two blocks that hold the hot rows of the other side's weight (rows are dealt to
    # blocks by their degrees).  The shorter side's hot row is a chain of general steps: no run step exists.
    assert (swapped, lone, solo, run_steps) == (int(U < I), 8, [81, 159] + [160] * 6, 0)
    _run(mf, oracle, U, I, 64, u, i, r, seed=5, epochs=3, blocks=8, waves=2)
