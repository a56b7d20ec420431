"""The fp32 edges through the scaling c * q of a SOLO run's chain wave (csrc/run_asm.hpp, MFSGD_SOLO_CHAIN_HALF: the two
packed multiplies that sit in the wait states of the DPP adds, next to the step's LDS reads).  A flushed, mis-rounded or
sign-dropping product there would show in the hot item's row and nowhere else, so the hot item's row itself is put on the
edge: non-zero subnormals that stay subnormal through the epochs (q_subnormal; tiny_products with its Q scaled by 2^-64,
where q' = fma(s, p, c * q) IS c * q rounded in the subnormal range: s * p underflows), signed zeros that stay zeros of
both signs (every rating is -0.0, so the row's signs are what c * -0.0 and the fma make of them), and NaN and +-Inf
through the chain of a lone tile.

The problems are tests/test_solo_chain_steady_gpu.py's (B = 16, W = 2, fewer than 5000 ratings): solo runs of 12..27 steps
at k = 64 / 128, 38..51 at k = 256 -- the tail alone, the steady body and every hand-over -- and the item with a tile of
its own at k = 64 (55..70 steps, 16 lone-tile cells).  Persistent and round-launch paths, 2 epochs, factors bit for bit
(tobytes) against the oracle replaying the exported order from the factors the test sets.  (tests.test_gpu_parity._run
draws the factors from the seed and cannot start from a family's, so the handle is driven here the way
tests/test_contract_edges_gpu.py drives it; the comparison is _run's, with -0.0 told from +0.0.)

What keeps a case from being vacuous is asserted on the oracle's states only (check_edge)."""
import functools

import numpy as np
import pytest

from tests import edge_inputs as E
from tests.test_solo_chain_steady_gpu import PROBLEM_A, PROBLEM_C, PROBLEM_LONE
from tests.test_solo_chain_unrolled_gpu import _hot_item_problem

pytestmark = pytest.mark.gpu

EPOCHS = 2
HOT = 0  # _hot_item_problem's hot item
FAMILY_Q_SCALE = {"q_subnormal": 1.0, "tiny_products": 2.0 ** -64, "signed_zero": 1.0}
PROBLEMS = {"A": PROBLEM_A, "C": PROBLEM_C}
SOLO_LENGTHS = {64: range(12, 28), 128: range(12, 28), 256: range(12, 52)}


@functools.lru_cache(maxsize=None)
def _problem(args):
    return _hot_item_problem(*args)


def edge_inputs(fam, U, I, k, u, i):
    """(P0, Q0, r) of the family over a hot-item problem, the hot item's row on the edge (module docstring)."""
    P0, Q0, r = E.family(fam, U, I, k, u.size)
    Q0 = (Q0 * np.float32(FAMILY_Q_SCALE[fam])).astype(np.float32)  # a power of two
    if fam == "signed_zero":
        # Every rating is -0.0, every item row zeros, every user row positive: s = fma(-lr, +0.0, lr * -0.0) = -0.0 at
        # every step of the hot item (a dot of zeros of both signs is +0.0), q' = fma(-0.0, p, c * q) keeps the sign of
        # each q where c * -0.0 is -0.0, and p' = fma(s, q, c * p) stays positive: the row's pattern of signs survives
        # the epochs.  (With ordinary ratings beside them the users' entries change sign and the row ends as +0.0 throughout.)
        P0 = np.abs(P0) + np.float32(0.01)
        Q0[2::3] = np.float32(0.0)
        Q0[HOT, 0::2] = np.float32(-0.0)
        Q0[HOT, 1::2] = np.float32(0.0)
        r = np.full(u.size, -0.0, np.float32)
    return P0, Q0, r


def oracle_states(oracle, P0, Q0, u, i, r, order):
    """[(P, Q, rmse)] after each epoch of the oracle replaying `order` from (P0, Q0)."""
    P, Q = P0.copy(), Q0.copy()
    out = []
    for _ in range(EPOCHS):
        oracle.sgd_pass_ordered(P, Q, u, i, r, order, E.LR, E.LAM)
        out.append((P.copy(), Q.copy(), oracle.rmse(P, Q, u, i, r)))
    return out


def check_edge(fam, Q0, states, i):
    """On the oracle's side: the hot item's row is on its edge before the first epoch and after each one, and it moved."""
    assert (i == HOT).sum() >= 400
    rows = [Q0[HOT]] + [Q[HOT] for _, Q, _ in states]
    if fam == "signed_zero":
        for row in rows:
            assert (row == 0).all()
        for row in rows:  # zeros of both signs, before and after: at least a quarter of the row each
            assert (E.bits(row) == 0x80000000).mean() >= 0.25 and (E.bits(row) == 0).mean() >= 0.25
        assert any((E.bits(Q[1:]) != E.bits(Q0[1:])).any() for _, Q, _ in states)  # (other rows do change their signs)
    else:
        for row in rows:
            assert E.is_subnormal(row).all(), (fam, row)
        for before, after in zip(rows, rows[1:]):
            assert (E.bits(before) != E.bits(after)).all()
    for P, Q, _ in states:
        assert np.isfinite(P).all() and np.isfinite(Q).all()


def _fit(mf, U, I, k, u, i, r, P0, Q0, flags):
    """[(P, Q, rmse) after each epoch], order, debug_schedule."""
    with mf.MatrixFactorizationSGD(U, I, k, E.LR, E.LAM, 11, blocks=16, waves=2, flags=flags) as m:
        m.set_ratings(u, i, r)
        m.set_factors(P0, Q0)
        got = []
        for _ in range(EPOCHS):
            rm = m.fit(1)
            got.append(m.get_factors() + (float(rm[0]),))
        return got, m.order()[0], m.debug_schedule()


def _both_paths(mf, oracle, U, I, k, u, i, r, P0, Q0, what, check, compare):
    """Persistent and round-launch; the oracle once per exported order.  Returns the schedules."""
    from mfsgd_amd import _lib

    assert E.host_keeps_subnormals()
    seen, scheds = {}, []
    for name, flags in (("persistent", 0), ("round_launch", _lib.FLAG_ROUND_LAUNCH)):
        got, order, sched = _fit(mf, U, I, k, u, i, r, P0, Q0, flags)
        if order.tobytes() not in seen:
            seen[order.tobytes()] = oracle_states(oracle, P0, Q0, u, i, r, order)
            check(seen[order.tobytes()])
        for epoch, (g, w) in enumerate(zip(got, seen[order.tobytes()])):
            compare(f"{what} {name} epoch {epoch + 1}", g, w)
        scheds.append(sched)
    return scheds


def _bit_for_bit(what, got, want):
    for name, g, w in (("P", got[0], want[0]), ("Q", got[1], want[1])):
        assert g.tobytes() == w.tobytes(), f"{what}: {name} differs in {(E.bits(g) != E.bits(w)).mean():.4f} of its entries"
    np.testing.assert_allclose(got[2], want[2], rtol=1e-9, atol=0)


def _solo_lengths(sched):
    n = sched[2][:, 0] >> 16
    return [int(x) for x in n[n > 0]]


@pytest.mark.parametrize("problem", sorted(PROBLEMS))
@pytest.mark.parametrize("fam", sorted(FAMILY_Q_SCALE))
@pytest.mark.parametrize("k", [64, 128, 256])  # L = 16, 32, 64
def test_scaled_row_on_the_edge_through_solo_runs(mf, oracle, k, fam, problem):
    U, I, u, i, _ = _problem(PROBLEMS[problem])
    assert u.size < 5000
    P0, Q0, r = edge_inputs(fam, U, I, k, u, i)
    scheds = _both_paths(mf, oracle, U, I, k, u, i, r, P0, Q0, f"k={k} {fam} {problem}",
                         lambda states: check_edge(fam, Q0, states, i), _bit_for_bit)
    lengths = _solo_lengths(scheds[0])
    print(f"k={k} {fam} {problem}: solo run lengths {sorted(set(lengths))}")
    assert len(lengths) >= 16 and sum(lengths) >= 400 and set(lengths) <= set(SOLO_LENGTHS[k]), sorted(set(lengths))


@pytest.mark.parametrize("fam", sorted(FAMILY_Q_SCALE))
def test_scaled_row_on_the_edge_through_the_lone_tile_chain(mf, oracle, fam):
    U, I, u, i, _ = _problem(PROBLEM_LONE)
    assert u.size < 5000
    P0, Q0, r = edge_inputs(fam, U, I, 64, u, i)
    scheds = _both_paths(mf, oracle, U, I, 64, u, i, r, P0, Q0, f"lone {fam}", lambda states: check_edge(fam, Q0, states, i),
                         _bit_for_bit)
    lengths = _solo_lengths(scheds[0])
    assert int((scheds[0][0][:, 5] & 1).sum()) == 16  # kCellLoneTile
    assert set(lengths) <= set(range(55, 71)) and {n % 8 for n in lengths} == set(range(8)), sorted(set(lengths))


def test_nan_and_inf_in_the_row_through_the_lone_tile_chain(mf, oracle):
    """NaN, +Inf and -Inf in the hot item's row at the start: c * q hands each on as IEEE does, the first dot is NaN and
    the row and every user that rated the item turn NaN where the oracle's do; the entries that stay finite are equal."""
    U, I, u, i, r = _problem(PROBLEM_LONE)
    P0, Q0 = E.ordinary_factors(U, I, 64)
    Q0[HOT, 1::7] = np.float32(np.nan)
    Q0[HOT, 2::7] = np.float32(np.inf)
    Q0[HOT, 3::7] = np.float32(-np.inf)

    def check(states):
        P, Q, rm = states[0]
        raters = np.unique(u[i == HOT])
        assert np.isnan(Q[HOT]).all() and np.isnan(P[raters]).all() and np.isnan(rm)
        # (their other ratings carry the NaN on to items and from there to users that never rated the hot item: half of
        # the users rated it, and some rows are still finite after the first epoch)
        assert np.isfinite(P).all(axis=1).sum() >= 100 and 0.25 <= E.nan_share(P, Q) <= 0.95
        assert E.nan_share(*states[-1][:2]) >= E.nan_share(P, Q)

    def compare(what, got, want):
        E.assert_same_but_for_the_nans(f"{what}: P", got[0], want[0])
        E.assert_same_but_for_the_nans(f"{what}: Q", got[1], want[1])
        E.assert_rmse_same_but_for_the_nans(got[2], want[2])

    scheds = _both_paths(mf, oracle, U, I, 64, u, i, r, P0, Q0, "lone NaN and Inf", check, compare)
    assert int((scheds[0][0][:, 5] & 1).sum()) == 16  # kCellLoneTile
