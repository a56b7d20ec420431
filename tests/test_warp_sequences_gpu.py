"""The two WARP calls inside the life of one handle: sample_unseen_violating and partial_fit_pairwise(weights=) drawn
between set_ratings, fit, set_hyper, set_seen / mark_seen / clear_seen, add_users / add_items and the factor calls, on a
handle and on the model of tests/handle_model.py in lock step.  handle_model.py is imported as it is: the runner below adds
the two ops to its Runner and draws from a subset of its kinds.  The model answers the pick with the restated rule
(tests/warp_common.py) over its own index, counts and factors, and the weighted step with the restated sequential loop;
every later op, the final get_factors included, is answered for the factors those steps left.  The draws depend on the
seed and the model's abstract state alone, so what a sequence reaches is checked in a dry run, without a GPU."""
import tempfile

import numpy as np
import pytest

from tests import handle_model as hm
from tests import warp_common as WC

OK, NO_DEVICE, STATE = hm.OK, hm.NO_DEVICE, hm.STATE
KINDS = dict(set_ratings=0.5, init_factors=1, set_factors=0.5, fit=0.6, set_hyper=0.5, set_seen=1.5, mark_seen=1, clear_seen=0.15,
             add_users=0.7, add_items=1, get_factors=1, seen_size=0.5)  # x handle_model's weight
NEW = dict(sample_violating=9, fit_weighted=9)
GEOMETRIES = ("k8", "k64_b16_w2")
N_OPS = 60


class WarpRunner(hm.Runner):
    def weights(self):
        base = super().weights()
        w = {kind: base[kind] * scale for kind, scale in KINDS.items()}
        w.update(NEW)
        return w

    def lists(self):
        keys = self.seen
        return lambda u: (keys[np.searchsorted(keys, u << 32):np.searchsorted(keys, (u + 1) << 32)] & 0xFFFFFFFF)

    def op_sample_violating(self, g):
        """0 .. 200 rows over the current counts, appended rows among them; m on both sides of a round of L lanes."""
        none = int(g.integers(8)) == 0
        n = 0 if none else int(g.integers(1, 201))
        users, pos = g.integers(0, self.U, n).astype(np.int32), g.integers(0, self.I, n).astype(np.int32)
        L = self.group_lanes
        m = int(g.choice([1, 3, L, L + 1, 2 * L + 3]))
        margin = float(g.choice([0.0, 0.02, 0.2, np.inf]))
        seed, first = int(g.integers(1 << 30)), int(g.integers(1 << 40))
        self.note(f"[n={n}, m={m}, margin={margin}, index={'none' if self.seen is None else self.seen.size}]")
        if self.seen is None or self.F != "full":
            want = STATE
        else:
            want = OK if self.device or n == 0 else NO_DEVICE
        code, got = self.call(want, lambda: self.m.sample_unseen_violating(users, pos, m, margin, seed, first, draws=True,
                                                                          margins=True, ranks=True))
        if code == OK and n > 0:
            self.uploaded()
            for what in ("mark_seen", "add_items", "add_users", "set_hyper", "fit", "fit_weighted"):
                if what in self.since:
                    self.facts["violating_after_" + what] += 1
            self.since.clear()
        if code == OK and not self.dry:
            ref = WC.violating(self.lists(), self.I, users, pos, m, margin, seed, first,
                               lambda u, i: self.oracle.predict(self.P, self.Q, u, i))
            for a, b, name in zip(got, ref, ("items", "draws", "margins", "ranks")):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{name} of sample_unseen_violating differ from the model's"
            if n and (got[0] >= 0).any():
                self.facts["violating_found_a_pick"] += 1
            if n and (got[1] == m).any():
                self.facts["violating_found_none"] += 1
        self.check_seen_lists()  # the index is as it was
        self.check_counts()
        return code

    def op_fit_weighted(self, g):
        """0 .. 200 weighted triples over the current counts: a hot user and a hot item (many levels), appended rows, and
        weights that are WARP's for drawn ranks, negative, or zero."""
        none = int(g.integers(8)) == 0
        n = 0 if none else int(g.integers(1, 201))
        u, i = g.integers(0, self.U, n).astype(np.int32), g.integers(0, self.I, n).astype(np.int32)
        if n:
            u[g.integers(0, n, n // 5 + 1)] = 2
            i[g.integers(0, n, n // 5 + 1)] = hm.HOT
        j = ((i + g.integers(1, self.I, n)) % self.I).astype(np.int32)
        w = self.mf.warp_weights(g.integers(0, self.I, n)) if not self.dry else np.zeros(n, np.float32)
        w = np.where(g.integers(0, 4, n) == 0, g.standard_normal(n).astype(np.float32), w).astype(np.float32)
        self.note(f"[n={n}]")
        if self.F != "full":
            want = STATE
        else:
            want = OK if self.device or n == 0 else NO_DEVICE
        code, got = self.call(want, lambda: self.m.partial_fit_pairwise(u, i, j, weights=w, margins=True, info=True))
        if code == OK and n > 0:
            self.uploaded()
            self.pending.add("partial_fit")
            self.since.add("fit_weighted")
            if self.grown() and ((u >= self.U0).any() or (i >= self.I0).any() or (j >= self.I0).any()):
                self.facts["fit_weighted_on_an_appended_row"] += 1
        if code == OK and not self.dry:
            x, info = got
            self.P, self.Q, ref = WC.c_pass(self.P, self.Q, u, i, j, w, float(self.lr), float(self.lam))
            hm._same_bits(x, ref, "margins of partial_fit_pairwise(weights=)")
            levels = self.m.triple_levels(u, i, j)[1]
            assert (info["n"], info["pieces"], info["levels"], info["max_width"]) == \
                (n, min(n, 1), levels["levels"], levels["max_width"]), (info, levels)
        self.check_seen_lists()
        self.check_counts()
        return code

    def step(self, rng, kind=None):
        before = len(self.log)
        super().step(rng, kind)
        done = self.log[before].split()[1].split("(")[0]
        if self.log[before].endswith("-> ok") and done in ("mark_seen", "add_items", "add_users", "set_hyper", "fit"):
            self.since.add(done)


def run_sequence(mf, oracle, seed, n_ops, config, *, dry=False):
    """handle_model.run_sequence with the runner above."""
    cfg = dict(blocks=0, waves=0, flags=0, lr=0.02, lam=0.03, seed=7, profile="gpu")
    cfg.update(config)
    rng = np.random.default_rng(seed)
    start = None if dry else mf.debug_device_bytes()
    with tempfile.TemporaryDirectory() as tmpdir:
        run = WarpRunner(mf, oracle, cfg, device=True, dry=dry, wrong=None, tmpdir=tmpdir)
        run.since = set()
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
        except Exception as e:
            raise hm.SequenceMismatch(f"{type(e).__name__}: {e}\nconfig {cfg}, seed {seed}; ops so far:\n" + "\n".join(run.log)) from e
    return run


def _reached(run):
    """What a sequence is for: both calls succeed and are refused, and the pick follows every call that moves what it reads."""
    counts, facts = run.counts, run.facts
    assert counts[("sample_violating", "ok")] >= 5 and counts[("fit_weighted", "ok")] >= 5, dict(counts)
    assert counts[("sample_violating", "STATE")] >= 1 and counts[("fit_weighted", "STATE")] >= 1, dict(counts)
    for what in ("mark_seen", "add_items", "set_hyper", "fit", "fit_weighted"):
        assert facts["violating_after_" + what] >= 1, (what, dict(facts))
    assert counts[("get_factors", "ok")] >= 1 and facts["fit_weighted_on_an_appended_row"] >= 1, dict(facts)


def _seed(geometry):
    """Chosen in the dry run, for what _reached asks; the draws do not depend on the geometry but through L."""
    return 55


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_what_the_sequences_reach(geometry):
    """A dry run: no library, the ops and their outcomes as the model alone gives them."""
    _reached(run_sequence(None, None, _seed(geometry), N_OPS, hm.GEOMETRIES[geometry], dry=True))


@pytest.mark.gpu
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_sequence(mf, oracle, geometry):
    run = run_sequence(mf, oracle, _seed(geometry), N_OPS, hm.GEOMETRIES[geometry])
    _reached(run)
    assert run.facts["violating_found_a_pick"] >= 1 and run.facts["violating_found_none"] >= 1, dict(run.facts)
