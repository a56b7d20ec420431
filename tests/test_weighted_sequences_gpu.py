"""The weighted draw inside the life of one handle: set_item_weights, clear_item_weights and sample_unseen_weighted drawn
between set_seen / mark_seen / clear_seen, add_users / add_items, reserve and the factor calls, on a handle and on the model
of tests/handle_model.py in lock step.  handle_model.py is imported as it is: the runner below adds the three ops to its
Runner, keeps the weights the handle should hold (and the item count they were set for) beside the model's index, and
answers every draw and every unseen mass with the restatement (tests/weighted_common.py) over its own lists.  What a
sequence reaches depends on the seed and the model's abstract state alone, so it is checked in a dry run, without a GPU."""
import tempfile

import numpy as np
import pytest

from tests import handle_model as hm
from tests import weighted_common as WC

OK, INVALID, NO_DEVICE, STATE = hm.OK, hm.INVALID, hm.NO_DEVICE, hm.STATE
KINDS = dict(init_factors=1.5, set_factors=0.3, set_seen=1.5, mark_seen=1.5, clear_seen=0.3, add_users=1, add_items=0.6, reserve=0.5,
             seen_size=0.5, get_factors=0.5)  # x handle_model's weight
NEW = dict(set_weights=7, clear_weights=0.7, sample_weighted=12)
N_OPS = 70
SEED = 29  # chosen in the dry run, for what _reached asks


class WeightedRunner(hm.Runner):
    def weights(self):
        base = super().weights()
        w = {kind: base[kind] * scale for kind, scale in KINDS.items()}
        w.update(NEW)
        return w

    def lists(self):
        keys = self.seen
        return lambda u: (keys[np.searchsorted(keys, u << 32):np.searchsorted(keys, (u + 1) << 32)] & 0xFFFFFFFF)

    def check_weights(self):
        if not self.dry:
            got = self.m.item_weights()
            assert (got is None) == (self.w is None) and (got is None or np.array_equal(got, self.w)), "item_weights() differ"

    def op_set_weights(self, g):
        """Weights for the current item count (a third of them zero, or all, or huge), or for another count: refused."""
        v = ("some", "some", "some", "huge", "zero", "short")[int(g.integers(6))]
        n = self.I - 1 if v == "short" else self.I
        w = g.integers(1, 7, n).astype(np.uint32)
        w[g.random(n) < 0.35] = 0
        if v == "huge":
            w = np.where(w > 0, 0xFFFFFFFF, 0).astype(np.uint32)
        if v == "zero":
            w[:] = 0
        self.note(f"[{v}: n={n}, items {self.I}, index={'none' if self.seen is None else self.seen.size}]")
        code, _ = self.call(INVALID if v == "short" else OK if self.device else NO_DEVICE, lambda: self.m.set_item_weights(w))
        if code == OK:
            if self.w is not None and self.w.size != self.I:
                self.facts["weights_set_again_after_add_items"] += 1
            if self.seen is not None and self.seen.size:
                self.facts["weights_set_on_an_index_with_pairs"] += 1
            self.w = w
        self.check_weights()
        return code

    def op_clear_weights(self, g):
        code, _ = self.call(OK, lambda: self.m.clear_item_weights())
        self.w = None
        self.check_weights()
        return code

    def op_sample_weighted(self, g):
        """0 .. 200 rows over the current users, appended ones among them."""
        n = 0 if int(g.integers(8)) == 0 else int(g.integers(1, 201))
        users = g.integers(0, self.U, n).astype(np.int32)
        m = int(g.choice([1, 3, 7]))
        seed, first = int(g.integers(1 << 30)), int(g.integers(1 << 40))
        self.note(f"[n={n}, m={m}, index={'none' if self.seen is None else self.seen.size}, "
                  f"weights={'none' if self.w is None else self.w.size}, items {self.I}]")
        if self.seen is None or self.w is None or self.w.size != self.I:
            want = STATE
        else:
            want = OK if self.device or n == 0 else NO_DEVICE
        code, got = self.call(want, lambda: self.m.sample_unseen_weighted(users, m, seed, first, mass=True))
        if code == STATE and self.seen is not None and self.w is not None:
            self.facts["refused_for_stale_weights"] += 1
            if not self.dry:
                assert f"item weights cover {self.w.size} items, the model has {self.I}" in self.last_msg, self.last_msg
        if code == OK and n > 0:
            for what in sorted(self.since):
                self.facts["weighted_after_" + what] += 1
            self.since.clear()
            if (users >= self.U0).any():
                self.facts["weighted_for_an_appended_user"] += 1
        if code == OK:  # (the restatement needs the index and the weights alone: a dry run has both)
            items, mass = WC.sample_weighted(self.lists(), self.w, users, m, seed, first, mass=True)
            if not self.dry:
                assert got[0].dtype == np.int32 and got[0].tobytes() == items.tobytes(), "draws differ from the model's"
                assert got[1].dtype == np.int64 and got[1].tobytes() == mass.tobytes(), "unseen masses differ from the model's"
            if n and (items >= 0).any():
                self.facts["weighted_drew_an_item"] += 1
            if n and (items < 0).any():
                self.facts["weighted_had_nothing_to_draw"] += 1
        self.check_weights()
        self.check_seen_lists()  # the index is as it was
        return code

    def step(self, rng, kind=None):
        before = len(self.log)
        super().step(rng, kind)
        done = self.log[before].split()[1].split("(")[0]
        if self.log[before].endswith("-> ok") and done in ("set_seen", "mark_seen", "add_users", "add_items", "reserve"):
            self.since.add(done)


def run_sequence(mf, oracle, seed, n_ops, config, *, dry=False):
    """handle_model.run_sequence with the runner above."""
    cfg = dict(blocks=0, waves=0, flags=0, lr=0.02, lam=0.03, seed=7, profile="gpu")
    cfg.update(config)
    rng = np.random.default_rng(seed)
    start = None if dry else mf.debug_device_bytes()
    with tempfile.TemporaryDirectory() as tmpdir:
        run = WeightedRunner(mf, oracle, cfg, device=True, dry=dry, wrong=None, tmpdir=tmpdir)
        run.since, run.w = set(), None
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
    """What the sequence is for: the draw succeeds and is refused, and follows every call that moves what it reads."""
    counts, facts = run.counts, run.facts
    assert counts[("sample_weighted", "ok")] >= 8 and counts[("sample_weighted", "STATE")] >= 2, dict(counts)
    assert counts[("set_weights", "ok")] >= 3 and counts[("set_weights", "INVALID_ARG")] >= 1, dict(counts)
    for what in ("mark_seen", "set_seen", "add_users"):
        assert facts["weighted_after_" + what] >= 1, (what, dict(facts))
    for what in ("weights_set_on_an_index_with_pairs", "weights_set_again_after_add_items", "refused_for_stale_weights",
                 "weighted_for_an_appended_user", "weighted_drew_an_item", "weighted_had_nothing_to_draw"):
        assert facts[what] >= 1, (what, dict(facts))


def test_what_the_sequence_reaches():
    """A dry run: no library, the ops and their outcomes as the model alone gives them."""
    _reached(run_sequence(None, None, SEED, N_OPS, hm.GEOMETRIES["k8"], dry=True))


@pytest.mark.gpu
def test_sequence(mf, oracle):
    run = run_sequence(mf, oracle, SEED, N_OPS, hm.GEOMETRIES["k8"])
    _reached(run)
