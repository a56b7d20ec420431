"""The draw of mfsgd_sample_unseen (include/mfsgd.h) restated in numpy, uint64 throughout: what tests/test_implicit_cpu.py
checks on its own and tests/test_implicit_gpu.py compares the device with, bit for bit."""
import numpy as np

M64 = (1 << 64) - 1
SAMPLE_CHUNK = 1 << 22  # csrc/handle.hpp: kSampleChunk, draws per piece of a call


def _u64(x):
    return np.uint64(int(x) & M64)


def mix32(seed, c):
    """r of the header: the upper 32 bits of splitmix64's output for the counters c (any integer array), as uint64."""
    c = np.asarray(c).astype(np.uint64)
    z = _u64(seed) + _u64(0x9E3779B97F4A7C15) * (c + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * _u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * _u64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(32)


def unseen_at(S, t):
    """The t-th (from 0, ascending) item that is not in the sorted, distinct list S, for an array of t: t + p."""
    S = np.asarray(S, np.int64)
    t = np.asarray(t, np.int64)
    return t + np.searchsorted(S - np.arange(S.size), t, side="right")


def draw(S, n_items, seed, c):
    """The items drawn at the counters c for a user whose seen list is S, among n_items items (int32, shape of c)."""
    c = np.asarray(c)
    cnt = int(n_items) - len(S)
    if cnt == 0:
        return np.full(c.shape, -1, np.int32)
    t = (mix32(seed, c) * np.uint64(cnt)) >> np.uint64(32)
    return unseen_at(S, t).astype(np.int32)


def sample(lists, n_items, users, m, seed=0, first=0):
    """What sample_unseen(users, m, seed, first) must return when user u's list is lists(u) (a callable; sorted and
    distinct).  Rows are grouped by user, so a call of millions of rows over a few users stays vectorised."""
    users = np.asarray(users, np.int64)
    out = np.empty((users.size, m), np.int32)
    d = np.arange(m, dtype=np.uint64)
    for u in np.unique(users):
        rows = np.flatnonzero(users == u)
        c = _u64(first) + rows.astype(np.uint64)[:, None] * np.uint64(m) + d  # first + x * m + d
        out[rows] = draw(lists(int(u)), n_items, seed, c)
    return out


def lists_of(u, i):
    """lists(user) over the distinct pairs (u, i): each user's items, ascending."""
    keys = np.unique((np.asarray(u, np.int64) << 32) | np.asarray(i, np.int64))
    ku, ki = keys >> 32, keys & 0xFFFFFFFF
    return lambda user: ki[np.searchsorted(ku, user):np.searchsorted(ku, user, side="right")]
