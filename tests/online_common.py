"""What the online-update tests share (tests/test_online_cpu.py, tests/test_online_gpu.py): the definition of the
dependency levels restated in Python, the order they stand for, and the batches that reach each shape of a level list."""
import numpy as np

PIECE = 1 << 20  # ratings per piece (include/mfsgd.h, "online updates")


def py_levels(u, i):
    """level[j] as include/mfsgd.h defines it, piece by piece."""
    level = np.zeros(len(u), np.int32)
    for j0 in range(0, len(u), PIECE):
        last_u, last_i = {}, {}
        for j in range(j0, min(j0 + PIECE, len(u))):
            a, b = int(u[j]), int(i[j])
            level[j] = 1 + max(last_u.get(a, -1), last_i.get(b, -1))
            last_u[a] = last_i[b] = level[j]
    return level


def py_info(level):
    """The fields of mfsgd_online_info that follow from the levels."""
    n = len(level)
    pieces, levels, max_width = 0, 0, 0
    for j0 in range(0, n, PIECE):
        width = np.bincount(level[j0:j0 + PIECE])
        pieces, levels, max_width = pieces + 1, levels + width.size, max(max_width, int(width.max()))
    return dict(n=n, pieces=pieces, levels=levels, max_width=max_width)


def level_order(level, reverse=False):
    """The ratings in a stable sort by (piece, level); with reverse, each level's ratings backwards."""
    n = len(level)
    piece = np.arange(n, dtype=np.int64) // PIECE
    within = -np.arange(n, dtype=np.int64) if reverse else np.arange(n, dtype=np.int64)
    return np.lexsort((within, level, piece)).astype(np.int64)


def _ratings(rng, n):
    return (rng.integers(1, 11, n) * 0.5).astype(np.float32)


def random_batch(U=37, I=29, n=3000, seed=5):
    rng = np.random.default_rng(seed)
    return U, I, rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32), _ratings(rng, n)


def distinct_batch(n=5000, seed=6):
    """No user and no item twice: one level."""
    rng = np.random.default_rng(seed)
    return n, n, rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32), _ratings(rng, n)


def one_item_batch(n=600, seed=7):
    """n users rate item 3: n levels of width 1."""
    rng = np.random.default_rng(seed)
    return n, 5, rng.permutation(n).astype(np.int32), np.full(n, 3, np.int32), _ratings(rng, n)


def one_user_batch(n=600, seed=8):
    U, I, u, i, r = one_item_batch(n, seed)
    return I, U, i, u, r


def same_pair_batch(n=300, seed=9):
    rng = np.random.default_rng(seed)
    return 4, 6, np.full(n, 2, np.int32), np.full(n, 5, np.int32), _ratings(rng, n)


def two_piece_batch(extra, seed=10, U=3001, I=3001):
    n = PIECE + extra
    rng = np.random.default_rng(seed)
    return U, I, rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32), _ratings(rng, n)


def hot_item_batch(U=4096, I=4096, n=12000, seed=11):
    """A wide random batch in which every 40th rating is of item 7."""
    rng = np.random.default_rng(seed)
    u, i = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    i[::40] = 7
    return U, I, u, i, _ratings(rng, n)


def boundary_widths(G):
    """Level widths around G = ratings of one workgroup pass: exactly G, G + 1 and 1 in succession, then up again by
    doubling (every narrow width on the way), over the boundary once more and down."""
    up = [1 << x for x in range(1, 20) if (1 << x) < G]
    return [G, G + 1, 1] + up + [G, G + 1, G, 1]


def widths_batch(widths, seed=12):
    """Levels of exactly the given widths, in succession (each at most twice the one before).  Rating x of level l is
    of user x.  Where the level before has a rating x, that user carries the dependence and the item is a fresh one;
    where it has not, the rating takes the item of rating x - prev of the level before, which nobody else rates."""
    rng = np.random.default_rng(seed)
    W = max(widths)
    u, i, before = [], [], []
    for l, w in enumerate(widths):
        prev = len(before) if l else w
        assert w <= 2 * prev
        items = [l * W + x if x < prev else before[x - prev] for x in range(w)]
        u += range(w)
        i += items
        before = items
    u, i = np.array(u, np.int32), np.array(i, np.int32)
    return W, len(widths) * W, u, i, _ratings(rng, u.size)
