"""Deterministic rating sets whose ROW LENGTHS decide where the re-rank's candidate stream changes candidate (numpy only).

k_rerank streams the rows of up to 64 candidates per wave as one sequence of 64-entry pieces (rerank.hip: wave_sims) and finds
each entry's candidate from a per-piece start mask.  Which candidates a wave gets, and in what order, depends on atomics in
select, so the only way to pin a boundary to a lane is to make the row lengths uniform: with every row L long, candidate j
of any wave starts at stream position j * L, whoever it is.  tests/test_rerank_stream_premises.py proves from the data (and the
oracle) that every case is what it claims to be; tests/test_gpu_rerank_stream.py pins each of them to the oracle.

Conventions of every case (those of tests/boundary_shapes.py): raw user ids are exactly 1..U and raw item ids exactly 1..I;
ratings are half stars 1.0 .. 5.0; no user's training ratings are all equal; every user has at least 5 training ratings."""
import functools

import numpy as np

from tests.boundary_shapes import Case, _Rows, _half_stars, _varied

PIECE = 64        # entries per piece of the stream (the premise file holds the kernel's constants as literals)
UNIFORM_U, UNIFORM_I = 520, 300


def _distinct_items(rng, n, weights):
    """n distinct raw item ids drawn without replacement by the weights (over items 1..len(weights))"""
    return rng.choice(len(weights), size=n, replace=False, p=weights) + 1


def _skew(I):
    w = 1.0 / (np.arange(I, dtype=np.float64) + 8.0)
    return w / w.sum()


def uniform_rows(L, U=UNIFORM_U, I=UNIFORM_I, n_test=3, seed=0):
    """every user has exactly L training ratings, on items drawn from a skewed distribution (so that rows overlap), and
    n_test test ratings on other items"""
    rng = np.random.Generator(np.random.PCG64(4100 + 7 * L + U + seed))
    w = _skew(I)
    perm = rng.permutation(I)  # which raw item holds which popularity rank
    rows = _Rows()
    for u in range(1, U + 1):
        it = perm[_distinct_items(rng, L + n_test, w) - 1] + 1
        rows.add(u, it[:L], _varied(rng, L), False)
        rows.add(u, it[L:], _half_stars(rng, n_test), True)
    return rows.finish(rng, U, I, {"all": np.arange(1, U + 1)})


def giant_rows(U=300, I=3200, seed=0):
    """user 1 rates items 1..3000; users 2..21 rate 513..700 items each (ten fixed ones of the last 200 items among them, which
    nobody else need rate); the rest 5..70 items from a skewed distribution over all items"""
    rng = np.random.Generator(np.random.PCG64(5200 + U + I + seed))
    rows = _Rows()
    w = _skew(I)
    perm = rng.permutation(I)
    rows.add(1, np.arange(1, 3001), _varied(rng, 3000), False)
    rows.add(1, np.arange(3001, 3006), _half_stars(rng, 5), True)
    heavy = np.arange(2, 22)
    for j, u in enumerate(heavy):
        n = int(rng.integers(513, 701))
        own = 3001 + 10 * j + np.arange(10)
        others = perm[_distinct_items(rng, n + 4, w) - 1] + 1
        others = others[~np.isin(others, own)]
        rows.add(u, own, _half_stars(rng, 10), False)
        rows.add(u, others[:n - 10], _varied(rng, n - 10), False)
        rows.add(u, others[n - 10:n - 7], _half_stars(rng, 3), True)
    light = np.arange(22, U + 1)
    for u in light:
        n = int(np.clip(rng.lognormal(np.log(22.0), 0.7), 5, 70))
        it = perm[_distinct_items(rng, n + 2, w) - 1] + 1
        rows.add(u, it[:n], _varied(rng, n), False)
        rows.add(u, it[n:], _half_stars(rng, 2), True)
    return rows.finish(rng, U, I, {"giant": [1], "heavy": heavy, "light": light})


def clone_rows(n_clones=100, n_disjoint=100, shared=64, own=8, seed=0):
    """users 1..n_clones rate the same `shared` items (1..shared) with differing ratings; the n_disjoint users behind them rate
    `own` items each that nobody else rates.  Test rows: two of the shared items for the disjoint users (they stay out of
    every TRAINING row of theirs), two items of a disjoint user for every clone."""
    rng = np.random.Generator(np.random.PCG64(6300 + n_clones + seed))
    U, I = n_clones + n_disjoint, shared + own * n_disjoint
    rows = _Rows()
    clones = np.arange(1, n_clones + 1)
    disjoint = np.arange(n_clones + 1, U + 1)
    for u in clones:
        rows.add(u, np.arange(1, shared + 1), _varied(rng, shared), False)
    for j, u in enumerate(disjoint):
        rows.add(u, shared + 1 + own * j + np.arange(own), _varied(rng, own), False)
        rows.add(u, [1 + j % shared, 1 + (j + 7) % shared], _half_stars(rng, 2), True)
    for u in clones:
        rows.add(u, shared + 1 + own * ((u * 3) % n_disjoint) + np.arange(2), _half_stars(rng, 2), True)
    return rows.finish(rng, U, I, {"clones": clones, "disjoint": disjoint}, {"shared": np.arange(1, shared + 1)})


_CASES = {
    "all63": lambda: uniform_rows(63),
    "all64": lambda: uniform_rows(64),
    "all65": lambda: uniform_rows(65),
    "all5": lambda: uniform_rows(5, U=300, I=40, n_test=2),
    "giant": giant_rows,
    "clones": clone_rows,
    "clones400": lambda: clone_rows(n_clones=300, n_disjoint=100, seed=1),  # kcap = 399: the shortlist tile of 1024, 512-product buffers
}


@functools.lru_cache(maxsize=None)
def case(name):
    return _CASES[name]()


def row_lengths(c):
    """training ratings of every raw user id, at [id - 1]"""
    return np.bincount(c.train[0], minlength=c.num_users + 1)[1:]
