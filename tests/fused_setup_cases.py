"""Rating sets for the fit's fused set-up kernels (prep.hip k_user_setup; numpy only): one planted user per training-row
length on either side of every padded size of the register sort network (64, 128, 512, 2 048, 4 096, 8 192), of the split of
its strides into lane, register and LDS exchanges, and of the three size classes, among about 200 filler users.  Ratings
are half stars, so a whole-file fit takes the fused path (means, deviations, norms and preprocessed ratings inside the sort
kernels); the variants below send the same users down the other paths or make the fit fail.
tests/test_fused_setup_premises.py proves on the CPU that every set is what it claims to be;
tests/test_gpu_fused_setup.py pins each to the oracle."""
import functools

import numpy as np

from tests import setup_edges as se

PLANTED_LENGTHS = (1, 2, 5, 63, 64, 65, 127, 128, 129, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192)
SMALLER_LENGTHS = (5, 64, 129, 513, 2049)
ITEMS = 9000
FIRST_FILLER = 101
NON_DYADIC_RATING = 3.37
MEAN_ONE_USER = 9001          # two ratings, 0.5 and 1.5: the mean is exactly 1 and 0.5 lies below it
DUPLICATE_LENGTHS = (127, 4096)  # a one-wave segment and a 512-thread one (4 097 rows with the duplicate)


def _build(lengths, fillers, seed):
    rng = np.random.Generator(np.random.PCG64(31000 + seed))
    rows = []
    for j, L in enumerate(lengths):
        its = rng.choice(ITEMS, L + (2 if L >= 5 else 0), replace=False) + 1
        rows.append((1 + j, its[:L], its[L:]))
    for j in range(fillers):
        L = int(rng.integers(5, 41))
        its = rng.choice(ITEMS, L + 2, replace=False) + 1
        rows.append((FIRST_FILLER + j, its[:L], its[L:]))
    train, test = se._assemble(rng, rows, "half")
    planted = np.arange(1, len(lengths) + 1, dtype=np.int32)
    c = se.Case(train, test, planted, np.empty(0, dtype=np.int32), True,
                {"lengths": dict(zip(planted.tolist(), lengths)),
                 "mid": sum(se.SEG_SHORT_CAP < L <= se.SEG_MID_CAP for L in lengths),
                 "long": sum(se.SEG_MID_CAP < L <= se.SEG_BLOCK_CAP for L in lengths)})
    for cols in (c.train, c.test):
        for a in cols:
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def planted():
    """the 20 planted users (raw ids 1 .., in the order of PLANTED_LENGTHS) and 200 fillers of 5 - 40 ratings"""
    return _build(PLANTED_LENGTHS, 200, 0)


@functools.lru_cache(maxsize=None)
def smaller():
    """a second, smaller set for a re-fit of the same handle: other users at the same raw ids, other row extents"""
    return _build(SMALLER_LENGTHS, 50, 1)


@functools.lru_cache(maxsize=None)
def non_dyadic():
    """planted() with one rating of the 129-row user off the dyadic grid: the fit must build perm_uf and take the unfused chain"""
    c = planted()
    user = {v: k for k, v in c.facts["lengths"].items()}[129]
    r = c.train[2].copy()
    row = int(np.flatnonzero(c.train[0] == user)[7])
    r[row] = NON_DYADIC_RATING
    r.setflags(write=False)
    return se.Case((c.train[0], c.train[1], r), c.test, c.planted, c.items, True, dict(c.facts, row=row))


def with_mean_one_user(c):
    """the training rows of c plus a user whose two ratings 0.5 and 1.5 average exactly 1: scale(0.5, 1) == 0"""
    u, i, r = c.train
    at = len(u) // 3
    return (np.insert(u, [at, at], MEAN_ONE_USER).astype(np.int32), np.insert(i, [at, at], [11, 12]).astype(np.int32),
            np.insert(r, [at, at], [0.5, 1.5]))
