"""The premises of tests/test_gpu_fused_setup.py, from the data and the oracle alone (no GPU): every planted length is what it
claims, sits where it claims relative to the sort network's padded sizes and the size classes, and the oracle accepts the
sets."""
import numpy as np

from tests import fused_setup_cases as fc
from tests import setup_edges as se


def _dyadic(r):
    return bool(np.array_equal(r * 16, np.round(r * 16)))


def test_planted_lengths_are_exact_and_on_both_sides_of_every_size():
    c = fc.planted()
    got = se.lengths_of(c.train)
    assert {u: got[u] for u in c.facts["lengths"]} == c.facts["lengths"]
    lengths = sorted(c.facts["lengths"].values())
    assert lengths == sorted(fc.PLANTED_LENGTHS)
    # the network's padded sizes: 64 .. 512 on one wave, 1 024 / 2 048 on four, 4 096 / 8 192 on eight; a length below, on and
    # (up to the last) above each of those the planted set names, and both sides of every class limit
    for size in (64, 128, 512, 2048, 4096, 8192):
        assert size - 1 in lengths and size in lengths and (size + 1 in lengths) == (size < 8192)
    assert (c.facts["mid"], c.facts["long"]) == (3, 6)
    assert max(got.values()) == se.SEG_BLOCK_CAP
    fillers = [n for u, n in got.items() if u >= fc.FIRST_FILLER]
    assert len(fillers) == 200 and min(fillers) >= 5 and max(fillers) <= 40
    assert _dyadic(c.train[2]) and not np.array_equal(c.train[2], np.round(c.train[2]))  # half stars
    assert not np.array_equal(c.train[0], np.sort(c.train[0]))  # shuffled
    assert all(got[int(u)] >= 5 for u in np.unique(c.test[0]))


def test_the_oracle_accepts_the_sets(oracle):
    for c in (fc.planted(), fc.smaller(), fc.non_dyadic()):
        m = oracle.Model(*c.train)
        assert np.array_equal(m.user_iteration_order(), se.user_order(c.train[0]))
        assert m.num_users == len(np.unique(c.train[0])) > 4 and len(c.train[0]) > 4
        assert np.isfinite(m.normalized_deviations()).all() and np.isfinite(m.preprocessed()).all()
        # an order that is not the file order, and norms that a wrong fold order would change in some user
        assert not np.array_equal(se.canonical(c.train), np.arange(len(c.train[0])))


def test_smaller_set():
    c = fc.smaller()
    got = se.lengths_of(c.train)
    assert {u: got[u] for u in c.facts["lengths"]} == dict(zip(range(1, 6), fc.SMALLER_LENGTHS))
    assert (c.facts["mid"], c.facts["long"]) == (1, 1) and len(got) == 55 and _dyadic(c.train[2])
    big = se.lengths_of(fc.planted().train)
    assert all(got[u] != big[u] for u in range(1, 6))  # the same raw ids, other extents


def test_non_dyadic_variant_differs_in_one_rating():
    a, b = fc.planted(), fc.non_dyadic()
    assert np.array_equal(a.train[0], b.train[0]) and np.array_equal(a.train[1], b.train[1])
    diff = np.flatnonzero(a.train[2] != b.train[2])
    assert diff.tolist() == [b.facts["row"]] and b.train[2][diff[0]] == fc.NON_DYADIC_RATING
    assert not _dyadic(b.train[2]) and a.facts["lengths"][int(b.train[0][diff[0]])] == 129


def test_mean_one_user():
    c = fc.planted()
    u, i, r = fc.with_mean_one_user(c)
    mine = r[u == fc.MEAN_ONE_USER]
    assert sorted(mine.tolist()) == [0.5, 1.5] and mine.mean() == 1.0 and mine.min() < 1.0
    assert len(u) == len(c.train[0]) + 2 and _dyadic(r) and fc.MEAN_ONE_USER not in c.train[0]
    assert len(np.unique(u.astype(np.int64) * (1 << 32) + i)) == len(u)


def test_duplicates_stay_in_their_class():
    c = fc.planted()
    by_length = {v: k for k, v in c.facts["lengths"].items()}
    for L, cap in zip(fc.DUPLICATE_LENGTHS, (se.SEG_SHORT_CAP, se.SEG_BLOCK_CAP)):
        u, i, r = se.with_duplicate(c, by_length[L])
        assert len(u) == len(c.train[0]) + 1 and _dyadic(r)
        n = int((u == by_length[L]).sum())
        assert n == L + 1 and n <= cap and (cap == se.SEG_SHORT_CAP or n > se.SEG_MID_CAP)
        pairs = u.astype(np.int64) * (1 << 32) + i
        assert len(np.unique(pairs)) == len(pairs) - 1
