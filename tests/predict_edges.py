"""Deterministic inputs for the kNN PREDICTION kernels (numpy only): training sets whose match counts are exact by construction,
and test batches whose run structure — in the order the engine sorts them into — sits on the kernels' fixed sizes.
tests/test_predict_edge_premises.py proves from the data and the oracle that every case is what it claims to be;
tests/test_gpu_predict_edges.py pins every case to the oracle, bit for bit, through each of the four kernels.

A row's MATCHES are the neighbours of its user that rated its item.  With the handle's k at 2048 and U <= 2049 users,
kcap = U - 1 and every other user is in every list: on a planted item rated by exactly c users a user who did not rate it has
exactly c matches and one who did has c - 1.  The raters of a planted item with c >= 4 include the users at dense index 0, 63,
64 and U - 1 (boundary_shapes.users_by_dense): the first bit and the last bit of bitmap word 0, the first bit of word 1 and the
last valid bit of the last word.

Conventions of planted(): raw user ids are exactly 1..U; every user rates six of the background items 2..40 with half stars
that are not all equal (more than 4 ratings each: the memo-order rule SURVEY N6 stays out of it); the planted items take the
ids 41, 42, ... in the order of the counts; rows are in a seeded shuffled order."""
import functools
import re
from dataclasses import dataclass

import numpy as np

from tests.boundary_shapes import trie_keys, users_by_dense

K = 2048  # the handle's k: kcap = U - 1 in every case
COUNTS = (1, 4, 5, 64, 65, 68, 69, 128, 129, 132, 192, 193)  # + U - 1 and U, all clipped to <= U and de-duplicated
GROUPED_USERS = (65, 66, 129, 257, 258, 321, 322, 513)  # kcap 64 .. 512: the bottom and the top of each TR form
GENERAL_USERS = (514, 1025, 2049)                       # kcap 513, 1024, 2048: the general kernel's CAP = 1024 and 2048
RUN_USERS = (65, 257, 513)                              # one case per G of the grouped kernels: G = 4, 2, 1
UNKNOWN_USER = 900_001   # (+ 0, 1, 2, ...: ids the train set lacks)
UNKNOWN_ITEM = 800_001
WAVES = 4                # waves per workgroup of both grouped kernels
ITEM_CHUNK = 64          # rows per workgroup of the item-grouped kernel and of the sweep
ROW_CHUNK = 32           # rows per wave of the row-grouped kernel
RUN_KEYS = 20            # no batch of run_batch() has more runs than this
# the seed of every case: picked (once, on the CPU oracle) so that the conditions on the INPUTS that the premise file asserts
# hold — a match of similarity exactly 0.0, matches of both signs, and file order folding to other bits than id / list order
SEEDS = {65: 2, 66: 1, 129: 1, 257: 1, 258: 1, 321: 1, 322: 1, 513: 1, 514: 1, 1025: 1, 2049: 1}


def counts_of(U):
    """the rater counts of the planted items of case U, in planting order"""
    return tuple(dict.fromkeys(min(c, U) for c in COUNTS + (U - 1, U)))


def planned_matches(U):
    """the match counts the case's test rows must show: c for the non-rater (there is none at c = U), c - 1 for the rater"""
    out = set()
    for c in counts_of(U):
        out.add(c - 1)
        if c < U:
            out.add(c)
    return out


@dataclass
class Case:
    num_users: int
    train: tuple     # (users int32, items int32, ratings float64), shuffled
    test: tuple      # the planted rows: per planted item one non-rater (where there is one), then one rater
    matches: tuple   # the planned match count of every test row
    items: dict      # c -> raw id of the planted item with c raters
    raters: dict     # c -> raw ids of its raters


def planted(U, counts, seed):
    rng = np.random.Generator(np.random.PCG64(52_000 + 97 * U + seed))
    order = users_by_dense(U)
    corner = order[list(dict.fromkeys((0, 63, 64, U - 1)))]  # (U = 65: dense 64 is the last user)
    users = np.arange(1, U + 1, dtype=np.int64)
    bg_items = np.argsort(rng.random((U, 39)), axis=1)[:, :6] + 2
    bg_r = rng.integers(2, 11, (U, 6)) / 2.0
    bg_r[:, 0], bg_r[:, 1] = 1.5, 4.5  # never all equal
    bg_r = np.take_along_axis(bg_r, np.argsort(rng.random((U, 6)), axis=1), axis=1)
    u, i, r = [np.repeat(users, 6)], [bg_items.reshape(-1)], [bg_r.reshape(-1)]
    items, raters, tu, ti, tm = {}, {}, [], [], []
    for j, c in enumerate(counts):
        assert 1 <= c <= U and c not in items
        item = 41 + j
        if c >= 4:
            rest = rng.permutation(np.setdiff1d(users, corner))[:c - len(corner)]
            who = np.concatenate([corner, rest])
        else:
            who = rng.permutation(np.setdiff1d(users, corner))[:c]
        who = rng.permutation(who)
        items[c], raters[c] = item, np.sort(who).astype(np.int32)
        u.append(who)
        i.append(np.full(c, item, dtype=np.int64))
        r.append(rng.integers(2, 11, c) / 2.0)
        out = np.setdiff1d(users, who)
        if len(out):
            tu.append(int(rng.choice(out)))
            ti.append(item)
            tm.append(c)
        tu.append(int(rng.choice(who)))
        ti.append(item)
        tm.append(c - 1)
    u, i, r = np.concatenate(u), np.concatenate(i), np.concatenate(r)
    rows = rng.permutation(len(u))
    train = (u[rows].astype(np.int32), i[rows].astype(np.int32), r[rows].copy())
    test = (np.asarray(tu, dtype=np.int32), np.asarray(ti, dtype=np.int32), rng.integers(2, 11, len(tu)) / 2.0)
    return Case(U, train, test, tuple(tm), items, raters)


@functools.lru_cache(maxsize=None)
def case(U):
    return planted(U, counts_of(U), SEEDS[U])


def with_unknowns(c):
    """the planted rows plus an unknown-user row and an unknown-item row"""
    u = np.concatenate([c.test[0], [UNKNOWN_USER, c.test[0][0]]]).astype(np.int32)
    i = np.concatenate([c.test[1], [c.test[1][0], UNKNOWN_ITEM]]).astype(np.int32)
    return u, i, np.concatenate([c.test[2], [3.0, 4.0]])


# ---- batches with a planted run structure ---------------------------------------------------------------------------------
def items_by_dense(train):
    """the fit's raw item ids in dense order"""
    ids = np.unique(train[1]).astype(np.int64)
    return ids[np.argsort(trie_keys(ids), kind="stable")]


def engine_order(train, batch, by_item):
    """the permutation the engine sorts a batch into: a stable sort by dense item (user) index, unknown ones last"""
    known = items_by_dense(train) if by_item else users_by_dense(int(train[0].max()))
    col = np.asarray(batch[1 if by_item else 0], dtype=np.int64)
    dense = np.full(int(max(known.max(), col.max())) + 1, len(known), dtype=np.int64)
    dense[known] = np.arange(len(known))
    return np.argsort(dense[col], kind="stable")


def parse_form(form):
    """'items TR=4 G=2' -> ('items', 2)"""
    m = re.fullmatch(r"(items|rows) TR=\d+ G=(\d+)", form)
    return m.group(1), int(m.group(2))


class _Runs:
    """runs of rows of one key (item or user), laid out in the order of the sorted batch; a None in a run's `others` is a row
    the train set cannot place in the OTHER column (inactive inside the run)"""

    def __init__(self, rng, keys, others):
        self.rng, self.keys, self.others = rng, list(keys), np.asarray(others)
        self.runs, self.n, self.at = [], 0, 0

    def add(self, length, inactive=()):
        """a run of `length` rows of the next key; rows at the positions `inactive` of it (or all of it: "all") are inactive"""
        assert length > 0 and self.keys, "out of keys"
        key = self.keys.pop(0)
        if isinstance(inactive, str):
            inactive = range(length)
        col = []
        for j in range(length):
            col.append(None if j in set(inactive) else int(self.others[self.at % len(self.others)]))
            self.at += 1
        self.runs.append((key, col))
        self.n += length
        return self

    def align(self, chunk, residue=0):
        """a filler run up to the next row index that is `residue` modulo `chunk`"""
        gap = (residue - self.n) % chunk
        return self.add(gap) if gap else self


def _heavy_first(c, n):
    """the items that the runs of an item-sorted batch take, in dense order: the first n are planted items with more than 65
    raters where the case has them (every row of their runs has more than 64 matches, so all waves of the workgroup are in
    the windowed fold together), then the items behind the last of those"""
    dense = items_by_dense(c.train).tolist()
    heavy = {item for cnt, item in c.items.items() if cnt > 65}
    first = [j for j, item in enumerate(dense) if item in heavy][:n]
    if len(first) < n or len(dense) - first[-1] - 1 < RUN_KEYS - n:  # (too few items behind them for the other runs)
        return dense
    return [dense[j] for j in first] + dense[first[-1] + 1:]


def run_batch(c, form):
    """A batch for the grouped kernel of `form` ('items TR=.. G=..' or 'rows TR=.. G=..'), shuffled so that rows of one run
    keep their order (the engine's sort is stable, so the planted positions inside a run survive).  Returns
    (users, items, ratings): the structure is what tests/test_predict_edge_premises.py reads back out of engine_order()."""
    kind, G = parse_form(form)
    U = c.num_users
    rng = np.random.Generator(np.random.PCG64(71_000 + 13 * U + G + (0 if kind == "items" else 500)))
    if kind == "items":
        W = WAVES * G  # rows of a run that a workgroup takes per trip
        runs = _Runs(rng, _heavy_first(c, 4), rng.permutation(np.arange(1, U + 1)))
        runs.add(64)                      # chunk 0: one run fills it
        runs.add(63)                      # chunk 1 but its last row
        runs.add(65)                      # starts on the last row of chunk 1, fills chunk 2
        runs.add(129)                     # chunks 3 and 4 and the FIRST row of chunk 5
        runs.add(1).add(W - 1).add(W).add(W + 1)
        runs.align(ITEM_CHUNK)
        # unknown users in the first, a middle and the last slot of a group of G (trips 0, 1 and 2 of wave 0)
        runs.add(3 * W, inactive=(0, W + G // 2, 2 * W + G - 1))
        runs.add(5, inactive="all").add(3)  # the bitmap load is skipped for the first: the second must load its own
        runs.align(ITEM_CHUNK)
        runs.add(4, inactive="all").add(2)  # the same at the start of a chunk: nothing was loaded before
        n_unknown = 4
        runs.align(ITEM_CHUNK, (1 - n_unknown) % ITEM_CHUNK)  # with the unknown-item rows behind: a last chunk of 1 row
        tail = [(UNKNOWN_ITEM + j, [int(v)]) for j, v in enumerate(rng.permutation(np.arange(1, U + 1))[:n_unknown - 1])]
        tail.append((UNKNOWN_ITEM + n_unknown, [None]))  # (neither the user nor the item is known)
    else:
        its = items_by_dense(c.train)
        runs = _Runs(rng, users_by_dense(U), rng.permutation(its))
        runs.add(32)                      # wave 0: one user
        runs.add(31)                      # wave 1 but its last row
        runs.add(33)                      # starts on the last row of wave 1, fills wave 2
        runs.add(65)                      # waves 3 and 4 and the first row of wave 5
        runs.add(1)
        for length in (G - 1, G, G + 1):  # G + 1 (and G - 1 > 0): the user changes in the middle of a group
            if length > 0:
                runs.add(length)
        runs.align(ROW_CHUNK)
        runs.add(3 * G + 3, inactive=(0, G + 1, 3 * G + 2))  # unknown items inside a user's run: first, inner, last row
        runs.add(G + 1).add(3, inactive="all").add(2)
        n_unknown = 3
        runs.align(ROW_CHUNK, (1 - n_unknown) % ROW_CHUNK)    # with the unknown-user rows behind: a last wave of 1 row
        tail = [(UNKNOWN_USER + j, [int(v)]) for j, v in enumerate(rng.permutation(its)[:n_unknown - 1])]
        tail.append((UNKNOWN_USER + n_unknown, [None]))
    assert len(runs.runs) <= RUN_KEYS
    key_col, other_col, run_of = [], [], []
    for j, (key, col) in enumerate(runs.runs + tail):
        for v in col:
            key_col.append(int(key))
            other_col.append(v)
            run_of.append(j)
    n = len(key_col)
    fill = (UNKNOWN_USER if kind == "items" else UNKNOWN_ITEM) + 50
    other_col = [fill + j if v is None else v for j, v in enumerate(other_col)]
    # shuffle across runs, keep the order inside every run
    slot = rng.permutation(n)
    run_of = np.asarray(run_of)
    for j in range(run_of.max() + 1):
        slot[run_of == j] = np.sort(slot[run_of == j])
    k_arr, o_arr = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    k_arr[slot], o_arr[slot] = key_col, other_col
    ratings = rng.integers(2, 11, n) / 2.0
    return (o_arr, k_arr, ratings) if kind == "items" else (k_arr, o_arr, ratings)


# ---- the sweep's lists of k -------------------------------------------------------------------------------------------------
def sweep_ks(kcap):
    """strictly ascending lists of 1, 63 and 64 values of k (64 is the ABI's limit: one lane per k).  The long lists hold 1, 63,
    64, 65, kcap - 1, kcap and one value above kcap (kcap + 7; none at kcap = 2048, the largest k there is): list positions on
    both sides of `j >= ks[q]` at the 64-neighbour trip boundaries and at the end of the list.  The single value is kcap - 1:
    the table is built for the largest k of a list, so this one keeps the case's kernel form with one live lane, and cuts exactly
    the last neighbour off every list."""
    top = min(2048, kcap + 7)
    must = sorted({v for v in (1, 63, 64, 65, kcap - 1, kcap, top) if 1 <= v <= 2048})
    out = [[kcap - 1]]
    for n_k in (63, 64):
        rest = [v for v in np.unique(np.linspace(2, top - 1, 4 * n_k).astype(int)).tolist() if v not in must]
        step = len(rest) / (n_k - len(must))
        picked = [rest[int(j * step)] for j in range(n_k - len(must))]
        ks = sorted(must + picked)
        assert len(ks) == n_k == len(set(ks))
        out.append(ks)
    return out
