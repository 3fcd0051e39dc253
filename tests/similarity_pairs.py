"""One small fit and a pair list for the bulk similarity tests (numpy only, nothing on disk; no tests in here).

case() builds, once per process, about 40 CRAFTED users over 2 200 items plus a few filler users, with tenth-star ratings
(tests/rating_scales.py: non-dyadic, so a sum's bits depend on its order), and the list of (u, v) pairs that
tests/test_similarity_batch_premises.py examines and tests/test_gpu_similarity_batch.py sends through the library:

  given-order class   rows of 1, 2, 3 and 4 ratings, and seven more of 3 or 4 ratings on the HOT items that every long row
                      holds; the file order of each tiny row is neither its ascending raw-id order nor its trie order
  piece edges         rows of 5, 63, 64, 65, 127, 128 and 129 items (the pair kernels walk a row in 64-entry pieces)
  lopsided            one row of 2 049 items, which contains the rows of 127, 128 and 129
  identical           two users with the same 140 items (inside the long row)
  disjoint            two users with 70 items each and none in common

Pairs: every ordered pair of the crafted users (u == v included), then pairs with one or both raw ids absent from train,
duplicated pairs, and (u, v) directly followed by (v, u)."""
import functools
from dataclasses import dataclass

import numpy as np

from tests import scala_model
from tests.rating_scales import rating_values

N_ITEMS = 2200
HOT = 6                          # the first HOT items of the pool: in every row of 63 items or more
ABSENT = (900_001, 900_002)      # raw user ids outside the fit
PIECE_EDGE_ROWS = (5, 63, 64, 65, 127, 128, 129)
LONG_ROW = 2049
IDENTICAL_ITEMS = 140


@dataclass
class PairCase:
    train: tuple        # (users int32, items int32, ratings float64) in file order
    crafted: list       # raw ids of the crafted users
    tiny: list          # those with <= 4 ratings
    filler: list
    us: np.ndarray      # the pair list
    vs: np.ndarray
    rows: dict          # raw user -> its (item, rating) rows in file order

    @property
    def pairs(self):
        return list(zip(self.us.tolist(), self.vs.tolist()))


def item_orders(items):
    """(ascending raw id, trie order) of a list of distinct items"""
    return sorted(items), sorted(items, key=lambda i: scala_model.trie_key(scala_model.improve(i)))


def _file_order(rng, items):
    """a permutation of `items` that is neither ascending nor the trie order (any order of a single item)"""
    items = list(items)
    if len(items) < 2:
        return items
    asc, trie = item_orders(items)
    if len(items) == 2:  # (two items have two orders: not the ascending one)
        return asc[::-1]
    for _ in range(200):
        cand = [items[j] for j in rng.permutation(len(items))]
        if cand != asc and cand != trie:
            return cand
    raise AssertionError("no file order found")


@functools.lru_cache(maxsize=None)
def case():
    rng = np.random.default_rng([2026, 10, 19])
    pool = (rng.permutation(N_ITEMS) + 1) * 3 + 1          # raw item ids, sparse
    hot = pool[:HOT].tolist()
    long_items = pool[:LONG_ROW].tolist()                  # the long row: hot items and everything the nested rows draw from
    rows, crafted, tiny = {}, [], []
    next_user = [1000]

    def add(items, is_tiny=False):
        u = next_user[0] * 7 + 3
        next_user[0] += 1
        items = _file_order(rng, items) if is_tiny else [items[j] for j in rng.permutation(len(items))]
        rows[u] = [(int(i), float(r)) for i, r in zip(items, rating_values(rng, "tenths", len(items)))]
        crafted.append(u)
        if is_tiny:
            tiny.append(u)
        return u

    def draw(n, source):
        """n items: the hot ones first when n >= 63, the rest drawn from `source`"""
        head = hot if n >= 63 else []
        rest = [i for i in source if i not in set(head)]
        return head + [rest[j] for j in rng.permutation(len(rest))[: n - len(head)]]

    for n in (1, 2, 3, 4):                                   # given-order class, anywhere in the long row
        add(draw(n, long_items[HOT:400]), True)
    for n in (3, 4, 3, 4, 4, 3, 4):                          # given-order class on the hot items
        add([hot[j] for j in rng.permutation(HOT)[:n]], True)
    for n in PIECE_EDGE_ROWS:
        add(draw(n, long_items) if n >= 127 else draw(n, pool[:700].tolist()))
    add(long_items)
    same = draw(IDENTICAL_ITEMS, long_items)
    add(same)
    add(same)
    add(pool[LONG_ROW : LONG_ROW + 70].tolist())             # disjoint from each other and from the long row
    add(pool[LONG_ROW + 70 : LONG_ROW + 140].tolist())
    for n in (9, 17, 33, 40, 80, 96, 150, 200, 260, 300, 400, 520, 700, 1000):  # ordinary rows: lopsided and balanced pairs
        add(draw(n, pool[:1400].tolist()))
    filler = []
    for _ in range(12):
        u = next_user[0] * 7 + 3
        next_user[0] += 1
        items = [int(pool[j]) for j in rng.permutation(N_ITEMS)[:30]]
        rows[u] = [(i, float(r)) for i, r in zip(items, rating_values(rng, "tenths", 30))]
        filler.append(u)
    # file order: every user's rows keep their own order, the users are interleaved at random
    owner = rng.permutation(np.repeat(np.array(list(rows), dtype=np.int64), [len(rows[u]) for u in rows]))
    cursor = {u: 0 for u in rows}
    tu, ti, tr = [], [], []
    for u in owner.tolist():
        i, r = rows[u][cursor[u]]
        cursor[u] += 1
        tu.append(u); ti.append(i); tr.append(r)
    train = (np.asarray(tu, np.int32), np.asarray(ti, np.int32), np.asarray(tr, np.float64))
    pairs = [(u, v) for u in crafted for v in crafted]
    big, t3 = crafted[18], tiny[4]
    pairs += [(ABSENT[0], big), (big, ABSENT[0]), (ABSENT[1], t3), (t3, ABSENT[1]),        # one id absent
              (ABSENT[0], ABSENT[1]), (ABSENT[0], ABSENT[0]),                              # both absent
              (t3, big), (t3, big), (big, t3), (big, t3), (crafted[13], crafted[16]), (crafted[13], crafted[16]),  # duplicates
              (tiny[5], crafted[17]), (crafted[17], tiny[5]), (tiny[6], tiny[7]), (tiny[7], tiny[6])]  # (u, v) then (v, u)
    us, vs = (np.asarray(x, np.int32) for x in zip(*pairs))
    for a in train + (us, vs):
        a.setflags(write=False)
    assert len(rows[big]) == LONG_ROW
    return PairCase(train, crafted, tiny, filler, us, vs, rows)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)
