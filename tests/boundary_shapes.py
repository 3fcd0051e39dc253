"""Deterministic rating sets whose SHAPE sits on the fixed sizes of the neighbour build (numpy only): the 256-row GEMM tile and
U_pad, the 64-column K_pad, the 16 384-column tile of k_tail_select, its 12 register-held tiles, its 256-entry chunks and its
1024-piece table.  tests/test_boundary_premises.py proves from the data (and the oracle) that every case is what it claims to
be; tests/test_gpu_boundary_shapes.py pins each of them to the oracle.

Conventions of every case: raw user ids are exactly 1..U and raw item ids exactly 1..I; ratings are half stars 1.0 .. 5.0; no
user's training ratings are all equal (scale() is never 0, no norm is 0); every user has at least 5 training ratings (the
<= 4-rating memo-order rule stays out of it); rows are in a seeded shuffled order.

A user's DENSE index — the column of the similarity panel it owns, and so its tile — is the rank of its raw id in Scala's
HashSet iteration order (common.h: trie_key(improve(id))), not id - 1: users_by_dense(U)[d] is the raw id of dense index d,
and every planted "edge" user is placed by dense index.  The premise file checks this order against the oracle's."""
import functools
from dataclasses import dataclass, field

import numpy as np

K = 50        # the neighbourhood size of every case that does not vary k
TILE = 16384  # columns per tile of k_tail_select (the premise file holds the kernel's constants as literals)
_M = np.uint64(0xFFFFFFFF)


def trie_keys(ids):
    """common.h int_trie_key of every id: ascending keys == HashSet iteration order == dense order"""
    h = np.asarray(ids, dtype=np.int64).astype(np.uint64) & _M
    h = (h + (~(h << np.uint64(9)) & _M)) & _M
    h ^= h >> np.uint64(14)
    h = (h + (h << np.uint64(4))) & _M
    h ^= h >> np.uint64(10)
    key = (h >> np.uint64(30)) & np.uint64(3)
    for digit, shift in enumerate((27, 22, 17, 12, 7, 2)):
        key |= ((h >> np.uint64(5 * digit)) & np.uint64(31)) << np.uint64(shift)
    return key


def users_by_dense(U):
    """raw id of every dense index, for raw ids 1..U"""
    raw = np.arange(1, U + 1, dtype=np.int64)
    return raw[np.argsort(trie_keys(raw), kind="stable")]


def dense_of(U):
    """dense index of raw id r at [r] (cell 0 unused)"""
    out = np.zeros(U + 1, dtype=np.int64)
    out[users_by_dense(U)] = np.arange(U)
    return out


def head_items(train, head):
    """raw ids of the `head` dense columns: descending rater count, ties by dense item index (prep.hip: k_pop_keys + stable sort)"""
    items, counts = np.unique(train[1], return_counts=True)
    order = np.lexsort((trie_keys(items), -counts))
    return items[order[:head]]


@dataclass
class Case:
    train: tuple
    test: tuple
    num_users: int
    num_items: int
    groups: dict = field(default_factory=dict)  # population name -> raw user ids (int32), in planting order
    items: dict = field(default_factory=dict)   # planted item name -> raw item id(s)


class _Rows:
    def __init__(self):
        self.u, self.i, self.r, self.t = [], [], [], []

    def add(self, u, i, r, is_test):
        i = np.asarray(i, dtype=np.int64)
        self.u.append(np.broadcast_to(np.asarray(u, dtype=np.int64), i.shape).copy())
        self.i.append(i)
        self.r.append(np.broadcast_to(np.asarray(r, dtype=np.float64), i.shape).copy())
        self.t.append(np.broadcast_to(np.asarray(is_test, dtype=bool), i.shape).copy())

    def finish(self, rng, U, I, groups, items=None):
        u, i, r, t = (np.concatenate(x) for x in (self.u, self.i, self.r, self.t))
        keys = u * (1 << 32) + i
        assert len(np.unique(keys)) == len(keys), "a (user, item) pair twice"
        assert r.min() >= 1.0 and r.max() <= 5.0 and np.array_equal(2 * r, np.round(2 * r))
        assert np.array_equal(np.unique(u[~t]), np.arange(1, U + 1)), "raw user ids are not exactly 1..U"
        assert np.array_equal(np.unique(i[~t]), np.arange(1, I + 1)), "raw item ids are not exactly 1..I"
        assert np.isin(i[t], i[~t]).all()
        assert np.bincount(u[~t], minlength=U + 1)[1:].min() >= 5, "a user with fewer than 5 training ratings"
        lo, hi = np.full(U + 1, 9.0), np.zeros(U + 1)
        np.minimum.at(lo, u[~t], r[~t])
        np.maximum.at(hi, u[~t], r[~t])
        assert (lo[1:] < hi[1:]).all(), "a user whose training ratings are all equal"
        out = []
        for part in (~t, t):
            ix = rng.permutation(np.flatnonzero(part))
            out.append((u[ix].astype(np.int32), i[ix].astype(np.int32), r[ix].copy()))
        return Case(out[0], out[1], U, I, {g: np.asarray(v, dtype=np.int32) for g, v in groups.items()}, dict(items or {}))


def _half_stars(rng, n):
    return rng.integers(2, 11, n) / 2.0


def _varied(rng, n):
    """n half-star ratings that are not all equal"""
    r = _half_stars(rng, n)
    r[0], r[1] = 1.5, 4.5
    return r


def _zipf(rng, item_ids):
    """(cdf over popularity ranks, raw item id of every rank): shifted Zipf over a seeded permutation of item_ids"""
    w = 1.0 / (np.arange(len(item_ids), dtype=np.float64) + 10.0)
    cdf = np.cumsum(w / w.sum())
    cdf[-1] = 1.0
    return cdf, rng.permutation(np.asarray(item_ids, dtype=np.int64))


def _split_and_add(rows, rng, u, it, r):
    """five ratings of every user always train, the others test with probability 0.2"""
    order = np.lexsort((rng.random(len(u)), u))
    start = np.flatnonzero(np.concatenate([[True], u[order][1:] != u[order][:-1]]))
    rank = np.arange(len(u)) - np.repeat(start, np.diff(np.concatenate([start, [len(u)]])))
    is_test = np.zeros(len(u), dtype=bool)
    is_test[order] = (rank >= 5) & (rng.random(len(u)) < 0.2)
    # a user whose training ratings came out all equal (one in ~10^5) gets its first one moved by half a star
    lo, hi = np.full(int(u.max()) + 1, 9.0), np.zeros(int(u.max()) + 1)
    np.minimum.at(lo, u[~is_test], r[~is_test])
    np.maximum.at(hi, u[~is_test], r[~is_test])
    first = np.zeros(len(u), dtype=bool)
    first[order] = rank == 0
    fix = first & (lo[u] == hi[u])
    r = np.where(fix, np.where(r < 5.0, r + 0.5, r - 0.5), r)
    rows.add(u, it, r, is_test)


def _biased_ratings(rng, u, it, U, I):
    ub, ib = rng.normal(0.0, 0.45, U + 1), rng.normal(0.0, 0.45, I + 1)
    return np.clip(np.round(2.0 * (3.3 + ub[u] + ib[it] + rng.normal(0.0, 0.95, len(u)))) / 2.0, 1.0, 5.0)


def _background(rows, rng, users, cdf, item_of_rank, per_user, U, I):
    """ordinary users (raw ids): about per_user distinct items each by Zipf popularity, ratings from user and item biases"""
    users = np.asarray(users, dtype=np.int64)
    n_items = len(cdf)
    counts = np.clip(rng.lognormal(np.log(per_user) - 0.08, 0.4, len(users)), 9, max(9, n_items // 2)).astype(np.int64)
    u = np.repeat(users, counts + counts // 3 + 4)
    it = item_of_rank[np.minimum(np.searchsorted(cdf, rng.random(len(u))), n_items - 1)]
    key = np.unique(u * (1 << 32) + it)
    u, it = key >> 32, key & 0xFFFFFFFF
    _split_and_add(rows, rng, u, it, _biased_ratings(rng, u, it, U, I))


# ---- A, B, G: U around the 256-row tile; head widths around 64 and around I ---------------------------------------------------
def _private_dense(U, n):
    """dense indices of the n private users: both ends of the panel and both sides of every 256 edge that exists"""
    out = []
    for d in (0, U - 1, 255, 256, 254, 511, 512, 7, 100, 101, 102):
        if 0 <= d < U and d not in out:
            out.append(d)
    return out[:n]


def tile256(U, I=130, n_private=6, per_user=25, seed=0):
    """U users over I items.  n_private "private" users rate 5 items each that nobody else rates (the last 5 * n_private item
    ids): their similarity with everybody is exactly 0.0, cosine and Jaccard; their two test rows sit on popular items."""
    rng = np.random.Generator(np.random.PCG64(7000 + 31 * U + I + seed))
    order = users_by_dense(U)
    n_bg_items = I - 5 * n_private
    cdf, item_of_rank = _zipf(rng, np.arange(1, n_bg_items + 1))
    private = order[np.asarray(_private_dense(U, n_private), dtype=np.int64)]
    bg = np.setdiff1d(np.arange(1, U + 1), private)
    rows = _Rows()
    _background(rows, rng, bg, cdf, item_of_rank, per_user, U, I)
    own = {}
    for j, x in enumerate(private):
        own[int(x)] = n_bg_items + 1 + 5 * j + np.arange(5)
        rows.add(x, own[int(x)], np.roll([1.0, 5.0, 3.5, 2.0, 4.5], j), False)
        rows.add(x, item_of_rank[[2 * j, 2 * j + 1]], _half_stars(rng, 2), True)
    return rows.finish(rng, U, I, {"private": private, "background": bg},
                       {"private": own, "popular": item_of_rank[:6].copy()})


# ---- C, D: U around the 16 384-column tile and around 12 tiles ----------------------------------------------------------------
def tile16k(U, edge_dense, edge_items, I=400, per_user=16, seed=0):
    """U users over I items.  The users at the dense indices edge_dense (those below U) hold near-identical rows: the same 12
    items nobody else rates, one of the 12 ratings different for each, and the three most popular items.  edge_items maps a
    name to dense indices: one further item per name, rated by exactly the users at those indices that exist (dropped when
    none does) — edge users or background users, who get it on top of their row.  Planted items take the highest item ids."""
    rng = np.random.Generator(np.random.PCG64(9000 + U + seed))
    order = users_by_dense(U)
    edge_d = [d for d in dict.fromkeys(edge_dense) if d < U]
    edge = order[edge_d]
    raters = {name: [d for d in ds if d < U] for name, ds in edge_items.items()}
    raters = {name: ds for name, ds in raters.items() if ds}
    n_bg_items = I - 12 - len(raters)
    shared = n_bg_items + 1 + np.arange(12)
    item_id = {name: n_bg_items + 13 + j for j, name in enumerate(raters)}
    cdf, item_of_rank = _zipf(rng, np.arange(1, n_bg_items + 1))
    bg = np.setdiff1d(np.arange(1, U + 1), edge)
    rows = _Rows()
    _background(rows, rng, bg, cdf, item_of_rank, per_user, U, I)
    pattern = np.array([1.0, 5.0, 2.0, 4.5, 1.5, 4.0, 2.5, 5.0, 1.0, 3.5, 4.5, 2.0])
    for j, x in enumerate(edge):
        r = pattern.copy()
        r[j % 12] = 3.0  # (no entry of the pattern is 3.0)
        rows.add(x, shared, r, False)
        rows.add(x, item_of_rank[:3], [4.0, 2.5, 3.5], False)
        rows.add(x, item_of_rank[[3, 4]], _half_stars(rng, 2), True)
    extra = []
    for name, ds in raters.items():
        rows.add(order[ds], np.full(len(ds), item_id[name]), 3.0 + 0.5 * (np.arange(len(ds)) % 4), False)
        extra += [int(order[d]) for d in ds if d not in edge_d]
    return rows.finish(rng, U, I, {"edge": edge, "edge_item_raters": np.unique(np.asarray(extra, dtype=np.int64)), "background": bg},
                       {"shared": shared, "popular": item_of_rank[:6].copy(), **item_id})


C_EDGE = (0, 8191, 16382, 16383, 16384, 16385, 32767, 32768)  # + the last dense index, U - 1
C_ITEMS = {"pair": (16383, 16384),                   # the last cell of tile 0 and the first of tile 1
           "tile1": (16384, 16500, 20000, 32767),    # every rater in tile 1
           "tile2": (32768,)}                        # none in tile 0 or 1
D_EDGE = (0, 16383, 16384, 180223, 180224, 196607, 196608)
D_ITEMS = {"pair": (16383, 16384), "last": (180224, 196607, 196608)}  # tile 11, and tile 12 where it exists


def case_c(U):
    return tile16k(U, C_EDGE + (U - 1,), C_ITEMS)


def case_d(U):
    return tile16k(U, D_EDGE, D_ITEMS, per_user=10, seed=5)


def d_sample(c):
    """the 48 users of case D whose neighbourhoods are built: the edge users, the rest evenly spaced raw ids"""
    edge = c.groups["edge"].astype(np.int64)
    fill = np.setdiff1d(np.arange(1, c.num_users + 1, c.num_users // 60), edge)[:48 - len(edge)]
    return np.concatenate([edge, fill]).astype(np.int32)


def every(ids, step):
    """every step-th id of a population (the background may be sampled; planted rows never are)"""
    return np.asarray(ids)[::step]


# ---- E: tail entries per row around the 256-entry chunk ---------------------------------------------------------------------------
E_TAILS = (0, 1, 255, 256, 257, 511, 512, 513)
E_HOT = 64  # the items every background user rates 12 of: the head at head_items = 64


def emax_case(U, I=700, seed=0):
    """Items 1..64 are hot (every background user rates each with probability 12/64), items 65..I cold (15/636): at
    head_items = 64 the head is exactly the hot items.  One planted user per n of E_TAILS rates 10 hot items and exactly n cold
    ones; one more ("headless") rates 300 cold items and no hot one."""
    rng = np.random.Generator(np.random.PCG64(11000 + U + seed))
    n_planted = len(E_TAILS) + 1
    planted = np.sort(rng.choice(np.arange(1, U + 1), n_planted, replace=False))
    bg = np.setdiff1d(np.arange(1, U + 1), planted)
    p = np.concatenate([np.full(E_HOT, 12.0 / E_HOT), np.full(I - E_HOT, 15.0 / (I - E_HOT))])
    rows = _Rows()
    ui, ii = np.nonzero(rng.random((len(bg), I)) < p)
    u, it = bg[ui], ii.astype(np.int64) + 1
    _split_and_add(rows, rng, u, it, _biased_ratings(rng, u, it, U, I))
    hot, cold = np.arange(1, E_HOT + 1), np.arange(E_HOT + 1, I + 1)
    tails = {}
    for x, n in zip(planted, E_TAILS + (300,)):
        headless = x == planted[-1]
        mine = rng.permutation(hot)
        its = np.concatenate([mine[:0 if headless else 10], rng.choice(cold, n, replace=False)])
        rows.add(x, its, _varied(rng, len(its)), False)
        rows.add(x, mine[10:12], _half_stars(rng, 2), True)
        tails[int(x)] = (n, 0 if headless else 10)
    return rows.finish(rng, U, I, {"planted": planted, "background": bg}, {"entries": tails})


# ---- F: pieces per (chunk, tile) around the 1024-piece table ----------------------------------------------------------------------
def pmax_case(n_block_users, n_block_items, extra_rater=False, U=1000, seed=0):
    """Items 1..4 are hot (everybody rates each with probability 0.9: the head at head_items = 4), items 5..300 ordinary (a
    background user rates about 20), the n_block_items items above them are rated by all n_block_users block users and by nobody
    else — with extra_rater by one background user more, on the first block item.  groups["exact"] is the block user whose
    tail entries are exactly the block items; every second other block user rates three ordinary items as well."""
    rng = np.random.Generator(np.random.PCG64(13000 + n_block_users + seed))
    I = 300 + n_block_items
    block = np.sort(rng.choice(np.arange(1, U + 1), n_block_users, replace=False))
    bg = np.setdiff1d(np.arange(1, U + 1), block)
    block_items = 301 + np.arange(n_block_items)
    rows = _Rows()
    p = np.concatenate([np.full(4, 0.9), np.full(296, 20.0 / 296.0)])
    ui, ii = np.nonzero(rng.random((len(bg), 300)) < p)
    u, it = bg[ui], ii.astype(np.int64) + 1
    _split_and_add(rows, rng, u, it, _biased_ratings(rng, u, it, U, I))
    for j, x in enumerate(block):
        rows.add(x, block_items, _varied(rng, n_block_items), False)
        hot = np.flatnonzero(rng.random(4) < 0.9) + 1
        rows.add(x, hot, _half_stars(rng, len(hot)), False)
        ordinary = rng.permutation(np.arange(5, 301))
        if j > 0 and j % 2 == 0:
            rows.add(x, ordinary[:3], _half_stars(rng, 3), False)
        rows.add(x, ordinary[3:5], _half_stars(rng, 2), True)
    groups = {"block": block, "exact": block[:1], "background": bg}
    if extra_rater:
        groups["extra"] = bg[len(bg) // 2:len(bg) // 2 + 1]
        rows.add(groups["extra"][0], block_items[:1], 4.0, False)
    return rows.finish(rng, U, I, groups, {"block": block_items})


def pieces_per_chunk_and_tile(train, user, head):
    """k_tail_select's piece counts for the row of raw user `user`, mirrored from its setup (setup_a / setup_b): the row's tail
    entries (items outside the head) in position order — ascending dense item index — are cut into chunks of 256; for a
    chunk and a column tile, entry e contributes (cnt + 63) >> 6 pieces, cnt = the raters of e's item whose dense index lies
    in the tile (the row's own user included), and P is the sum over the chunk's entries.  Returns P as [chunk][tile]."""
    U = int(train[0].max())
    dense = dense_of(U)
    in_head = np.zeros(int(train[1].max()) + 1, dtype=bool)
    in_head[head_items(train, head)] = True
    mine = train[1][train[0] == user]
    tail = mine[~in_head[mine]]
    tail = tail[np.argsort(trie_keys(tail), kind="stable")]
    n_tiles = (U + TILE - 1) // TILE
    out = []
    for c0 in range(0, len(tail), 256):
        per_tile = []
        for t in range(n_tiles):
            P = 0
            for item in tail[c0:c0 + 256]:
                d = dense[train[0][train[1] == item]]
                cnt = int(((d >= t * TILE) & (d < (t + 1) * TILE)).sum())
                P += (cnt + 63) >> 6
            per_tile.append(P)
        out.append(per_tile)
    return out


# ---- the exact parameter sets of the two test files ---------------------------------------------------------------------------------
A_USERS = (255, 256, 257, 511, 512, 513)
C_USERS = (16383, 16384, 16385, 32768, 32769)
D_USERS = (196608, 196609)
E_USERS = (600, 16500)
CASES = {f"a{U}": functools.partial(tile256, U) for U in A_USERS}
CASES.update({"b_i64": functools.partial(tile256, 257, I=64, n_private=0, per_user=20),
              "b_i40": functools.partial(tile256, 257, I=40, n_private=0, per_user=14)})
CASES.update({f"c{U}": functools.partial(case_c, U) for U in C_USERS})
CASES.update({f"d{U}": functools.partial(case_d, U) for U in D_USERS})
CASES.update({f"e{U}": functools.partial(emax_case, U) for U in E_USERS})
CASES.update({"f1024": functools.partial(pmax_case, 256, 256), "f1025": functools.partial(pmax_case, 256, 256, extra_rater=True),
              "f_wide": functools.partial(pmax_case, 400, 260)})
SMALL_CASES = [n for n in CASES if n[0] not in "d"]  # (the ~2 M-rating D cases are built where they are needed only)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()
