"""Deterministic rating sets and row batches whose SHAPE sits on the fixed sizes of the streamed Personalized predictor (numpy
only): the 8 192-column tile of k_ptiles / k_sim_rows, the 512 look-ahead registers and the 512-item chunk of k_sim_rows, the
64-rater trips and the 4 rows per workgroup of k_fold_rows, and the equal user blocks of plan_personal_rows.
tests/test_personalized_edge_premises.py proves from the data (and the oracle) that every case is what it claims to be and that
the slips it is planted against would show in the bits; tests/test_gpu_personalized_edges.py pins each case to the oracle.

Conventions are those of tests/boundary_shapes.py: raw user ids exactly 1..U, raw item ids exactly 1..I, half-star ratings,
every user with at least 5 training ratings that are not all equal, rows in a seeded shuffled file order.  A user's COLUMN is
its dense index (HashSet order: users_by_dense), and the items of a user's row are walked in ascending dense item index.

  S "stair"   1030 users x 1030 stair items, one tile: the user of dense rank a rates the stair items of dense rank b <= a, so
              user a has a + 1 items (511, 512, 513, 1024, 1025 all exist), item b has 1030 - b raters (1 .. 1030) and two users
              share min(a, b) + 1 items.  No user's mean lies on the half-star grid: every deviation, hence every product, is
              non-zero.  Stairs of 512 and 513 users put one seam of their own between them: no item, then one entry of one
              item, behind the 512 look-ahead registers.
  T "tiles"   tile16k at U = 8191 .. 16385: 1, 1, 2, 2 and 3 tiles, the last one a single column at 8193 and 16385; planted items
              with raters on both sides of a seam, with no rater in tile 0, and with 511 | 512 | 512+1 | 512+513 raters per tile.
  B "blocks"  a batch on S whose 13 users with a similarity row are cut into 13, 7, 3, 3, 2, 1 and 1 blocks, with rows that
              own no similarity row before the first block, at block seams and last."""
import functools
from dataclasses import dataclass

import numpy as np

from tests.boundary_shapes import _half_stars, _Rows, dense_of, tile16k, trie_keys, users_by_dense

# the kernels' fixed sizes (the premise file holds them against the text of the sources)
PTC = 8192        # PERSONAL_TCOLS: columns per tile
ROW_TPB = 512     # raters of an item that come from the look-ahead registers
ROW_CHUNK = 512   # items of a user staged at a time
FOLD_TRIP = 64    # raters per trip of k_fold_rows
FOLD_WAVES = 4    # rows per workgroup of k_fold_rows
ABSENT_USER, ABSENT_ITEM = 987_654, 876_543
MAE_TOL = 1e-9


@dataclass
class Batch:
    users: np.ndarray    # int32 raw ids
    items: np.ndarray    # int32 raw ids
    ratings: np.ndarray  # float64 (what the MAE is taken against)

    def __len__(self):
        return len(self.users)

    def take(self, ix):
        return Batch(self.users[ix], self.items[ix], self.ratings[ix])

    def shuffled(self, seed):
        """(the batch in a seeded shuffled order, the permutation)"""
        perm = np.random.default_rng(seed).permutation(len(self))
        return self.take(perm), perm

    def by_user(self):
        """sorted by raw user id, stable (the oracle keeps one similarity row per run of a user)"""
        return self.take(np.argsort(self.users, kind="stable"))


def _batch(u, i, seed):
    u, i = np.asarray(u, dtype=np.int32), np.asarray(i, dtype=np.int32)
    return Batch(u, i, _half_stars(np.random.default_rng(seed), len(u)))


def items_by_dense(ids):
    """raw item ids in ascending dense item index"""
    ids = np.asarray(ids, dtype=np.int64)
    return ids[np.argsort(trie_keys(ids), kind="stable")]


# ---- S: the stair -----------------------------------------------------------------------------------------------------------------
STAIR_N = 1030
STAIR_RATER_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 511, 512, 513, 1023, 1024, 1025, 1030)
STAIR_USER_RANKS = (5, 62, 63, 64, 510, 511, 512, 513, 1022, 1023, 1024, 1025, 1029)
# A fold in another order moves the last bits of num and den, and only one such move in six or so survives the division and the
# addition to the user's mean: 13 rows per item would leave some items' folds unwitnessed.  These 50 users more make 63.
STAIR_WITNESS_RANKS = tuple(range(16, 1000, 20))
# the ids of the GPU test: seam group -> the item counts of the users (chunk) or the rater counts of the items (pass, fold)
STAIR_GROUPS = {"chunk": (511, 512, 513, 1024, 1025), "pass": (511, 512, 513, 1023, 1024, 1025, 1030),
                "fold": (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)}


@functools.lru_cache(maxsize=None)
def stair(N=STAIR_N):
    """Case S.  groups["by_rank"][a] is the raw id of the user of dense rank a, items["stair"][b] the raw id of the stair item of
    dense rank b (raw ids 1..N; the five extra items N+1..N+5 give the ranks 0..4 five varied ratings more)"""
    rng = np.random.Generator(np.random.PCG64(17000 + N))
    by_rank = users_by_dense(N)
    stair_items = items_by_dense(np.arange(1, N + 1))
    extra = N + 1 + np.arange(5)
    a, b = np.tril_indices(N)  # every (a, b) with b <= a
    r = _half_stars(rng, len(a))
    # a mean on the half-star grid would make the deviation of every rating equal to it 0.0: half a star on one rating moves
    # 2 * sum by one, off the multiples of the count
    count = np.bincount(a, minlength=N) + np.where(np.arange(N) < 5, 5, 0)
    twice = np.round(2.0 * np.bincount(a, weights=r, minlength=N)).astype(np.int64) + np.where(np.arange(N) < 5, 32, 0)
    first = np.concatenate([[0], np.cumsum(np.arange(1, N))])  # the place of (a, 0) in the triangle
    on_grid = np.flatnonzero(twice % count == 0)
    r[first[on_grid]] = np.where(r[first[on_grid]] < 5.0, r[first[on_grid]] + 0.5, r[first[on_grid]] - 0.5)
    rows = _Rows()
    rows.add(by_rank[a], stair_items[b], r, False)
    for rank in range(5):
        rows.add(by_rank[rank], extra, np.roll([1.0, 5.0, 3.5, 2.0, 4.5], rank), False)  # (sum 16.0)
    return rows.finish(rng, N, N + 5, {"by_rank": by_rank}, {"stair": stair_items, "extra": extra})


def stair_item_with(n_raters, N=STAIR_N):
    """the raw id of the stair item that exactly n_raters users rate"""
    return int(stair(N).items["stair"][N - n_raters])


def stair_user_with(n_items, N=STAIR_N):
    """the raw id of the user that rates exactly n_items items (rank >= 5: stair items only)"""
    assert n_items > 5
    return int(stair(N).groups["by_rank"][n_items - 1])


@functools.lru_cache(maxsize=None)
def stair_batch():
    """every user of STAIR_USER_RANKS and STAIR_WITNESS_RANKS on the item of every rater count of STAIR_RATER_COUNTS (a training
    pair wherever the user's rank reaches the item's), a row of an unknown user and a row on an unknown item; sorted by user"""
    c = stair()
    users = c.groups["by_rank"][list(STAIR_USER_RANKS + STAIR_WITNESS_RANKS)]
    items = np.array([stair_item_with(n) for n in STAIR_RATER_COUNTS])
    u = np.concatenate([np.repeat(users, len(items)), [ABSENT_USER, users[3]]])
    i = np.concatenate([np.tile(items, len(users)), [items[0], ABSENT_ITEM]])
    return _batch(u, i, 171).by_user()


def stair_group_rows(batch, group, size):
    """the rows of a stair batch that belong to one id of STAIR_GROUPS"""
    if group == "chunk":
        return np.flatnonzero(batch.users == stair_user_with(size))
    return np.flatnonzero((batch.items == stair_item_with(size)) & (batch.users != ABSENT_USER))


# Every user of S rates the first stair item, whose 1030 raters reach into the second loop of k_sim_rows, so no cosine row of S
# is built by the look-ahead registers alone.  Two short stairs put that seam between them: at 512 users no item has more
# raters than the registers hold, at 513 the first item has exactly one more — the 513th rater, the user of rank 512.
SHORT_STAIRS = (512, 513)
SHORT_RATER_COUNTS = (1, 2, 65, 129, 511, 512, 513)
SHORT_USER_RANKS = (5, 63, 64, 255, 256, 509, 510, 511, 512)


@functools.lru_cache(maxsize=None)
def short_stair_batch(N):
    """the users of SHORT_USER_RANKS on the items of SHORT_RATER_COUNTS that a stair of N users has, a row of an unknown user
    and a row on an unknown item; sorted by user"""
    c = stair(N)
    users = c.groups["by_rank"][[a for a in SHORT_USER_RANKS if a < N]]
    items = np.array([stair_item_with(n, N) for n in SHORT_RATER_COUNTS if n <= N])
    u = np.concatenate([np.repeat(users, len(items)), [ABSENT_USER, users[3]]])
    i = np.concatenate([np.tile(items, len(users)), [items[0], ABSENT_ITEM]])
    return _batch(u, i, 571 + N).by_user()


# ---- T: the tiles -----------------------------------------------------------------------------------------------------------------
TILE_USERS = (8191, 8192, 8193, 16384, 16385)
TILE_COUNTS = {8191: 1, 8192: 1, 8193: 2, 16384: 2, 16385: 3}
T_EDGE = (0, 8190, 8191, 8192, 8193, 16383, 16384)  # + the last dense index, U - 1
T_ITEMS = {"pair": (8191, 8192),                    # the last column of tile 0 and the first of tile 1
           "tile1": (8192, 9000, 12000, 16383),     # no rater in tile 0
           "tile2": (16384,),                       # none in tile 0 or 1
           "wide": range(7680, 8705),               # 512 raters at the end of tile 0 and 513 at the start of tile 1
           "low": (0, 5, 8191)}
T_WIDE_PER_TILE = {8191: (511,), 8192: (512,), 8193: (512, 1), 16384: (512, 513), 16385: (512, 513, 0)}
T_BACKGROUND_DENSE = (7680, 7681, 8191)  # raters of "wide" that are (where 8191 is no edge user's place) ordinary users


@functools.lru_cache(maxsize=2)
def tiles(U):
    """Case T at U users"""
    return tile16k(U, T_EDGE + (U - 1,), T_ITEMS, I=400, per_user=16)


def planted_names(c):
    return [name for name in T_ITEMS if name in c.items]


def per_tile_counts(c, item):
    """raters of a raw item id per column tile, from the dense indices of the raters' raw ids"""
    d = dense_of(c.num_users)[c.train[0][c.train[1] == item]]
    return tuple(np.bincount(d // PTC, minlength=-(-c.num_users // PTC)).tolist())


def tile_query_users(c):
    """raw ids: every edge user, the users at T_BACKGROUND_DENSE, and the first ordinary user (by dense index) that rates no
    planted item"""
    order = users_by_dense(c.num_users)
    planted = set(c.groups["edge"].tolist()) | set(c.groups["edge_item_raters"].tolist())
    plain = next(int(x) for x in order if int(x) not in planted)
    out = c.groups["edge"].tolist() + [int(order[d]) for d in T_BACKGROUND_DENSE if d < c.num_users] + [plain]
    return np.array(list(dict.fromkeys(out)), dtype=np.int32), plain


@functools.lru_cache(maxsize=2)
def tile_batch(U):
    """every query user on every planted item that exists, on two of the 12 shared items (every edge user rates them: the fold
    gathers the similarity row at the columns 0, 8190 .. 8193, 16383, 16384 and U - 1 that exist) and on two popular items; a
    row of an unknown user and a row on an unknown item; sorted by user.  The edge users' rows on the shared, the planted and
    the first popular item are training pairs."""
    c = tiles(U)
    users, _ = tile_query_users(c)
    items = np.array([c.items[name] for name in planted_names(c)] + [c.items["shared"][0], c.items["shared"][7],
                                                                      c.items["popular"][0], c.items["popular"][5]])
    u = np.concatenate([np.repeat(users, len(items)), [ABSENT_USER, users[1]]])
    i = np.concatenate([np.tile(items, len(users)), [items[0], ABSENT_ITEM]])
    return _batch(u, i, 271 + U).by_user()


# ---- B: the blocks ----------------------------------------------------------------------------------------------------------------
BLOCK_USER_RANKS = (5, 62, 64, 129, 510, 512, 640, 768, 1020, 1022, 1025, 1026, 1027)  # the 13 users that own a similarity row
BLOCK_ROWLESS_RANKS = (2, 511, 700, 1023, 1029)  # rows on unknown items only: before the first user, between the 5th and the 6th,
#                                                  the 7th and the 8th, the 10th and the 11th, and after the last
BLOCK_REQUESTS = (1, 2, 5, 6, 12, 13, 100)
BLOCK_USERS_PER_LAUNCH = {1: [1] * 13, 2: [2] * 6 + [1], 5: [5, 5, 3], 6: [5, 5, 3], 12: [7, 6], 13: [13], 100: [13]}


def workspace_for(R, U):
    """the workspace_bytes at which include/knncf.h's rule asks for R rows of U doubles: budget = workspace_bytes / 2,
    R = budget / (8 U)"""
    return 2 * (8 * U * R)


def rows_asked(workspace_bytes, U):
    return max(1, (workspace_bytes // 2) // (8 * U))


def equal_blocks(nu, asked):
    """users per launch for nu users at `asked` rows: R = min(asked, nu) equalised to ceil(nu / ceil(nu / R))"""
    R = min(max(1, asked), nu)
    R = -(-nu // -(-nu // R))
    return [min(R, nu - b) for b in range(0, nu, R)]


def block_fold_rows(train, batch, users_per_launch):
    """rows per fold launch: the rows sorted by (dense user, dense item), what the train set lacks last; block b runs from its
    first user's first row (block 0: from row 0) to the next block's (the last block: to the end), so a row that owns no
    similarity row is folded where it sorts"""
    U, I = int(train[0].max()), int(train[1].max())
    known_u, known_i = (batch.users >= 1) & (batch.users <= U), (batch.items >= 1) & (batch.items <= I)
    du = np.where(known_u, dense_of(U)[np.where(known_u, batch.users, 1)], U)
    item_rank = np.zeros(I + 1, dtype=np.int64)
    item_rank[items_by_dense(np.arange(1, I + 1))] = np.arange(I)
    di = np.where(known_i, item_rank[np.where(known_i, batch.items, 1)], I)
    order = np.lexsort((di, du))
    du, di = du[order], di[order]
    owned = np.flatnonzero((du < U) & (di < I))  # rows of a known user on a known item
    first = owned[np.unique(du[owned], return_index=True)[1]]  # where each such user's rows begin
    cuts = [0] + [int(first[k]) for k in np.cumsum(users_per_launch)[:-1]] + [len(batch)]
    assert len(first) == sum(users_per_launch)
    return np.diff(cuts).tolist()


@functools.lru_cache(maxsize=None)
def block_batch():
    """Case B on the stair: the 13 users of BLOCK_USER_RANKS on three known items each (those with 65, 513 and 1025 raters) and
    on an unknown one, the users of BLOCK_ROWLESS_RANKS on unknown items only (two rows each), two unknown users, the rows of
    the first three users once more, all in a seeded shuffled order"""
    by_rank = stair().groups["by_rank"]
    users, rowless = by_rank[list(BLOCK_USER_RANKS)], by_rank[list(BLOCK_ROWLESS_RANKS)]
    items = np.array([stair_item_with(n) for n in (65, 513, 1025)] + [ABSENT_ITEM])
    u = np.concatenate([np.repeat(users, 4), np.repeat(rowless, 2), [ABSENT_USER, ABSENT_USER + 1], np.repeat(users[:3], 4)])
    i = np.concatenate([np.tile(items, 13), np.tile([ABSENT_ITEM, ABSENT_ITEM + 1], len(rowless)), [items[0], ABSENT_ITEM],
                        np.tile(items, 3)])
    return _batch(u, i, 371).shuffled(372)[0]


ROW_COUNTS = (1, 3, 4, 5, 9)


def count_batch(n):
    """the first n of nine rows on the stair: long and short folds, a training pair, an unknown user and an unknown item among
    them, so that the waves of the last workgroup differ in what they do"""
    rank = stair().groups["by_rank"]
    rows = [(rank[513], 1025), (rank[64], 65), (ABSENT_USER, 1030), (rank[1029], 193), (rank[5], None), (rank[512], 1),
            (rank[1024], 513), (rank[63], 1030), (rank[511], 129)]
    assert 1 <= n <= len(rows)
    u = [int(x) for x, _ in rows[:n]]
    i = [ABSENT_ITEM if m is None else stair_item_with(m) for _, m in rows[:n]]
    return _batch(u, i, 471)


# ---- the kernels' arithmetic on the host, for the premises ------------------------------------------------------------------------
class RowModel:
    """k_sim_rows and k_fold_rows as numpy walks over the training file, the oracle's per-row preprocessed ratings (`pre`) and
    normalized deviations (`dev`): the cosine row of a user by item (ascending dense item index; the raters of an item in
    ascending dense user index, tile by tile), and the file-order folds of a test row.  The keyword arguments of cosine_row are
    the slips the cases are planted against; with none of them the row IS the oracle's (the premise file compares)."""

    def __init__(self, train, pre, dev):
        self.users, self.items = np.asarray(train[0], dtype=np.int64), np.asarray(train[1], dtype=np.int64)
        self.pre, self.dev = np.asarray(pre, dtype=np.float64), np.asarray(dev, dtype=np.float64)
        self.U = int(self.users.max())
        self.dense = dense_of(self.U)
        ikey = trie_keys(self.items).astype(np.int64)
        d = self.dense[self.users]
        by_item = np.lexsort((d, ikey))  # (item, rater ascending): it_user / pi_pre
        cut = np.flatnonzero(np.concatenate([[True], ikey[by_item][1:] != ikey[by_item][:-1], [True]]))
        self.item_entries = {int(self.items[by_item[a]]): by_item[a:b] for a, b in zip(cut[:-1], cut[1:])}
        by_user = np.lexsort((ikey, d))  # (user, item ascending): the user's row
        cut = np.flatnonzero(np.concatenate([[True], d[by_user][1:] != d[by_user][:-1], [True]]))
        self.user_entries = {int(self.users[by_user[a]]): by_user[a:b] for a, b in zip(cut[:-1], cut[1:])}
        in_file = np.argsort(self.items, kind="stable")  # (item, file row): pf_user / pf_dev
        ids, start = np.unique(self.items[in_file], return_index=True)
        self.file_rows = {int(i): in_file[a:b] for i, a, b in zip(ids, start, np.append(start[1:], len(in_file)))}

    def cosine_row(self, u, second_pass_from=ROW_TPB, chunk_items=ROW_CHUNK, last_column=True):
        """acc[column] of raw user u.  second_pass_from = 2 * ROW_TPB: the raters 513 .. 1024 of an item inside a tile are
        never added; chunk_items = ROW_CHUNK - 1: the last item of every full chunk is never staged; last_column = False: the
        cell of dense index U - 1 is never written (left at 0.0 here)"""
        acc = np.zeros(self.U)
        mine = self.user_entries[int(u)]
        for k, e in enumerate(mine.tolist()):
            if k % ROW_CHUNK >= chunk_items:
                continue
            entries = self.item_entries[int(self.items[e])]
            cols = self.dense[self.users[entries]]
            place = np.arange(len(cols)) - np.searchsorted(cols, (cols // PTC) * PTC)  # the rater's place in its tile's part
            keep = (place < ROW_TPB) | (place >= second_pass_from)
            acc[cols[keep]] = acc[cols[keep]] + self.pre[e] * self.pre[entries[keep]]  # (distinct raters: no collision)
        if not last_column:
            acc[self.U - 1] = 0.0
        return acc

    def raters(self, item):
        """(raw ids, deviations) of the item's raters in file order"""
        rows = self.file_rows.get(int(item), np.empty(0, dtype=np.int64))
        return self.users[rows], self.dev[rows]

    @staticmethod
    def fold(sims, devs):
        """k_fold_rows' two left folds from +0.0 over every rater, zero similarities included"""
        num, den = 0.0, 0.0
        for s, d in zip(np.asarray(sims, dtype=np.float64).tolist(), np.asarray(devs, dtype=np.float64).tolist()):
            num = num + d * s
            den = den + abs(s)
        return num, den


def trips_reversed(x):
    """the raters of every trip of 64 in reverse: a fold that runs each trip from its last rater down"""
    x = np.asarray(x)
    return np.concatenate([x[p:p + FOLD_TRIP][::-1] for p in range(0, len(x), FOLD_TRIP)]) if len(x) else x


def late_refill_ids(sims):
    """the similarities a fold gathers when the rater ids two trips ahead are refilled only where a THIRD trip ahead exists
    for the lane: from the third trip on, the rater at place p with p + 64 >= n is answered with the similarity of the rater
    whose id the lane still holds, the one at p - 64 (or further back, by the same rule)"""
    n = len(sims)
    out = np.array(sims, dtype=np.float64)
    for p in range(2 * FOLD_TRIP, n):
        q = p
        while q >= 2 * FOLD_TRIP and q + FOLD_TRIP >= n:
            q -= FOLD_TRIP
        out[p] = sims[q]
    return out


def previous_trip_ids(sims, places=(FOLD_TRIP, 2 * FOLD_TRIP)):
    """the 65th and the 129th rater answered with the similarity of the rater one trip before"""
    out = np.array(sims, dtype=np.float64)
    for p in places:
        if p < len(out):
            out[p] = sims[p - FOLD_TRIP]
    return out
