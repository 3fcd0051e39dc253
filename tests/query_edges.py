"""Deterministic fits and queries whose SHAPE sits on the fixed sizes of the query path (csrc/foldin.hip, csrc/qb_helpers.h,
csrc/bystander.hip; numpy only): the per-thread ranges of block_exclusive_scan over the neighbour count (A) and over the
bitmap words (B), the 32-bit half words of k_query_sim_dual (B), the 64-entry stripes of the similarity, gather and fold
kernels (C) and the 1 024-thread stride of k_qb_prep (D).  tests/test_query_edge_premises.py proves from numpy and the
oracle that every case is what it claims to be; tests/test_gpu_query_edges.py pins each of them to the oracle.

An item's DENSE index is its rank in HashSet iteration order (engine.h:49; boundary_shapes.trie_keys), NOT the rank of its
raw id: `by_dense(items)[d]` is the raw id at dense index d.  A train row is sorted by dense item, so the ROW POSITION of an
item is its rank among the user's items by dense index.  The kernels' constants are kept here as literals; the premise file
compares them with the sources' text."""
import functools

import numpy as np

from tests.boundary_shapes import trie_keys
from tests.query_helpers import UNKNOWN_ITEM

ONE_BLOCK = 1024       # qb_helpers.h:10  threads (and LDS cells) of block_exclusive_scan; per = ceil(m / ONE_BLOCK)
STRIPE = 64            # foldin.hip:93 k_query_sim, :453 k_query_sim_dual, :543 k_qb_gather, :1023 k_qb_self_sim, :1129 k_qb_fold_all
HALF_WORD = 32         # foldin.hip:459-461 k_query_sim_dual probes tb[c >> 5] with 1u << (c & 31); :421-423 k_qb_transpose
FA_AHEAD = 8           # foldin.hip:1102 similarity loads in flight per lane of k_qb_fold_all
QB_DUAL_MIN = 32       # engine.h:351 chunks of at least this many queries run k_query_sim_dual
QB_MAX_CHUNK = 64      # engine.h:350 queries per chunk
SIM_LDS_WORDS = 4096   # foldin.hip:54 k_query_sim holds the bitmap in LDS up to this many words
PREP_THREADS = 1024    # foldin.hip:362 k_qb_prep strides a slot's rows by blockDim.x = ONE_BLOCK
MAX_ROWS = 65536       # api.cpp:1055 QUERY_MAX_RATINGS

K_WIDE = 25            # the k of every query of groups B and D
BATCH = QB_DUAL_MIN + 1


def half_stars(rng, n):
    return rng.integers(2, 11, n).astype(np.float64) / 2


def by_dense(items):
    """the distinct raw ids of `items` in dense order"""
    ids = np.unique(items)
    return ids[np.argsort(trie_keys(ids), kind="stable")]


def dense_of(train_items, ids):
    """dense index of every id of `ids` (all of them train items)"""
    order = by_dense(train_items)
    by_id = np.argsort(order, kind="stable")
    return by_id[np.searchsorted(order[by_id], ids)]


def per_thread(m):
    """block_exclusive_scan: elements per thread"""
    return -(-m // ONE_BLOCK)


def block_scan(counts, per=None, advance=True):
    """block_exclusive_scan's index arithmetic on the host: thread t owns [t * per, t * per + per), sums it, takes the
    exclusive prefix of the threads' sums and writes its range from there; out[m] = the total.  Cells that no thread writes
    stay -1.  per / advance are the two ways to get it wrong that the premise file asks about: a floor instead of the
    ceiling, and a running sum that does not advance inside a range."""
    counts = np.asarray(counts, dtype=np.int64)
    m = len(counts)
    per = per_thread(m) if per is None else per
    lo = np.minimum(m, np.arange(ONE_BLOCK, dtype=np.int64) * per)
    hi = np.minimum(m, lo + per)
    part = np.array([counts[a:b].sum() for a, b in zip(lo, hi)], dtype=np.int64)
    start = np.cumsum(part) - part
    out = np.full(m + 1, -1, dtype=np.int64)
    for t in range(ONE_BLOCK):
        run = start[t]
        for i in range(lo[t], hi[t]):
            out[i] = run
            if advance:
                run += counts[i]
    out[m] = part.sum()
    return out


def tuple_key(oracle, q, item):
    """common.h tuple_trie_key: the order of k_qb_keys' sort inside a slot"""
    return oracle.trie_key(oracle.improve(oracle.tuple2_hash(int(q), int(item))))


# ---- A. the scan over take = min(k, U) ----------------------------------------------------------------------------------------
SCAN_KS = (1023, 1024, 1025, 2047, 2048, 2049, 2100, 3000)
SCAN_USERS, SCAN_ITEMS = 2100, 300
SCAN_Q = 99_999
SCAN_EXPLAIN_KS = (1025, 2049)
SCAN_UPDATE_KS = (1025, 2049, 2100)
SCAN_BATCH_KS = (1025, 2049)
SCAN_BYSTANDER_K = 1025
SCAN_NEWCOMER = 98_765   # the bystander case's newcomer


def scan_train(synth):
    t = synth.syn_scaled(SCAN_USERS, SCAN_ITEMS, 60_000, seed=5, half_stars=True).train
    return t.users, t.items, t.ratings


def scan_query(train):
    """user 99 999 on 40 train items, half stars from 1 to 5"""
    items = np.unique(train[1])[::5][:40].astype(np.int32)
    ratings = (np.arange(len(items)) * 4 % 9 + 2).astype(np.float64) / 2
    return SCAN_Q, items, ratings


def scan_pred_items(train):
    return np.concatenate([np.unique(train[1]), [UNKNOWN_ITEM]]).astype(np.int32)


def scan_update(train):
    """a fitted user with 2 additional rows on items it has not rated"""
    u = int(np.unique(train[0])[7])
    free = np.setdiff1d(np.unique(train[1]), train[1][train[0] == u])[:2].astype(np.int32)
    return u, free, np.array([4.5, 1.5])


def scan_batch(train):
    """33 copies of the fold-in query under different user ids: one chunk, 33 workgroups of the scan"""
    _, items, ratings = scan_query(train)
    return [(SCAN_Q + j, items, ratings) for j in range(BATCH)]


def scan_explain_items(train):
    return np.concatenate([np.unique(train[1])[3::31][:9], [UNKNOWN_ITEM]]).astype(np.int32)


# ---- B. the scan over W = ceil(I / 64) and the bitmap words ---------------------------------------------------------------------
WIDE_USERS = 400
WIDE_ITEMS = (65_472, 65_536, 65_537, 131_072, 131_073, 262_209)  # W = 1023, 1024, 1025, 2048, 2049, 4098
WIDE_BATCH_ITEMS = (65_537, 131_073, 262_209)                      # W = 1025, 2049, 4098: per = 2, 3, 5
WIDE_JACCARD_ITEMS = 65_537
ROWS_ITEMS = 65_536        # the fit of the "all" query and of group D
LONG_USER, LONG_ROWS = WIDE_USERS + 1, 1023  # group D's planted train user
WIDE_Q = 70_000


def wide_train(n_items, n_users=WIDE_USERS, long_row=0):
    """every item of 0 .. n_items-1 rated, so the dense item count is n_items exactly; (user, item) pairs distinct.
    long_row > 0 adds user n_users + 1 with exactly that many rows"""
    items = np.arange(n_items, dtype=np.int64)
    users = items % n_users
    extra = np.arange(30_000, dtype=np.int64)
    e_items = extra * 7 % n_items  # (extra * 7 itself from 209 994 items on)
    e_users = (e_items % n_users + 1 + extra % (n_users - 1)) % n_users
    u = np.concatenate([users, e_users]).astype(np.int32) + 1
    i = np.concatenate([items, e_items]).astype(np.int32)
    rng = np.random.default_rng(19)
    r = rng.integers(1, 11, len(u)).astype(np.float64) / 2
    order = rng.permutation(len(u))
    u, i, r = u[order], i[order], r[order]
    if long_row:
        rng = np.random.default_rng(31)
        li = rng.choice(n_items, long_row, replace=False).astype(np.int32)
        at = np.sort(rng.choice(len(u), long_row, replace=False))  # spread over the file
        u = np.insert(u, at, np.int32(n_users + 1))
        i = np.insert(i, at, li)
        r = np.insert(r, at, half_stars(rng, long_row))
    return u, i, r


@functools.lru_cache(maxsize=2)
def wide_fit(n_items):
    return wide_train(n_items, long_row=LONG_ROWS if n_items == ROWS_ITEMS else 0)


def n_words(n_items):
    return -(-n_items // 64)


def planted_dense(n_items):
    """the dense indices the "words" query knows: the ends of the first 64-bit words and of their 32-bit halves, both ends of
    the words on the two sides of the scan's thread ranges t = 511, 512, 1023 (words per * t - 1 | per * t, for per = 2 as
    the issue names them and for the fit's own per), the first bit of the last word and the last two items"""
    W = n_words(n_items)
    want = [0, 31, 32, 63, 64, 127, 128]
    for per in sorted({2, per_thread(W)}):
        for t in (511, 512, 1023):
            for w in (per * t - 1, per * t):
                want += [64 * w, 64 * w + 31, 64 * w + 32, 64 * w + 63]
    want += [64 * (W - 1), n_items - 2, n_items - 1]
    return np.array(sorted({d for d in want if 0 <= d < n_items}), dtype=np.int64)


def words_query(n_items, q=WIDE_Q):
    """(q, items, ratings): the planted dense indices and 200 random items, half stars; the first four rows are the dense
    indices 63, 31, 64, 32, not ascending"""
    order = by_dense(np.arange(n_items))
    planted = planted_dense(n_items)
    rng = np.random.default_rng(n_items)
    rest = rng.choice(np.setdiff1d(np.arange(n_items), planted), 200, replace=False)
    head = np.array([63, 31, 64, 32])
    dense = np.concatenate([head, rng.permutation(np.concatenate([np.setdiff1d(planted, head), rest]))])
    return q, order[dense].astype(np.int32), half_stars(rng, len(dense))


def words4_query(n_items, q=WIDE_Q + 1):
    _, items, ratings = words_query(n_items)
    return q, items[:4].copy(), np.array([4.5, 1.0, 3.5, 2.0])


def wide_pred_items(n_items):
    """the planted items, 500 random ones and an unknown one"""
    order = by_dense(np.arange(n_items))
    rng = np.random.default_rng(n_items + 1)
    return np.concatenate([order[planted_dense(n_items)], rng.choice(n_items, 500, replace=False), [n_items + 5]]).astype(np.int32)


def wide_batch(n_items):
    """33 queries: "words" in slot 0, its 4-row cut in slot 32, between them rows of 3, 30 and 200 random items that each
    know an item of the last bitmap word"""
    order = by_dense(np.arange(n_items))
    rng = np.random.default_rng(n_items + 2)
    queries = [words_query(n_items)]
    for j in range(1, BATCH - 1):
        m = (3, 30, 200)[j % 3]
        dense = rng.choice(n_items - 100, m, replace=False)
        dense[-1] = max(n_items - 1 - j, 64 * (n_words(n_items) - 1))  # (the last word may hold a single item)
        queries.append((WIDE_Q + 100 + j, order[dense].astype(np.int32), half_stars(rng, m)))
    queries.append(words4_query(n_items))
    return queries


def all_query(n_items=ROWS_ITEMS, q=WIDE_Q + 2):
    """every train item once, in a shuffled order: MAX_ROWS rows, every bitmap word all ones"""
    rng = np.random.default_rng(47)
    items = rng.permutation(n_items).astype(np.int32)
    return q, items, half_stars(rng, n_items)


# ---- C. the 64-entry stripes of a train row and of an item's raters (fit "R") ---------------------------------------------------
ROW_ITEMS = 260            # raw ids 1 .. 260
ROW_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 192, 193)
SMALL4_DENSE = (10, 80, 81, 150)     # at row positions 0, 63, 64, 128 of the user "spread"
SMALL4_GIVEN = (81, 150, 10, 80)     # the given order of "small4": not the dense order
SMALL5_EXTRA = 5
RATER_COUNTS = (7, 8, 9, 63, 64, 65)  # raters of the dense items 250 .. 255: around FA_AHEAD and around the stripe
COUNT_DENSE = tuple(range(250, 256))
ROW_K = 20
ROW_QUERIES = {"long": 9001, "small4": 9002, "small5": 9003}
ROW_OTHER_IDS = (9101, 9102, 9103)   # "long" under other ids, in the slots between the planted ones
ROW_RATINGS = {"small4": (4.3, 0.9, 2.6, 3.8)}  # one decimal: the premise file shows that the order of these four shows in the bits


def _one_decimal(rng, n):
    return rng.integers(6, 50, n).astype(np.float64) / 10


@functools.lru_cache(maxsize=1)
def row_fit():
    """(train, users: name -> raw user id, rows: name -> dense indices of the user's row, order: raw item id by dense index)"""
    order = by_dense(np.arange(1, ROW_ITEMS + 1))
    rng = np.random.default_rng(61)
    long_dense = np.arange(130)
    small = set(SMALL4_DENSE) | {SMALL5_EXTRA}
    low = np.array([d for d in range(0, 150) if d not in small])        # below small4's last item
    high = np.array([d for d in range(151, 250) if d not in small])     # above it, short of the counted items
    rows = {}
    for L in ROW_LENGTHS:
        # about three quarters of a row are items of "long" (at least one), the rest other items
        n_in = min(max(1, (3 * L) // 4), 130)
        n_in = max(n_in, L - 120)
        rows[f"len{L}"] = np.sort(np.concatenate([rng.choice(long_dense, n_in, replace=False),
                                                  rng.choice(np.arange(130, 250), L - n_in, replace=False)]))
    rows["full64"] = np.arange(64)
    rows["full64+1"] = np.arange(65)
    rows["full128"] = np.arange(128)
    rows["clone"] = np.arange(130)
    mid1 = rng.choice(np.arange(11, 80), 62, replace=False)
    mid2 = rng.choice(np.arange(82, 150), 63, replace=False)
    rows["spread"] = np.sort(np.concatenate([[10, 80, 81, 150], mid1, mid2]))
    last = SMALL4_DENSE[-1]
    for name, pos in (("at63", 63), ("at64", 64), ("atlast", 128)):
        rows[name] = np.sort(np.concatenate([rng.choice(low, pos, replace=False), [last], rng.choice(high, 128 - pos, replace=False)]))
    rows["none"] = np.sort(rng.choice(np.arange(151, 250), 10, replace=False))
    users = {name: 1 + n for n, name in enumerate(rows)}
    # fillers: 65 users of 6 random items each, the counted items on the first 7 .. 65 of them, then every item still without
    # a rater dealt round
    first = len(rows) + 1
    fillers = list(range(first, first + max(RATER_COUNTS)))
    fill = {u: set(rng.choice(250, 6, replace=False).tolist()) for u in fillers}
    for d, c in zip(COUNT_DENSE, RATER_COUNTS):
        for u in fillers[:c]:
            fill[u].add(d)
    rated = set(np.concatenate(list(rows.values())).tolist()) | set().union(*fill.values())
    for n, d in enumerate(sorted(set(range(ROW_ITEMS)) - rated)):
        fill[fillers[n % len(fillers)]].add(d)
    us, its = [], []
    for name, dense in rows.items():
        us += [users[name]] * len(dense)
        its += order[dense].tolist()
    for u in fillers:
        us += [u] * len(fill[u])
        its += order[sorted(fill[u])].tolist()
    us, its = np.array(us, dtype=np.int32), np.array(its, dtype=np.int32)
    rts = _one_decimal(rng, len(us))
    # the rows of 63, 64 and 65 entries follow "long" on their common items, so that they are near neighbours of it
    _, q_items, q_ratings = row_query("long", order)
    mine = dict(zip(q_items.tolist(), q_ratings.tolist()))
    for name in ("len63", "len64", "len65", "full64", "full64+1"):
        for j in np.flatnonzero(us == users[name]):
            if int(its[j]) in mine and j % 5:
                rts[j] = mine[int(its[j])]
    perm = rng.permutation(len(us))
    return (us[perm], its[perm], rts[perm]), users, rows, order


def row_query(name, order=None):
    """(q, items, ratings) of "long" (dense 0 .. 129, shuffled), "small4" (SMALL4_GIVEN) or "small5" (small4 and one more row)"""
    if order is None:
        order = row_fit()[3]
    if name == "long":
        rng = np.random.default_rng(67)
        dense = rng.permutation(130)
        return ROW_QUERIES[name], order[dense].astype(np.int32), _one_decimal(rng, 130)
    dense = np.array(SMALL4_GIVEN + ((SMALL5_EXTRA,) if name == "small5" else ()))
    ratings = np.array(ROW_RATINGS["small4"] + ((1.7,) if name == "small5" else ()))
    return ROW_QUERIES[name], order[dense].astype(np.int32), ratings


def row_batch33(name):
    """the planted query in slots 0, 1 and 32, "long" under other ids between them"""
    _, li, lr = row_query("long")
    queries = [(ROW_OTHER_IDS[j % 3], li, lr) for j in range(BATCH)]
    for slot in (0, 1, BATCH - 1):
        queries[slot] = row_query(name)
    return queries, (0, 1, BATCH - 1)


def row_batch64():
    """"small4" in slot 63 beside "long" in slot 62"""
    _, li, lr = row_query("long")
    queries = [(ROW_OTHER_IDS[j % 3], li, lr) for j in range(QB_MAX_CHUNK)]
    queries[62] = row_query("long")
    queries[63] = row_query("small4")
    return queries, (62, 63)


# ---- D. query row counts (on wide_fit(ROWS_ITEMS)) --------------------------------------------------------------------------------
ROW_COUNTS = (1, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049)
ROW_COUNTS_PERSONALIZED = (63, 64, 65, 1025)
NEW_ITEMS = 1_000_000
DUP_ROWS = 1100
DUP_Q = 80_000


def count_query(n, q=None):
    """n rows on train items apart from every 7th, which is on an unknown item"""
    rng = np.random.default_rng(1000 + n)
    items = rng.choice(ROWS_ITEMS, n, replace=False).astype(np.int32)
    items[6::7] = NEW_ITEMS + np.arange(len(items[6::7]), dtype=np.int32)
    return (71_000 + n if q is None else q), items, half_stars(rng, n)


def count_pred_items(items):
    rng = np.random.default_rng(len(items))
    return np.concatenate([items, rng.choice(ROWS_ITEMS, 200, replace=False)]).astype(np.int32)


def sorted_keys(oracle, q, items):
    """the slot's rows in the order of k_qb_keys' (stable) sort: (row indices, keys)"""
    keys = np.array([tuple_key(oracle, q, i) for i in items], dtype=np.int64)
    at = np.argsort(keys, kind="stable")
    return at, keys[at]


def duplicate_query(oracle, position):
    """1 100 rows on distinct train items and one more on the item at sorted position `position`: the equal keys sit at
    sorted positions position | position + 1"""
    rng = np.random.default_rng(83)
    items = rng.choice(ROWS_ITEMS, DUP_ROWS, replace=False).astype(np.int32)
    at, _ = sorted_keys(oracle, DUP_Q, items)
    twice = items[at[position]]
    return DUP_Q, np.append(items, twice).astype(np.int32), half_stars(rng, DUP_ROWS + 1)


def long_update(m):
    """the planted 1 023-row user with m additional rows: m - 1 on train items it has not rated and one on an unknown item"""
    train = wide_fit(ROWS_ITEMS)
    free = np.setdiff1d(np.arange(ROWS_ITEMS), train[1][train[0] == LONG_USER])
    items = np.concatenate([free[7::5000][:m - 1], [NEW_ITEMS]]).astype(np.int32)
    return LONG_USER, items, np.array([2.5, 4.0, 1.5])[:m]
