"""Deterministic rating sets whose SHAPE sits on the fixed sizes of the fit's set-up stage (prep.hip, sort_util.hip; numpy
only): the three size classes of the per-user LDS sorts and the fall-back to the global radix sorts (A), the 2 048-element
LDS chunks of k_ordered_fold under 256 user segments and 16 item segments per block (B), the 2 048-user scan tile and the
runs of equal users inside a wave (C), the radix sort's tiles, its self-scan limit and its pass count (D), the limits of the
direct id tables (E), and the fits small enough for Set1..Set4 / Map1..Map4 (F).  tests/test_setup_edge_premises.py proves
from the data (and the oracle) that every case is what it claims to be; tests/test_gpu_setup_edges.py pins each of them to
the oracle.  The kernels' constants are kept here as LITERALS; the premise file compares them with the sources' text.

Every builder returns a Case: train and test column triples (users int32, items int32, ratings float64), the raw ids of
the planted users and items, whether the planted users' neighbourhoods are compared (knn) and `facts`, the numbers the
premise file checks.  A user's DENSE index is the rank of its raw id in HashSet iteration order (boundary_shapes.trie_keys)
— first occurrence when the file holds at most four users — and an item's the rank of its trie key."""
import functools
from dataclasses import dataclass, field

import numpy as np

from tests.boundary_shapes import trie_keys

SEG_SHORT_CAP, SEG_MID_CAP, SEG_BLOCK_CAP = 512, 2048, 8192  # prep.hip: one wave / one 256-thread / one 512-thread workgroup
FOLD_CHUNK = 2048     # prep.hip k_ordered_fold: elements per LDS chunk, counted from the block's first element
FOLD_BATCH = 16       # k_ordered_fold FB: values per software-pipelined batch
USER_SPB, ITEM_SPB = 256, 16  # segments per block of the user folds (TPB) and of prep_item_stats
SCAN_TILE = 2048      # prep.hip SCAN_TILE = TPB * 8 users per block of k_user_tile_sums / k_user_ptr
TPB = 256
WAVE = 64
RS_TILE_U32, RS_TILE_U64 = 256 * 16, 256 * 12  # sort_util.hip RsTile: RS_THREADS * ITEMS keys per tile
RS_SELF_SCAN_TILES = 64
UQ_TILE = 2048
ID_LIMIT = 1 << 24
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
K = 10                # the neighbourhood size of every kNN comparison
PIECES = (15, 16, 17, 31, 32, 33)  # elements of a segment on one side of a chunk cut: around one and two fold batches


def bits_for(max_value):
    """common.h bits_for"""
    b = 1
    while b < 64 and (max_value >> b) != 0:
        b += 1
    return b


def user_order(users):
    """raw user ids in dense order: trie order, first occurrence up to four users (Set1..Set4)"""
    ids, first = np.unique(users, return_index=True)
    if len(ids) <= 4:
        return ids[np.argsort(first)]
    return ids[np.argsort(trie_keys(ids), kind="stable")]


def item_order(items):
    ids = np.unique(items)
    return ids[np.argsort(trie_keys(ids), kind="stable")]


def rank_of(order, ids):
    """dense index of every id of ids (all present in order)"""
    by_id = np.argsort(order, kind="stable")
    return by_id[np.searchsorted(order[by_id], ids)]


def canonical(train, users_in_order=None):
    """the file rows in canonical order: dense user, then dense item"""
    order = user_order(train[0]) if users_in_order is None else np.asarray(users_in_order)
    return np.lexsort((rank_of(item_order(train[1]), train[1]), rank_of(order, train[0])))


@dataclass
class Case:
    train: tuple
    test: tuple
    planted: np.ndarray                          # raw ids of the planted users, in planting order
    items: np.ndarray                            # raw ids of the planted items
    knn: bool = True                             # compare the neighbourhoods of the planted users with >= 5 ratings
    facts: dict = field(default_factory=dict)    # what the premise file checks


def ratings_of(rng, n, grid):
    """n ratings in [1, 5], not all equal from n = 2 on: half stars ("half") or hundredths ("off": sums depend on the order)"""
    if grid == "half":
        r = rng.integers(2, 11, n) / 2.0
        a, b = 1.5, 4.5
    else:
        r = np.round(rng.uniform(1.0, 5.0, n), 2)
        a, b = 1.37, 4.61
    if n >= 2:
        r[0], r[1] = a, b
    return r


def _assemble(rng, rows, grid, order="shuffle"):
    """rows: (raw user, train items, test items) per user run, in file order when order == "grouped".  A user's ratings
    are drawn per run; (user, item) pairs must be distinct over the whole case."""
    tu, ti, tr, su, si, sr = [], [], [], [], [], []
    for u, a, b in rows:
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
        r = ratings_of(rng, len(a) + len(b), grid)
        tu.append(np.full(len(a), u, dtype=np.int64)), ti.append(a), tr.append(r[:len(a)])
        su.append(np.full(len(b), u, dtype=np.int64)), si.append(b), sr.append(r[len(a):])
    tu, ti, tr, su, si, sr = (np.concatenate(x) for x in (tu, ti, tr, su, si, sr))
    pairs = np.concatenate([tu, su]) * (1 << 32) + (np.concatenate([ti, si]) & 0xFFFFFFFF)
    assert len(np.unique(pairs)) == len(pairs), "a (user, item) pair twice"
    if order == "shuffle":
        p = rng.permutation(len(tu))
        tu, ti, tr = tu[p], ti[p], tr[p]
    p = rng.permutation(len(su))
    return ((tu.astype(np.int32), ti.astype(np.int32), tr.copy()),
            (su[p].astype(np.int32), si[p].astype(np.int32), sr[p].copy()))


def lengths_of(train):
    """raw user id -> number of training rows"""
    ids, counts = np.unique(train[0], return_counts=True)
    return dict(zip(ids.tolist(), counts.tolist()))


# ---- A: row-length classes -------------------------------------------------------------------------------------------------------
A_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095,
             4096, 4097, 8191, 8192)
A_ITEMS = 9000
A_FIRST_ORDINARY = 101


def row_lengths(grid="half", beyond=False, seed=0):
    """one planted user (raw ids 1 .., in the order of A_LENGTHS) per training-row length of A_LENGTHS — with `beyond` one more
    of SEG_BLOCK_CAP + 1 — and 60 ordinary users of 30 - 90 ratings over 9 000 items, the training rows shuffled.  Train and
    test are built apart: the lengths are exact.  Users of >= 5 ratings have two test rows.  grid == "half": every sum of
    ratings is exact in any order (k_exact_sum, usersAvg folded in the canonical order) — the order-sensitivity premise
    holds for the norms only; "off": usersAvg folds along perm_uf."""
    rng = np.random.Generator(np.random.PCG64(21000 + seed + (7 if grid == "off" else 0) + (13 if beyond else 0)))
    lengths = A_LENGTHS + ((SEG_BLOCK_CAP + 1,) if beyond else ())
    rows = []
    for j, L in enumerate(lengths):
        its = rng.choice(A_ITEMS, L + (2 if L >= 5 else 0), replace=False) + 1
        rows.append((1 + j, its[:L], its[L:]))
    for j in range(60):
        L = int(rng.integers(30, 91))
        its = rng.choice(A_ITEMS, L + 2, replace=False) + 1
        rows.append((A_FIRST_ORDINARY + j, its[:L], its[L:]))
    train, test = _assemble(rng, rows, grid)
    planted = np.arange(1, len(lengths) + 1, dtype=np.int32)
    return Case(train, test, planted, np.empty(0, dtype=np.int32), True,
                {"lengths": dict(zip(planted.tolist(), lengths)),
                 "mid": sum(SEG_SHORT_CAP < L <= SEG_MID_CAP for L in lengths),
                 "long": sum(SEG_MID_CAP < L <= SEG_BLOCK_CAP for L in lengths)})


def with_duplicate(c, user):
    """the training rows of c plus one (user, item) pair of `user` a second time, with another rating, at a seeded row"""
    rng = np.random.Generator(np.random.PCG64(22000 + int(user)))
    u, i, r = c.train
    t = int(rng.choice(np.flatnonzero(u == user)))
    at = int(rng.integers(0, len(u) + 1))
    return (np.insert(u, at, u[t]), np.insert(i, at, i[t]), np.insert(r, at, 1.0 if r[t] > 3.0 else 5.0))


# ---- B: fold chunks ---------------------------------------------------------------------------------------------------------------
def _split(total, parts, least):
    """`parts` lengths of at least `least` that sum to total"""
    base, rem = divmod(total, parts)
    assert base >= least, (total, parts)
    return [base + (1 if j < rem else 0) for j in range(parts)]


def _block_plan(plan, tail, least=5):
    """segment lengths of one fold block.  plan: (cut index k, (left, right), fillers) in ascending k — `fillers` segments fill
    the gap up to FOLD_CHUNK * k - left, then one segment of left + right elements lies across the cut.  `tail` lengths follow.
    Returns (lengths, [(segment index in the block, k, left, right)])."""
    lengths, marks, pos = [], [], 0
    for k, (left, right), fillers in plan:
        gap = FOLD_CHUNK * k - left - pos
        lengths += _split(gap, fillers, least)
        marks.append((len(lengths), k, left, right))
        lengths.append(left + right)
        pos = FOLD_CHUNK * k + right
    return lengths + list(tail), marks


def _last_block_plan(fillers_a, fillers_b, tail_n):
    """a block whose segment `fillers_a - 1` ends exactly on the first cut and whose next one (40 elements) starts on it; after
    `fillers_b` more segments one of 2 048 + 2 048 + 1 starts on the second cut and ends one element into the fourth chunk"""
    lengths = _split(FOLD_CHUNK, fillers_a, 5) + [40] + _split(FOLD_CHUNK - 40, fillers_b, 5)
    ends_on, starts_on, spans = fillers_a - 1, fillers_a, len(lengths)
    lengths += [2 * FOLD_CHUNK + 1] + [30] * tail_n
    return lengths, {"ends_on_cut": ends_on, "starts_on_cut": starts_on, "three_chunks": spans}


B_USERS, B_USER_ITEMS = 600, 4500
_PAIRS = tuple(zip(PIECES, PIECES[::-1]))  # (left, right): both sides take every size of PIECES


def fold_users(seed=0):
    """600 users (raw ids 1..600) over 4 500 items, ratings off the grid, shuffled file.  The row lengths are assigned by
    DENSE index.  Block 0 (dense users 0..255) and block 1 (256..511) each hold six users whose segments lie across the cuts
    2 048 * 1 .. 6 of their block with _PAIRS' (left, right) elements on the two sides — block 1 with the pairs rotated by one, so
    that every pair meets a cut of either buffer parity; block 2 (512..599) holds _last_block_plan."""
    rng = np.random.Generator(np.random.PCG64(23000 + seed))
    raw = np.arange(1, B_USERS + 1, dtype=np.int64)
    by_dense = raw[np.argsort(trie_keys(raw), kind="stable")]
    lengths, straddlers = [], []
    for blk in range(2):
        pairs = _PAIRS[blk:] + _PAIRS[:blk]
        ls, marks = _block_plan([(k + 1, pairs[k], 40) for k in range(6)], [30] * 10)
        assert len(ls) == USER_SPB
        straddlers += [(blk * USER_SPB + s, k, left, right) for s, k, left, right in marks]
        lengths += ls
    ls, special = _last_block_plan(20, 15, B_USERS - 2 * USER_SPB - 37)
    lengths += ls
    assert len(lengths) == B_USERS
    special = {name: 2 * USER_SPB + s for name, s in special.items()}
    rows = []
    for d, L in enumerate(lengths):
        its = rng.choice(B_USER_ITEMS, L + 2, replace=False) + 1
        rows.append((int(by_dense[d]), its[:L], its[L:]))
    train, test = _assemble(rng, rows, "off")
    planted_dense = [s[0] for s in straddlers] + list(special.values())
    return Case(train, test, by_dense[planted_dense].astype(np.int32), np.empty(0, dtype=np.int32), True,
                {"side": "users", "spb": USER_SPB, "straddlers": straddlers, **special})


B_ITEM_USERS, B_ITEMS = 4200, 80


def fold_items(seed=0):
    """the same plan on the item side: 80 items (raw ids 1..80) in five blocks of 16 consecutive dense items, rated by 4 200
    users, ratings off the grid, shuffled file.  An item's segment is its raters; an item of c raters is rated by c consecutive
    users of a rotating window, so every user rates about ten items.  Blocks 0 and 1 put three pairs each across the cuts
    2 048 * 1 .. 3, blocks 2 and 3 the same pairs across the cuts 2 .. 4 (the other buffer parity); block 4 is _last_block_plan.
    One test row per item, by the user behind its window."""
    rng = np.random.Generator(np.random.PCG64(24000 + seed))
    raw = np.arange(1, B_ITEMS + 1, dtype=np.int64)
    by_dense = raw[np.argsort(trie_keys(raw), kind="stable")]
    lengths, straddlers = [], []
    for blk in range(4):
        pairs = _PAIRS[3 * (blk % 2):3 * (blk % 2) + 3]
        first = 1 + blk // 2
        plan = [(first + j, pairs[j], (4 if blk < 2 else 6) if j == 0 else (4 if blk < 2 else 2)) for j in range(3)]
        n_plan = sum(p[2] + 1 for p in plan)
        ls, marks = _block_plan(plan, [30] * (ITEM_SPB - n_plan), least=5)
        assert len(ls) == ITEM_SPB, (blk, len(ls))
        straddlers += [(blk * ITEM_SPB + s, k, left, right) for s, k, left, right in marks]
        lengths += ls
    ls, special = _last_block_plan(4, 4, ITEM_SPB - 10)
    lengths += ls
    assert len(lengths) == B_ITEMS and max(lengths) < B_ITEM_USERS
    special = {name: 4 * ITEM_SPB + s for name, s in special.items()}
    start, tu, ti, su, si = 0, [], [], [], []
    for d, c in enumerate(lengths):
        tu.append((start + np.arange(c)) % B_ITEM_USERS + 1)
        ti.append(np.full(c, by_dense[d]))
        su.append((start + c) % B_ITEM_USERS + 1)
        si.append(by_dense[d])
        start = (start + c + 131) % B_ITEM_USERS
    tu, ti = np.concatenate(tu), np.concatenate(ti)
    assert len(np.unique(tu)) == B_ITEM_USERS
    p = rng.permutation(len(tu))
    train = (tu[p].astype(np.int32), ti[p].astype(np.int32), ratings_of(rng, len(tu), "off"))
    test = (np.asarray(su, dtype=np.int32), np.asarray(si, dtype=np.int32), ratings_of(rng, len(su), "off"))
    planted_dense = [s[0] for s in straddlers] + list(special.values())
    some_users = user_order(train[0])[::350].astype(np.int32)
    return Case(train, test, some_users, by_dense[planted_dense].astype(np.int32), False,
                {"side": "items", "spb": ITEM_SPB, "straddlers": straddlers, **special})


def small_fit(U, I, per_user, grid="off", seed=0):
    """exactly U users (raw ids 1..U) and I items (1..I): every user rates min(per_user, I) items, every item is rated; one
    test row per user that has an unrated item left; shuffled"""
    rng = np.random.Generator(np.random.PCG64(25000 + 977 * U + 31 * I + seed))
    k = min(per_user, I)
    mine = [set((rng.choice(I, k, replace=False) + 1).tolist()) for _ in range(U)]
    rated = set().union(*mine)
    for j, item in enumerate(sorted(set(range(1, I + 1)) - rated)):
        mine[j % U].add(item)
    rows = []
    for u in range(U):
        a = rng.permutation(sorted(mine[u]))
        free = np.setdiff1d(np.arange(1, I + 1), a)
        rows.append((u + 1, a, rng.choice(free, 1) if len(free) else []))
    train, test = _assemble(rng, rows, grid)
    planted = user_order(train[0])[[0, U // 2, U - 1]] if U >= 3 else user_order(train[0])
    return Case(train, test, np.unique(planted).astype(np.int32), np.arange(1, I + 1, dtype=np.int32), k >= 5 and U >= 2,
                {"U": U, "I": I})


# ---- C: scan tiles and wave runs ------------------------------------------------------------------------------------------------
C_USERS = (1, 2047, 2048, 2049, 4096, 4097)


def scan_users(U, seed=0):
    """U users (raw ids 1..U) of 5 - 9 half-star ratings over 64 items, the users at dense index 0 and U - 1 of 12; the file
    is grouped by user in ascending raw id, as every MovieLens file is.  Planted: 12 users evenly spaced over the dense order,
    both ends among them; they and every 16th user have one test row."""
    rng = np.random.Generator(np.random.PCG64(26000 + U + seed))
    raw = np.arange(1, U + 1, dtype=np.int64)
    by_dense = raw[np.argsort(trie_keys(raw), kind="stable")]
    planted = by_dense[np.unique(np.linspace(0, U - 1, 12).astype(np.int64))]
    rows = []
    for u in raw:
        L = 12 if u in (by_dense[0], by_dense[-1]) else int(rng.integers(5, 10))
        t = 1 if (u % 16 == 0 or u in planted) else 0
        its = rng.choice(64, L + t, replace=False) + 1
        rows.append((int(u), its[:L], its[L:]))
    train, test = _assemble(rng, rows, "half", order="grouped")
    return Case(train, test, planted.astype(np.int32), np.empty(0, dtype=np.int32), True, {"U": U})


C_RUNS = (63, 64, 65, 128, 256)
C_OFFSETS = (0, 1, 63)
C_REMAINDERS = (0, 1, 63)


def wave_runs(remainder, seed=0):
    """a file grouped into RUNS of equal users over 700 items, half stars: one planted user per (run length of C_RUNS, row
    offset mod 64 of C_OFFSETS), its run starting at exactly that offset; one run of 100 rows from row 200 (mod 256), across a
    workgroup edge; one user with two runs of 10 rows inside one wave, another user's 5 rows between them; total rows = remainder
    (mod 64).  The rows between planted runs belong to eight filler users in runs of at most 6 rows, so every filler user
    owns many separate runs."""
    rng = np.random.Generator(np.random.PCG64(27000 + seed))  # (the three files differ in their last rows only)
    n_items = 700
    items_of, used, rows, pos = {}, {}, [], 0
    facts = {"runs": [], "remainder": remainder}

    def take(u, c):
        if u not in items_of:
            items_of[u], used[u] = rng.permutation(n_items) + 1, 0
        out = items_of[u][used[u]:used[u] + c]
        used[u] += c
        assert len(out) == c
        return out

    fill = [0]

    def pad(count):
        nonlocal pos
        while count > 0:
            c = min(count, 1 + fill[0] % 6)
            rows.append((900 + fill[0] % 8, take(900 + fill[0] % 8, c), []))
            fill[0] += 1
            count -= c
            pos += c

    def run(u, c, test=0):
        nonlocal pos
        its = take(u, c + test)
        rows.append((u, its[:c], its[c:]))
        facts["runs"].append((u, pos, c))
        pos += c

    user = 1
    for c in C_RUNS:
        for off in C_OFFSETS:
            pad((off - pos) % WAVE)
            run(user, c, test=2)
            user += 1
    pad((200 - pos) % TPB)
    facts["edge_user"] = user
    run(user, 100, test=2)
    pad((-pos) % WAVE)
    facts["twice_user"] = user + 1
    run(user + 1, 10, test=2)
    run(user + 2, 5, test=2)
    run(user + 1, 10)
    pad(64)
    pad((remainder - pos) % WAVE)
    train, test = _assemble(rng, rows, "half", order="grouped")
    assert len(train[0]) == pos
    return Case(train, test, np.arange(1, user + 3, dtype=np.int32), np.empty(0, dtype=np.int32), True, facts)


# ---- D: sort tiles and passes -----------------------------------------------------------------------------------------------------
D_USERS, D_ITEMS, D_TEST = 3000, 2000, 2000
D_SIZES = (3072, 3073, 4096, 4097, 196608, 196609, 262144, 262145)


def sort_tiles(n, seed=0):
    """n training ratings in distinct cells of a 3 000 x 2 000 grid, drawn without replacement, off the grid, in the order
    drawn; 2 000 test rows from other cells"""
    rng = np.random.Generator(np.random.PCG64(28000 + seed))  # (the same stream for every n: a longer file extends a shorter one)
    cells = rng.choice(D_USERS * D_ITEMS, D_SIZES[-1] + D_TEST, replace=False)
    r = np.round(rng.uniform(1.0, 5.0, len(cells)), 2)
    u, i = (cells // D_ITEMS + 1).astype(np.int32), (cells % D_ITEMS + 1).astype(np.int32)
    train = (u[:n].copy(), i[:n].copy(), r[:n].copy())
    test = (u[-D_TEST:].copy(), i[-D_TEST:].copy(), r[-D_TEST:].copy())
    ids, counts = np.unique(train[0], return_counts=True)
    planted = ids[np.argsort(-counts, kind="stable")[:6]]  # the six longest rows
    return Case(train, test, planted.astype(np.int32), np.unique(train[1]).astype(np.int32), False, {"n": n})


def pass_counts(U, I, seed=0):
    """exactly U users and I items, 20 000 ratings in distinct cells, off the grid; bits_for(255) = 8 and bits_for(256) = 9:
    the number of radix passes, and with it the buffer the first pass writes to, changes between them"""
    rng = np.random.Generator(np.random.PCG64(29000 + 1009 * U + I + seed))
    cells = rng.choice(U * I, 20_000 + 600, replace=False)
    r = np.round(rng.uniform(1.0, 5.0, len(cells)), 2)
    u, i = (cells // I + 1).astype(np.int32), (cells % I + 1).astype(np.int32)
    train = (u[:20_000].copy(), i[:20_000].copy(), r[:20_000].copy())
    test = (u[20_000:].copy(), i[20_000:].copy(), r[20_000:].copy())
    assert len(np.unique(train[0])) == U and len(np.unique(train[1])) == I
    planted = user_order(train[0])[[0, U // 2, U - 1]]
    return Case(train, test, planted.astype(np.int32), np.unique(train[1]).astype(np.int32), True, {"U": U, "I": I})


def unique_tiles(n, seed=0):
    """n ratings of 300 users x 120 items in distinct cells (half stars): with the id tables off, sort_keys_u32 and unique_u32
    run over n row keys — n = UQ_TILE and UQ_TILE + 1"""
    rng = np.random.Generator(np.random.PCG64(30000 + seed))
    cells = rng.choice(300 * 120, UQ_TILE + 1 + 300, replace=False)
    r = rng.integers(2, 11, len(cells)) / 2.0
    u, i = (cells // 120 + 1).astype(np.int32), (cells % 120 + 1).astype(np.int32)
    train = (u[:n].copy(), i[:n].copy(), r[:n].copy())
    test = (u[-300:].copy(), i[-300:].copy(), r[-300:].copy())
    planted = user_order(train[0])[[0, 150, -1]]
    return Case(train, test, planted.astype(np.int32), np.unique(train[1]).astype(np.int32), False, {"n": n})


# ---- E: ids -----------------------------------------------------------------------------------------------------------------------------
E_VARIANTS = ("zero", "table_max", "user_limit", "item_limit", "user_minus_one", "int32_ends")


def _remap(ids, mapping):
    out = np.asarray(ids, dtype=np.int64).copy()
    for old, new in mapping.items():
        out[np.asarray(ids) == old] = new
    return out


def ids_case(variant):
    """small_fit(300, 120, 30) on half stars with its ids moved: "zero" ids 0..299 / 0..119; "table_max" the largest user
    and item id at ID_LIMIT - 1 (the last cell of either direct table); "user_limit" / "item_limit" that id alone at ID_LIMIT
    (one past the tables: the general path); "user_minus_one" the smallest user id at -1; "int32_ends" the smallest and largest
    ids of both kinds at INT32_MIN and INT32_MAX.  The test rows are joined by rows of a negative id, of one beyond the tables
    and of an absent one inside them, on the user side and on the item side."""
    base = small_fit(300, 120, 30, grid="half", seed=99)
    umap, imap, shift = {}, {}, 0
    if variant == "zero":
        shift = -1
    elif variant == "table_max":
        umap, imap = {300: ID_LIMIT - 1}, {120: ID_LIMIT - 1}
    elif variant == "user_limit":
        umap = {300: ID_LIMIT}
    elif variant == "item_limit":
        imap = {120: ID_LIMIT}
    elif variant == "user_minus_one":
        umap = {1: -1}
    elif variant == "int32_ends":
        umap, imap = {1: INT32_MIN, 300: INT32_MAX}, {1: INT32_MIN, 120: INT32_MAX}
    else:
        raise KeyError(variant)
    mu = lambda a: (_remap(a, umap) + shift).astype(np.int32)
    mi = lambda a: (_remap(a, imap) + shift).astype(np.int32)
    train = (mu(base.train[0]), mi(base.train[1]), base.train[2])
    strangers = np.array([-7, ID_LIMIT + 5, 100_000], dtype=np.int32)  # negative, beyond the tables, absent
    known_u, known_i = train[0][:3], train[1][3:6]
    test = (np.concatenate([mu(base.test[0]), strangers, known_u, strangers[:1]]),
            np.concatenate([mi(base.test[1]), known_i, strangers, strangers[1:2]]),
            np.concatenate([base.test[2], np.full(7, 3.0)]))
    assert not np.isin(strangers, train[0]).any() and not np.isin(strangers, train[1]).any()
    return Case(train, test, mu(base.planted), np.unique(train[1])[::7].astype(np.int32), True,
                {"variant": variant, "table": variant in ("zero", "table_max"), "strangers": strangers})


# ---- F: tiny fits -----------------------------------------------------------------------------------------------------------------------
F_IDS = (7, 3, 9, 1, 5)
_CLONE = (np.arange(1, 7), np.array([1.0, 5.0, 2.0, 4.0, 3.0, 3.0]))  # mean 3: deviations -1, 1, -1/2, 1/2, 0, 0, exact squares


def tiny_users(U, second_order=False, seed=0):
    """users F_IDS[:U] with 6 half-star ratings each over 8 items and their 2 other items as test rows.  The file is grouped by
    user in F_IDS' order — with second_order in the reverse order, the users' rows interleaved.  Users 3 and 9 (from U = 3 on)
    are exact clones whose squared deviations sum exactly: every third user's similarity with them is one value, and the tie
    goes to the smaller dense index — 3 before 9 by first occurrence (9 before 3 with second_order), 9 before 3 in trie order."""
    rng = np.random.Generator(np.random.PCG64(31000 + seed))
    tu, ti, tr, su, si, sr = [], [], [], [], [], []
    for u in F_IDS[:U]:
        if u in (3, 9):
            its, r = _CLONE
            rest = np.array([7, 8])
        else:
            p = rng.permutation(8) + 1
            its, rest, r = p[:6], p[6:], ratings_of(rng, 6, "half")
        tu.append(np.full(6, u)), ti.append(its), tr.append(r)
        su.append(np.full(2, u)), si.append(rest), sr.append(ratings_of(rng, 2, "half"))
    tu, ti, tr = np.concatenate(tu), np.concatenate(ti), np.concatenate(tr)
    if second_order:  # row j of every user, users in reverse order
        p = np.arange(len(tu)).reshape(U, 6)[::-1].T.reshape(-1)
        tu, ti, tr = tu[p], ti[p], tr[p]
    train = (tu.astype(np.int32), ti.astype(np.int32), tr)
    test = (np.concatenate(su).astype(np.int32), np.concatenate(si).astype(np.int32), np.concatenate(sr))
    return Case(train, test, np.asarray(F_IDS[:U], dtype=np.int32), np.unique(train[1]), U >= 2,
                {"U": U, "second_order": second_order})


def tiny_rows(n):
    """the first n of five rows, ratings off the grid: user 7 rates items 3, 1, 4, 2 (neither ascending nor in HashMap order),
    then user 3 item 1.  Up to n = 4 the Map iterates in file order and perm_uh is not built."""
    u = np.array([7, 7, 7, 7, 3], dtype=np.int32)[:n]
    i = np.array([3, 1, 4, 2, 1], dtype=np.int32)[:n]
    r = np.array([1.59, 4.28, 3.73, 4.15, 2.21])[:n]  # (chosen so that the two orders of four squares sum to different bits)
    test = (np.array([7, 3, 99], dtype=np.int32), np.array([5, 2, 1], dtype=np.int32), np.array([3.0, 4.0, 2.0]))
    return Case((u, i, r), test, np.unique(u).astype(np.int32), np.unique(i).astype(np.int32), False, {"n": n})


def tiny_items(I, seed=0):
    """8 users who each rate every one of I items, off the grid, shuffled; the test rows name an unknown item and an unknown user"""
    rng = np.random.Generator(np.random.PCG64(32000 + I + seed))
    rows = [(u, rng.permutation(I) + 1, []) for u in range(1, 9)]
    train, _ = _assemble(rng, rows, "off")
    test = (np.array([1, 77, 8], dtype=np.int32), np.array([99, 1, I], dtype=np.int32), np.array([3.0, 4.0, 2.0]))
    return Case(train, test, np.array([1, 8], dtype=np.int32), np.arange(1, I + 1, dtype=np.int32), I >= 5, {"I": I})


# ---- the exact parameter sets of the two test files -----------------------------------------------------------------------------------
CASES = {"a_half": functools.partial(row_lengths, "half"), "a_off": functools.partial(row_lengths, "off"),
         "a_beyond": functools.partial(row_lengths, "off", beyond=True),
         "b_users": fold_users, "b_items": fold_items,
         "b_i16": functools.partial(small_fit, 300, 16, 8), "b_i17": functools.partial(small_fit, 300, 17, 8),
         "b_i1": functools.partial(small_fit, 40, 1, 1),
         "b_u256": functools.partial(small_fit, 256, 120, 20), "b_u257": functools.partial(small_fit, 257, 120, 20)}
CASES.update({f"c_u{U}": functools.partial(scan_users, U) for U in C_USERS})
CASES.update({f"c_runs{r}": functools.partial(wave_runs, r) for r in C_REMAINDERS})
CASES.update({f"d_n{n}": functools.partial(sort_tiles, n) for n in D_SIZES})
CASES.update({f"d_i{I}": functools.partial(pass_counts, 300, I) for I in (255, 256, 257)})
CASES.update({f"d_u{U}": functools.partial(pass_counts, U, 300) for U in (255, 256, 257)})
CASES.update({f"d_q{n}": functools.partial(unique_tiles, n) for n in (UQ_TILE, UQ_TILE + 1)})
CASES.update({f"e_{v}": functools.partial(ids_case, v) for v in E_VARIANTS})
CASES.update({f"f_u{U}": functools.partial(tiny_users, U) for U in (1, 2, 3, 4, 5)})
CASES.update({f"f_u{U}_second": functools.partial(tiny_users, U, True) for U in (4, 5)})
CASES.update({f"f_n{n}": functools.partial(tiny_rows, n) for n in (1, 2, 3, 4, 5)})
CASES.update({f"f_i{I}": functools.partial(tiny_items, I) for I in (1, 2, 3, 4, 5)})
A_DUPLICATES = {"a_off": (511, 512, 2047, 2048, 8191, 8192), "a_beyond": (8193,)}  # case -> training-row lengths of the users


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    for cols in (c.train, c.test):
        for a in cols:
            a.setflags(write=False)
    return c
