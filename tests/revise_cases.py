"""Inputs of the revise-query tests (knncf_revise_*: a user of the fit who removed or re-rated items), shared by the premises
test (CPU, oracle only) and the GPU tests so that both speak about the same queries.  A query is (user, removed items,
additional items, additional ratings); aug = train without the user's rows on the removed items ++ the additional rows."""
import numpy as np

UNKNOWN_ITEM = 999_999
CASES = ("delete1", "delete3", "rerate", "mixed")


def aug_of(train, q, removed, items, ratings):
    """train in file order without q's rows on `removed`, then the additional rows"""
    u, i, r = train
    keep = ~((u == q) & np.isin(i, np.asarray(removed, dtype=np.int32)))
    n = len(items)
    return (np.concatenate([u[keep], np.full(n, q, dtype=np.int32)]).astype(np.int32),
            np.concatenate([i[keep], np.asarray(items, dtype=np.int32)]).astype(np.int32),
            np.concatenate([r[keep], np.asarray(ratings, dtype=np.float64)]))


def appended(train, q, items, ratings):
    """what an implementation that ignores the removals would answer on: train ++ the additional rows"""
    return aug_of(train, q, [], items, ratings)


def pick_users(train):
    """the shortest and the longest row, rows near 20 / 60 / 200 ratings, random ones: about a dozen"""
    u, c = np.unique(train[0], return_counts=True)
    order = np.argsort(c, kind="stable")
    picks = [int(u[order[0]]), int(u[order[-1]])]
    for target in (20, 60, 200):
        picks.append(int(u[np.argmin(np.abs(c - target))]))
    rng = np.random.default_rng(7)
    picks += [int(x) for x in rng.choice(u, 8, replace=False)]
    return list(dict.fromkeys(picks))


def syn100k(d, shuffled=False):
    """the plain file order, or a shuffled one with non-dyadic ratings: the mean's fold order (surviving train rows in FILE
    order, then the additional rows) shows in the last bits"""
    full = (d.train.users, d.train.items, d.train.ratings)
    if shuffled:
        order = np.random.default_rng(41).permutation(len(full[0]))
        u, i, r = (a[order] for a in full)
        full = (u, i, np.round(r * 0.93 + 0.1, 2))
    return full


def other_value(r, dyadic):
    """a rating different from r, for a re-rated item"""
    r = np.asarray(r, dtype=np.float64)
    return np.where(r >= 3, r - 2, r + 2) if dyadic else np.round(5.9 - r, 2)


def case_query(train, q, case, dyadic=True, unknown=False):
    """(removed, items, ratings) of user q for one of CASES; the picks depend on (q, case) only"""
    rng = np.random.default_rng([q, CASES.index(case)])
    at = np.flatnonzero(train[0] == q)
    mine, vals = train[1][at], train[2][at]
    none_i, none_r = np.empty(0, dtype=np.int32), np.empty(0)
    if case in ("delete1", "delete3"):
        pick = rng.choice(len(mine), int(case[-1]), replace=False)
        return mine[pick].astype(np.int32), none_i, none_r
    if case == "rerate":  # the same items removed and given again with other values
        pick = rng.choice(len(mine), 2, replace=False)
        return mine[pick].astype(np.int32), mine[pick].astype(np.int32), other_value(vals[pick], dyadic)
    # mixed: delete 2, re-rate 1, add 2 new items
    pick = rng.choice(len(mine), 3, replace=False)
    free = np.setdiff1d(np.unique(train[1]), mine)
    new = rng.choice(free, 2, replace=False).astype(np.int32)
    if unknown:
        new[1] = UNKNOWN_ITEM
    items = np.array([new[0], mine[pick[2]], new[1]], dtype=np.int32)
    ratings = np.array([4.0 if dyadic else 4.3, float(other_value(vals[pick[2]], dyadic)), 2.0 if dyadic else 1.7])
    return mine[pick].astype(np.int32), items, ratings


def pred_items(train, q, removed, items):
    """every train item, the removed items, the additional items, the user's train items, one unknown id"""
    return np.concatenate([np.unique(train[1]), removed, items, train[1][train[0] == q], [UNKNOWN_ITEM]]).astype(np.int32)


# ---- the hand set: 40 users x 30 items + one item that only user 20 rates -------------------------------------------------
LONE_USER, LONE_ITEM = 20, 31


def small_set(seed=3):
    """40 users x 30 items in shuffled file order, non-dyadic ratings; users 1..6 have 1..4 ratings, user 7 has 3, user 8 has
    6, user 9 has 4, the others 5..20; item 31 is rated by user 20 alone"""
    rng = np.random.default_rng(seed)
    sizes = {1: 1, 2: 2, 3: 3, 4: 4, 5: 4, 6: 2, 7: 3, 8: 6, 9: 4}
    us, its = [], []
    for u in range(1, 41):
        n = sizes.get(u, int(rng.integers(5, 21)))
        row = rng.choice(np.arange(1, 31, dtype=np.int32), n, replace=False)
        if u == LONE_USER:
            row = np.append(row, LONE_ITEM).astype(np.int32)
        its.append(row)
        us.append(np.full(len(row), u, dtype=np.int32))
    us, its = np.concatenate(us), np.concatenate(its)
    rts = np.round(rng.uniform(0.5, 5.0, len(us)), 1)
    order = rng.permutation(len(us))
    return us[order], its[order].astype(np.int32), rts[order]


def small_queries(train):
    """name -> (user, removed, items, ratings) on the hand set"""
    def row(q):
        at = np.flatnonzero(train[0] == q)
        return train[1][at].astype(np.int32), train[2][at]

    none_i, none_r = np.empty(0, dtype=np.int32), np.empty(0)
    out = {}
    m8, _ = row(8)  # 6 train rows: delete 4, add 2 -> 4 rows in aug (the <= 4 class), the two additional rows in both orders
    free8 = np.setdiff1d(np.arange(1, 31), m8)[:2].astype(np.int32)
    out["into_small_a"] = (8, m8[[0, 2, 3, 5]], free8, np.array([4.3, 1.7]))
    out["into_small_b"] = (8, m8[[0, 2, 3, 5]], free8[::-1].copy(), np.array([1.7, 4.3]))
    m7, _ = row(7)  # 3 train rows: delete 1, add 3 -> 5 rows (out of the <= 4 class)
    free7 = np.setdiff1d(np.arange(1, 31), m7)[:3].astype(np.int32)
    out["out_of_small"] = (7, m7[1:2], free7, np.array([3.9, 0.7, 2.2]))
    m9, _ = row(9)  # every train row removed, 2 new rows: still a user of aug
    free9 = np.setdiff1d(np.arange(1, 31), m9)[:2].astype(np.int32)
    out["all_removed"] = (9, m9, free9, np.array([2.1, 4.4]))
    out["lone_item_removed"] = (LONE_USER, np.array([LONE_ITEM], dtype=np.int32), none_i, none_r)
    out["lone_item_rerated"] = (LONE_USER, np.array([LONE_ITEM], dtype=np.int32), np.array([LONE_ITEM], dtype=np.int32),
                                np.array([1.3]))
    m30, v30 = row(30)  # a longer row: delete 2, re-rate 1, add 1
    free30 = np.setdiff1d(np.arange(1, 31), m30)[:1].astype(np.int32)
    out["long_row_mixed"] = (30, m30[:3], np.array([m30[2], free30[0]], dtype=np.int32), np.array([float(other_value(v30[2], False)), 3.3]))
    return out
