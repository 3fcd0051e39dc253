"""Inputs of the Personalized query tests (KNNCF_PRED_PERSONALIZED on knncf_query_* / knncf_update_* / knncf_revise_*), shared
by the premises test (CPU, oracle only) and the GPU tests so that both speak about the same queries.  A query is (user, removed
items, additional items, additional ratings): no removals make it an update query, a user absent from train a fold-in query.
aug = train without the user's rows on the removed items ++ the additional rows (tests/revise_cases.aug_of)."""
import numpy as np

from tests.revise_cases import aug_of, pick_users  # noqa: F401  (re-exported)

UNKNOWN_ITEM = 999_999   # never in any aug
NEW_ITEM = 888_888       # unknown to train, given by some queries: only the query user rates it in aug
NONE_I, NONE_R = np.empty(0, dtype=np.int32), np.empty(0)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64).tolist()


def hold_out(full, users, m):
    """train = full minus the last m file rows of every user of `users`; rows[u] = (items, ratings) of those rows in file order"""
    out = np.zeros(len(full[0]), dtype=bool)
    rows = {}
    for u in users:
        idx = np.flatnonzero(full[0] == u)[-m:] if m else np.empty(0, dtype=np.int64)
        out[idx] = True
        rows[u] = (full[1][idx].astype(np.int32), full[2][idx])
    return tuple(a[~out] for a in full), rows


def syn100k(d, shuffled=False):
    """the plain file order, or a shuffled one with non-dyadic ratings"""
    full = (d.train.users, d.train.items, d.train.ratings)
    if shuffled:
        order = np.random.default_rng(41).permutation(len(full[0]))
        u, i, r = (a[order] for a in full)
        full = (u, i, np.round(r * 0.93 + 0.1, 2))
    return full


def pred_items(train, q, removed, items):
    """every train item, the user's own train items, the removed and the additional items, an id never seen, and the item
    unknown to train (the query's own when it gives it)"""
    return np.concatenate([np.unique(train[1]), train[1][train[0] == q], removed, items, [UNKNOWN_ITEM, NEW_ITEM]]).astype(np.int32)


def revise_queries(train, q):
    """name -> (removed, items, ratings) for a fitted user q: a removed item others rate, a re-rated item, both with an
    additional new item"""
    at = np.flatnonzero(train[0] == q)
    mine, vals = train[1][at].astype(np.int32), train[2][at]
    cnt = {int(i): int(c) for i, c in zip(*np.unique(train[1], return_counts=True))}
    shared = [j for j in range(len(mine)) if cnt[int(mine[j])] > 1]
    a, b = shared[0], shared[len(shared) // 2]
    other = lambda r: float(np.round(5.9 - r, 2)) if r != np.round(r) else float(r - 2 if r >= 3 else r + 2)
    return {
        "removed": (mine[[a]], NONE_I, NONE_R),
        "rerated": (mine[[b]], mine[[b]], np.array([other(vals[b])])),
        "mixed": (mine[[a, b]], np.array([NEW_ITEM, mine[b]], dtype=np.int32), np.array([3.7, other(vals[b])])),
    }


# ---- the hand set: the edges of the fold's 64-entry loads ----------------------------------------------------------------------
# items and their number of train raters; EDGE_NEVER is the one no query of edge_queries rates
EDGE_ITEMS = {11: 1, 12: 63, 13: 64, 14: 65, 15: 129, 16: 30}
EDGE_NEVER, EDGE_LONG = 16, 15
EDGE_FIRST, EDGE_MIDDLE, EDGE_LAST = 7, 60, 100  # fitted users whose row on EDGE_LONG is the first / a middle / the last file row of it
EDGE_LONE_USER, EDGE_LONE_ITEM = 5, 11           # the only rater of item 11


def edge_set(seed=11):
    """140 users x 6 train items (a seventh, NEW_ITEM, comes from the queries) with 1, 63, 64, 65 and 129 raters: item lists that
    end one short of, at, and one past a 64-entry load, and two loads plus one.  Non-dyadic ratings, shuffled file order, then
    the rows of EDGE_FIRST / EDGE_LAST on the 129-rater item moved to the front / the end of the file.  Most users have 1-4 rows."""
    rng = np.random.default_rng(seed)
    everyone = np.arange(1, 141, dtype=np.int32)
    raters = {15: everyone[:129]}
    raters[14] = np.concatenate([everyone[129:], rng.choice(everyone[:129], 65 - 11, replace=False)])
    raters[13] = rng.choice(everyone, 64, replace=False)
    raters[12] = rng.choice(everyone, 63, replace=False)
    raters[16] = rng.choice(np.setdiff1d(everyone, [EDGE_FIRST, EDGE_MIDDLE, EDGE_LAST]), 30, replace=False)
    raters[11] = np.array([EDGE_LONE_USER], dtype=np.int32)
    us = np.concatenate([raters[i] for i in sorted(raters)]).astype(np.int32)
    its = np.concatenate([np.full(len(raters[i]), i, dtype=np.int32) for i in sorted(raters)])
    rts = np.round(rng.uniform(0.6, 4.9, len(us)), 2)
    order = rng.permutation(len(us))
    us, its, rts = us[order], its[order], rts[order]
    first = int(np.flatnonzero((us == EDGE_FIRST) & (its == EDGE_LONG))[0])
    last = int(np.flatnonzero((us == EDGE_LAST) & (its == EDGE_LONG))[0])
    rest = [j for j in range(len(us)) if j not in (first, last)]
    order = np.array([first] + rest + [last])
    return us[order], its[order], rts[order]


def edge_queries(train):
    """name -> (user, removed, items, ratings).  Fold-in users with 1, 4, 5 and 6 rows; fitted users whose own row on the long item
    is its first / a middle / its last file row, as update queries (an additional row each) and as revise queries (another of
    their items removed, so the own row survives; the long row itself removed; the long row re-rated)."""
    u, i, r = train
    mine = lambda q: i[u == q].astype(np.int32)
    out = {
        "new_1": (901, NONE_I, np.array([15], dtype=np.int32), np.array([4.2])),
        "new_1_unknown": (902, NONE_I, np.array([NEW_ITEM], dtype=np.int32), np.array([1.3])),
        "new_4": (903, NONE_I, np.array([15, NEW_ITEM, 12, 14], dtype=np.int32), np.array([4.2, 1.1, 3.3, 2.4])),
        "new_5": (904, NONE_I, np.array([13, 15, 11, 14, 12], dtype=np.int32), np.array([0.7, 4.4, 2.9, 3.1, 1.8])),
        "new_6": (905, NONE_I, np.array([NEW_ITEM, 13, 15, 11, 14, 12], dtype=np.int32), np.array([2.2, 0.7, 4.4, 2.9, 3.1, 1.8])),
    }
    for name, q in (("first", EDGE_FIRST), ("middle", EDGE_MIDDLE), ("last", EDGE_LAST)):
        free = np.setdiff1d([12, 13, 14], mine(q))
        extra = np.array([NEW_ITEM] + free[:1].tolist(), dtype=np.int32)
        out[f"update_{name}"] = (q, NONE_I, extra, np.array([3.6, 1.4])[:len(extra)])
        out[f"update_{name}_bare"] = (q, NONE_I, NONE_I, NONE_R)
        out[f"revise_{name}_rerate_long"] = (q, np.array([EDGE_LONG], dtype=np.int32), np.array([EDGE_LONG], dtype=np.int32), np.array([0.9]))
        others = np.setdiff1d(mine(q), [EDGE_LONG])
        if len(others):
            out[f"revise_{name}_keep_long"] = (q, others[:1].astype(np.int32), extra[:1], np.array([2.8]))
            out[f"revise_{name}_drop_long"] = (q, np.array([EDGE_LONG], dtype=np.int32), NONE_I, NONE_R)
    # the lone item: removed (it leaves aug), re-rated (one term: the user's own)
    out["lone_removed"] = (EDGE_LONE_USER, np.array([EDGE_LONE_ITEM], dtype=np.int32), NONE_I, NONE_R)
    out["lone_rerated"] = (EDGE_LONE_USER, np.array([EDGE_LONE_ITEM], dtype=np.int32), np.array([EDGE_LONE_ITEM], dtype=np.int32), np.array([4.6]))
    return out


# ---- just past the fitted path's table limit ---------------------------------------------------------------------------------
def wide_set(seed=23, n_users=2100, n_items=300, per_user=25):
    rng = np.random.default_rng(seed)
    us = np.repeat(np.arange(1, n_users + 1, dtype=np.int32), per_user)
    its = np.concatenate([rng.choice(np.arange(1, n_items + 1, dtype=np.int32), per_user, replace=False) for _ in range(n_users)])
    rts = rng.integers(1, 11, len(us)).astype(np.float64) / 2
    order = rng.permutation(len(us))
    return us[order], its[order].astype(np.int32), rts[order]


# ---- the answers and their parts from the oracle -------------------------------------------------------------------------------
def oracle_answers(oracle, aug, q, sim, items, ns):
    """predict on `items` and recommend(n) for n of ns from predictor(aug, weightedSumDeviation(aug, S)): a fresh pipeline, only
    q ever evaluated"""
    p = oracle.Model(*aug).pipeline(sim, -1)
    return [p.predict(q, int(i)) for i in items], [p.recommend(q, n) for n in ns]


def fold_parts(oracle, aug, q, sim, item, own_last=False):
    """(num, den) of (q, item) on aug as :520-524 fold them, from the oracle's similarities and deviations; own_last moves q's
    own term from its file place to the end"""
    m = oracle.Model(*aug)
    p = m.pipeline(sim, -1)
    dev = m.normalized_deviations()
    rows = np.flatnonzero(aug[1] == item)
    if own_last:
        rows = np.concatenate([rows[aug[0][rows] != q], rows[aug[0][rows] == q]])
    num = den = 0.0
    for t in rows:
        s = p.raw_similarity(q, int(aug[0][t]))
        num = num + dev[t] * s
        den = den + abs(s)
    return num, den
