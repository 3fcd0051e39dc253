"""Inputs and expected values of the query-explanation tests (knncf_query_explain* / knncf_update_explain* /
knncf_revise_explain*), shared by the premises test (CPU, oracle only) and the GPU tests so that both speak about the same
queries.  A query is (user, removed items, additional items, additional ratings), as in tests/revise_cases.py; a fold-in or
update query has no removed items.  The expected terms come from tests/explain_model.TermModel on aug with a fresh pipeline
whose first call is the query user's neighbourhood."""
import numpy as np

from tests import explain_model
from tests import revise_cases as rc

NONE_I, NONE_R = np.empty(0, dtype=np.int32), np.empty(0)
ABSENT_USERS = (987_654, 987_655)
ABSENT_ITEM = 876_543

# ---- the dense train of explain_model.dense_train(n, 5): everybody rates item 1 ------------------------------------------------
DENSE_SEED, DENSE_K = 5, 200
DENSE_USER = 9001
DENSE_ITEMS = np.array([1, 2, 7, 40, ABSENT_ITEM], dtype=np.int32)
# trips of 64 segment entries (63, 64, 65), more than two trips with ties (131), and the 256 terms one BY_WEIGHT pass of
# k_qb_explain ranks per wave (64 lanes x 4 terms): 255, 256, 257
DENSE_SIZES = (63, 64, 65, 131, 255, 256, 257)


def dense_k(n):
    return max(DENSE_K, n + 1)  # every train user is a listed neighbour


def dense_query():
    """the fold-in user: item 1 like everybody, six of the other items; every similarity is positive"""
    return DENSE_USER, NONE_I, np.arange(1, 8, dtype=np.int32), np.array([5, 2, 2, 2, 2, 2, 2], dtype=np.float64)


def dense_update(train):
    """a fitted user of the dense train with one additional item: everybody else is a term of item 1"""
    u = int(np.unique(train[0])[0])
    free = np.setdiff1d(np.arange(1, 41), train[1][train[0] == u])[:1].astype(np.int32)
    return u, NONE_I, free, np.array([3.0])


# ---- the disjoint case: 16 cold users whose train items nobody else rates ------------------------------------------------------
DISJOINT_K = 400


def disjoint_query(case):
    """a fold-in user on the first eight background items: similarity exactly 0.0 with every cold user and with the
    background users that share none of the eight"""
    items = np.unique(case.train[1][case.train[1] <= 120])[:8].astype(np.int32)
    return DENSE_USER, NONE_I, items, np.array([5, 4, 3, 2, 1, 5, 4, 3], dtype=np.float64)


def cold_private_item(case):
    """(a cold user, one of its private train items)"""
    u = int(case.groups["cold"][0])
    return u, int(case.train[1][(case.train[0] == u) & (case.train[1] > 120)][0])


# ---- syn-100k ---------------------------------------------------------------------------------------------------------------------
def additions_only(train, q):
    """the two new items of q's "mixed" revise query as an update query"""
    _, items, ratings = rc.case_query(train, q, "mixed")
    return NONE_I, items[[0, 2]].copy(), ratings[[0, 2]].copy()


def absent_query(train, n):
    """fold-in user n: the first 20 train rows of a picked user under a raw id that train does not hold"""
    src = rc.pick_users(train)[2 + n]
    at = np.flatnonzero(train[0] == src)[:20]
    return ABSENT_USERS[n], NONE_I, train[1][at].astype(np.int32), train[2][at].copy()


def syn_queries(train, q):
    """name -> (user, removed, items, ratings) of picked user q: two revise queries and the additions-only update query"""
    return {"mixed": (q,) + rc.case_query(train, q, "mixed"), "delete1": (q,) + rc.case_query(train, q, "delete1"),
            "with": (q,) + additions_only(train, q)}


# ---- expected values ----------------------------------------------------------------------------------------------------------------
_models = {}


def term_model(oracle, tag, train, query, sim, k):
    """TermModel on aug of `query` whose first evaluation is the query user's; `tag` names the train set.  The oracle models
    and the term models are built once per process."""
    q, removed, items, ratings = query
    key = (tag, q, tuple(removed.tolist()), tuple(items.tolist()), tuple(ratings.tolist()))
    if key not in _models:
        _models[key] = oracle.Model(*rc.aug_of(train, q, removed, items, ratings))
    if (key, sim, k) not in _models:
        tm = explain_model.TermModel(oracle, _models[key], sim, k)
        tm._neighbors(q)  # first evaluation: the user's
        _models[key, sim, k] = tm
    return _models[key, sim, k]


def expected(rows, cap, order):
    """what the wrappers return for the model's rows: (raters [m, cap], sims, devs, counts, sums [m, 2], predictions), the
    cells beyond a row's min(count, cap) terms padded with -1 / nan"""
    m = len(rows)
    raters = np.full((m, cap), -1, dtype=np.int32)
    sims, devs = np.full((m, cap), np.nan), np.full((m, cap), np.nan)
    for j, row in enumerate(rows):
        r, s, d = row.terms(order)
        t = min(row.count, cap)
        raters[j, :t], sims[j, :t], devs[j, :t] = r[:t], s[:t], d[:t]
    return (raters, sims, devs, np.array([r.count for r in rows], dtype=np.int32),
            np.array([[r.num, r.den] for r in rows], dtype=np.float64).reshape(m, 2),
            np.array([r.prediction for r in rows], dtype=np.float64))
