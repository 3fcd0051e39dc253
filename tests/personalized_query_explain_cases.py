"""Inputs and expected values of the tests of knncf_query_explain_personalized* / knncf_update_explain_personalized* /
knncf_revise_explain_personalized*, shared by the premises test (CPU, oracle only) and the GPU tests so that both speak about
the same queries.  A query is (user, removed items, additional items, additional ratings), as in
tests/personalized_query_cases.py.  The expected terms of a row come from tests/personalized_explain_model.PersonalTermModel on
oracle.Model(*aug_of(train, query)), asked for row(query user, item): it asks the oracle only for raw_similarity(query user,
rater) and for the deviations, so it is the fresh-closure semantics with the query user as the first argument of every pair."""
import numpy as np

from tests import explain_model
from tests import personalized_explain_model as pm
from tests import personalized_query_cases as pc
from tests import query_explain_cases as qc

NONE_I, NONE_R = pc.NONE_I, pc.NONE_R
DENSE_SIZES = (63, 64, 65, 255, 256, 257, 600)
CLONE_ABSENT = 987_654

_models = {}


def term_model(oracle, tag, train, query, sim):
    """PersonalTermModel on aug of `query`; `tag` names the train set.  Built once per process."""
    q, removed, items, ratings = query
    key = (tag, int(q), tuple(np.asarray(removed).tolist()), tuple(np.asarray(items).tolist()), tuple(np.asarray(ratings).tolist()), sim)
    if key not in _models:
        _models[key] = pm.PersonalTermModel(oracle, oracle.Model(*pc.aug_of(train, q, removed, items, ratings)), sim)
    return _models[key]


def want_rows(oracle, tag, train, query, sim, items):
    """the model's rows of (query user, item) for every requested item"""
    tm = term_model(oracle, tag, train, query, sim)
    return [tm.row(query[0], int(i)) for i in np.asarray(items).tolist()]


def family(train, query):
    """the family whose single form answers the query: an absent user -> fold-in, no removals -> update, else revise"""
    q, removed, _, _ = query
    if len(removed):
        return "revise"
    return "update" if (train[0] == q).any() else "query"


def edge_cases():
    """(train, name -> query, name -> requested items) on pc.edge_set()"""
    train = pc.edge_set()
    queries = pc.edge_queries(train)
    return train, queries, {name: pc.pred_items(train, q[0], q[1], q[2]) for name, q in queries.items()}


def dense_cases(n):
    """(train, [(name, query)], requested items) on explain_model.dense_train(n, seed=n): the fold-in user of
    query_explain_cases (n + 1 terms on item 1, the own term last) and a fitted user with one more item (n terms, the own term
    at its file place)"""
    train = explain_model.dense_train(n, seed=n)
    return train, [("fold_in", qc.dense_query()), ("update", qc.dense_update(train))], qc.DENSE_ITEMS


def clone_cases():
    """(train, [(name, query)], requested items) on explain_model.clone_case(): a user of groups["clones0"] as a fold-in query (its
    train rows under an absent id), an update query (one NEW_ITEM row) and a revise query (its first item re-rated); the six
    most-rated train items"""
    c = explain_model.clone_case()
    u = int(c.groups["clones0"][0])
    at = np.flatnonzero(c.train[0] == u)
    mine, vals = c.train[1][at].astype(np.int32), c.train[2][at].astype(np.float64)
    again = float(vals[0] - 2 if vals[0] >= 3 else vals[0] + 2)
    queries = [("fold_in", (CLONE_ABSENT, NONE_I, mine, vals)),
               ("update", (u, NONE_I, np.array([pc.NEW_ITEM], dtype=np.int32), np.array([3.7]))),
               ("revise", (u, mine[:1], mine[:1], np.array([again])))]
    ids, counts = np.unique(c.train[1], return_counts=True)
    top = ids[np.argsort(-counts, kind="stable")][:6].astype(np.int32)
    return c.train, queries, top


def tie_cuts(rows):
    """cap -> the rows (indices) in which a cut after `cap` BY_WEIGHT terms falls inside a group of equal magnitudes"""
    cuts = {}
    for j, r in enumerate(rows):
        s = np.abs(r.sims[r.by_weight])
        for cap in range(1, r.count):
            if s[cap - 1] == s[cap]:
                cuts.setdefault(cap, []).append(j)
    return cuts


def wide_cases():
    """(train, [(name, query)], name -> requested items) on pc.wide_set() (2100 users): a fitted user with a NEW_ITEM row, and a
    fold-in user with eight rows"""
    train = pc.wide_set()
    u = int(np.unique(train[0])[17])
    mine = train[1][train[0] == u].astype(np.int32)
    others = np.setdiff1d(np.unique(train[1]), mine).astype(np.int32)
    queries = [("update", (u, NONE_I, np.array([pc.NEW_ITEM], dtype=np.int32), np.array([4.5]))),
               ("fold_in", (5001, NONE_I, others[:8].copy(), np.array([4.5, 1.0, 3.5, 2.0, 5.0, 0.5, 3.0, 2.5])))]
    items = {"update": np.array([mine[0], mine[-1], others[0], others[-1], pc.NEW_ITEM, pc.UNKNOWN_ITEM], dtype=np.int32),
             "fold_in": np.array([others[0], others[7], others[8], mine[0], pc.NEW_ITEM, pc.UNKNOWN_ITEM], dtype=np.int32)}
    return train, queries, items
