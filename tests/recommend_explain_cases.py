"""Inputs and helpers of the tests of knncf_*_recommend_explain* (recommendations with the terms behind them in one pass),
shared by the premises test (CPU, oracle only) and the GPU tests so that both speak about the same queries.  Everything is
built from the existing case modules.  A query is (user, removed items, additional items, additional ratings), as in
tests/revise_cases.py; a fold-in or update query has no removed items."""
import numpy as np

from tests import explain_model
from tests import personalized_query_explain_cases as pxc
from tests import query_explain_cases as qc
from tests import revise_cases as rc

NONE_I, NONE_R = qc.NONE_I, qc.NONE_R
N_RECO = 40               # every item of the dense train: counts are I - known items
DENSE_SIZES = (64, 257)   # explain_model.dense_train(n, qc.DENSE_SEED): U train users, I = 40 items
BATCH_USERS = 9100        # the 65 fold-in users of dense_batch are BATCH_USERS + j
BATCH_EMPTY, BATCH_REFUSED, BATCH_SHORT = 10, 32, 40  # count 0 / a duplicate item / count 2 at n = 3
family = pxc.family


def dense_train(n):
    return explain_model.dense_train(n, qc.DENSE_SEED)


def dense_queries(train):
    """name -> query: the fold-in user (33 recommended rows of 40 items) and a fitted user with one more item (32 rows)"""
    return {"fold_in": qc.dense_query(), "update": qc.dense_update(train)}


def full_query(user=BATCH_USERS + BATCH_EMPTY):
    """a fold-in user that rates all 40 items: nothing is left to recommend"""
    ratings = np.full(40, 2.0)
    ratings[0] = 5.0
    return user, NONE_I, np.arange(1, 41, dtype=np.int32), ratings


def short_query(user=BATCH_USERS + BATCH_SHORT):
    """a fold-in user that rates 38 items: 2 recommendations whatever n >= 2 asks for"""
    ratings = np.full(38, 3.0)
    ratings[0] = 5.0
    return user, NONE_I, np.arange(1, 39, dtype=np.int32), ratings


def dense_batch():
    """65 fold-in queries on the dense trains (64 + 1 per chunk at the default budget): item 1 and six others each; query
    BATCH_EMPTY has count 0, BATCH_SHORT count 2, BATCH_REFUSED repeats an item (KNNCF_E_DUPLICATE) in the middle of chunk 0"""
    rng = np.random.default_rng(77)
    out = []
    for j in range(65):
        six = np.sort(rng.choice(np.arange(2, 41), 6, replace=False))
        items = np.concatenate([[1], six]).astype(np.int32)
        ratings = np.concatenate([[5.0], rng.integers(1, 5, 6).astype(np.float64)])
        out.append((BATCH_USERS + j, NONE_I, items, ratings))
    out[BATCH_EMPTY], out[BATCH_SHORT] = full_query(), short_query()
    u, _, items, ratings = out[BATCH_REFUSED]
    out[BATCH_REFUSED] = (u, NONE_I, np.append(items, items[3]).astype(np.int32), np.append(ratings, 2.0))
    return out


# ---- the budgets of include/knncf.h ("Batched fold-in queries", "Explanations of query predictions", "Explanations of
# Personalized query predictions") --------------------------------------------------------------------------------------------
def chunk_of(workspace, U, I):
    return max(1, min(64, (workspace // 2) // (64 * U + 96 * I)))


def sub_range_of(workspace, cap, personalized):
    return max(1, (workspace // 2) // ((40 if personalized else 20) * cap + 28))


# workspace_bytes at U = 257, I = 40: 2 queries per chunk and 31 kNN rows per launch at cap = 64 (sub-ranges cut through a query's
# 33 rows and across slots); 31 queries per chunk (one similarity pass per query) and 33 (the dual kernel)
WORKSPACES = {2: 82_000, 31: 1_260_000, 33: 1_340_000}


# ---- hand set and syn-100k ------------------------------------------------------------------------------------------------------------
def small_cases():
    """(train, the seven hand-set revise queries in name order)"""
    train = rc.small_set()
    return train, list(rc.small_queries(train).values())


def syn_cases(train):
    """14 queries on syn-100k: two revise queries and one update query of four picked users, two fold-in users"""
    queries = [query for q in rc.pick_users(train)[:4] for query in qc.syn_queries(train, q).values()]
    return queries + [qc.absent_query(train, n) for n in (0, 1)]


def by_family(train, queries):
    """family -> the positions of its queries"""
    out = {}
    for j, query in enumerate(queries):
        out.setdefault(family(train, query), []).append(j)
    return out


def as_family(fam, query):
    """the query as the family's batched wrappers take it"""
    return query if fam == "revise" else (query[0], query[2], query[3])
