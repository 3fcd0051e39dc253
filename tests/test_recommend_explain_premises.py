"""The inputs of tests/test_gpu_recommend_explain.py exercise what those tests rely on — from the CPU oracle alone.

The dense fold-in and update users get 33 and 32 recommended rows whose term counts straddle cap = 8 and stay below cap = 64,
and every recommended prediction is the term model's; the seven hand-set queries have different counts below the widest of their
chunk; one dense query has nothing left to recommend and one has 2 rows where 3 are asked for."""
import numpy as np
import pytest

from tests import query_explain_cases as qc
from tests import recommend_explain_cases as cases
from tests import revise_cases as rc


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("n,terms", [(64, (5, 16)), (257, (26, 52))])
def test_dense_rows_and_their_term_counts(oracle, n, terms):
    train = cases.dense_train(n)
    assert len(np.unique(train[0])) == n and np.unique(train[1]).tolist() == list(range(1, 41))
    k = qc.dense_k(n)
    for name, want in (("fold_in", 33), ("update", 32)):
        query = cases.dense_queries(train)[name]
        tm = qc.term_model(oracle, f"dense{n}", train, query, oracle.SIM_COSINE, k)
        items, preds = tm.pipeline.recommend(query[0], cases.N_RECO)
        assert len(items) == want, name
        rows = tm.rows([query[0]] * len(items), items)
        assert np.array_equal(_bits(preds), _bits([r.prediction for r in rows])), name  # the explained prediction, bit for bit
        counts = [r.count for r in rows]
        if name == "fold_in":
            assert (min(counts), max(counts)) == terms
        assert max(counts) <= 64 and (n == 64 or min(counts) > 8)  # cap = 64 truncates nothing; cap = 8 every row at n = 257


def test_hand_set_counts_differ_inside_a_chunk(oracle):
    train, queries = cases.small_cases()
    counts = []
    for query in queries:
        p = oracle.Model(*rc.aug_of(train, *query)).pipeline(oracle.SIM_COSINE, 5)
        p.neighbors(query[0])
        counts.append(len(p.recommend(query[0], cases.N_RECO)[0]))
    assert counts == [27, 27, 26, 29, 18, 18, 19]
    assert all(cases.family(train, q) == "revise" for q in queries)


def test_empty_and_short_dense_queries(oracle):
    train = cases.dense_train(64)
    for query, n, want in ((cases.full_query(), cases.N_RECO, 0), (cases.short_query(), 3, 2), (cases.short_query(), cases.N_RECO, 2)):
        p = oracle.Model(*rc.aug_of(train, *query)).pipeline(oracle.SIM_COSINE, qc.dense_k(64))
        p.neighbors(query[0])
        assert len(p.recommend(query[0], n)[0]) == want


def test_dense_batch_shape():
    batch = cases.dense_batch()
    assert len(batch) == 65 and len({q[0] for q in batch}) == 65
    refused = batch[cases.BATCH_REFUSED]
    assert len(refused[2]) - len(np.unique(refused[2])) == 1
    for j, q in enumerate(batch):
        if j != cases.BATCH_REFUSED:
            assert len(np.unique(q[2])) == len(q[2]) and len(set(q[3].tolist())) > 1
    assert len(batch[cases.BATCH_EMPTY][2]) == 40 and len(batch[cases.BATCH_SHORT][2]) == 38


def test_workspaces_give_the_chunks_and_sub_ranges_claimed():
    for c, ws in cases.WORKSPACES.items():
        assert cases.chunk_of(ws, 257, 40) == c
    ws = cases.WORKSPACES[2]
    assert cases.sub_range_of(ws, 64, False) == 31 and cases.sub_range_of(ws, 64, True) == 15
