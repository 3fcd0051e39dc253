"""The premises of tests/test_gpu_query_explain.py, from the oracle alone (no GPU): the inputs of tests/query_explain_cases.py
have the term counts, ties, zero-similarity neighbours and truncated rows the GPU tests rely on, so none of them can pass
vacuously."""
import numpy as np
import pytest

from tests import explain_model
from tests import query_explain_cases as qc
from tests import revise_cases as rc


@pytest.mark.parametrize("n", qc.DENSE_SIZES)
def test_dense_train_term_counts(oracle, n):
    train = explain_model.dense_train(n, qc.DENSE_SEED)
    tm = qc.term_model(oracle, f"dense{n}", train, qc.dense_query(), oracle.SIM_COSINE, qc.dense_k(n))
    rows = [tm.row(qc.DENSE_USER, int(i)) for i in qc.DENSE_ITEMS]
    assert rows[0].count == n  # item 1: every train user is a term
    assert rows[-1].count == 0 and (rows[-1].num, rows[-1].den) == (0.0, 0.0)  # an id unknown to train
    assert qc.DENSE_USER not in rows[0].raters.tolist()  # the user rates item 1 itself in aug
    if n == 131:
        assert len(np.unique(np.abs(rows[0].sims))) == 21  # BY_WEIGHT has ties
        assert [r.count for r in rows[1:4]] == [19, 31, 16]
        up = qc.dense_update(train)
        assert qc.term_model(oracle, "dense131", train, up, oracle.SIM_COSINE, qc.DENSE_K).row(up[0], 1).count == 130


def test_disjoint_case_has_listed_neighbours_that_are_no_terms(oracle):
    case = explain_model.disjoint_case()
    train = case.train
    assert case.num_users == 160
    query = qc.disjoint_query(case)
    assert len(query[2]) == 8 and query[2].max() <= 120
    tm = qc.term_model(oracle, "disjoint", train, query, oracle.SIM_COSINE, qc.DISJOINT_K)
    near = tm._neighbors(qc.DENSE_USER)
    assert len(near) == 160 and sum(1 for s in near.values() if s == 0.0) == 62
    cold, private = qc.cold_private_item(case)
    assert train[0][train[1] == private].tolist() == [cold] and cold in near  # one listed rater ...
    assert tm.row(qc.DENSE_USER, private).count == 0                           # ... and no term
    more = []
    for i in np.unique(train[1][train[1] <= 120]).tolist():
        listed = sum(1 for x in train[0][train[1] == i].tolist() if x in near)
        more.append(listed - tm.row(qc.DENSE_USER, i).count)
    assert min(more) >= 0 and max(more) == 27


@pytest.mark.parametrize("which", range(13))
def test_syn100k_rows_truncate_at_16_and_fit_256(oracle, syn100k, which):
    train = rc.syn100k(syn100k)
    users = rc.pick_users(train)
    assert len(users) == 13
    q = users[which]
    query = qc.syn_queries(train, q)["mixed"]
    tm = qc.term_model(oracle, "syn100k", train, query, oracle.SIM_COSINE, 300)
    counts = np.array([tm.row(q, int(i)).count for i in rc.pred_items(train, q, query[1], query[2])])
    # cap = 16 truncates hundreds of rows, cap = 256 none (the maxima of the thirteen users run from 158 to 212)
    assert 158 <= counts.max() <= 212 and (counts == 0).any() and (counts > 16).sum() >= 200
