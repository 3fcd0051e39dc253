"""The premises of test_gpu_explain.py, on the CPU: the term lists that tests/explain_model.py derives from the oracle's
neighbour lists, deviations and the training file fold to the oracle's own wsd and prediction BIT FOR BIT — so the terms are
well defined by the reference, and the helper may stand in for it on the GPU."""
import numpy as np
import pytest

from tests import explain_model

SETTINGS = [("cosine", 10), ("cosine", 300), ("jaccard", 50)]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64).tolist()


def _sim(oracle, name):
    return {"cosine": oracle.SIM_COSINE, "jaccard": oracle.SIM_JACCARD}[name]


def _check_rows(oracle, tm, users, items):
    rows = tm.rows(users, items)
    for u, i, row in zip(users.tolist(), items.tolist(), rows):
        num, den = explain_model.fold(*row.terms(explain_model.SUM_ORDER)[1:])
        assert _bits([num, den]) == _bits([row.num, row.den])
        wsd = num / den if den > 0 else 0.0
        assert _bits(wsd) == _bits(tm.pipeline.wsd(u, i)), (u, i)
        assert _bits(row.prediction) == _bits(tm.pipeline.predict(u, i)), (u, i)
        assert u not in row.raters.tolist() and (row.sims != 0.0).all()
        r, s, d = row.terms(explain_model.BY_WEIGHT)
        assert sorted(zip(r.tolist(), _bits(s), _bits(d))) == sorted(zip(row.raters.tolist(), _bits(row.sims), _bits(row.devs)))
        mag = np.abs(s)
        assert (mag[:-1] >= mag[1:]).all()
    return rows


@pytest.fixture(scope="module")
def model100k(oracle, syn100k):
    d = syn100k
    return oracle.Model(d.train.users, d.train.items, d.train.ratings)


@pytest.mark.parametrize("sim_name,k", SETTINGS)
def test_fold_of_the_terms_is_the_oracles_wsd_and_prediction(oracle, syn100k, model100k, sim_name, k):
    d = syn100k
    pick = np.random.default_rng(11).choice(len(d.test.users), 60, replace=False)
    tm = explain_model.TermModel(oracle, model100k, _sim(oracle, sim_name), k)
    rows = _check_rows(oracle, tm, d.test.users[pick], d.test.items[pick])
    counts = np.array([r.count for r in rows])
    assert counts.max() <= k
    if k == 300:  # the premise of the GPU oracle test: rows with several terms, whose ORDER therefore matters
        assert (counts >= 2).mean() >= 0.9, counts.tolist()


@pytest.mark.parametrize("case_name", ["disjoint", "clones"])
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_zero_similarity_neighbours_and_exact_ties(oracle, case_name, sim_name):
    c = explain_model.disjoint_case() if case_name == "disjoint" else explain_model.clone_case()
    model = oracle.Model(*c.train)
    k = c.num_users  # k >= U - 1: everybody is in everybody's list, zero similarities included
    tm = explain_model.TermModel(oracle, model, _sim(oracle, sim_name), k)
    rows = _check_rows(oracle, tm, c.test[0][:80], c.test[1][:80])
    if case_name == "disjoint":
        cold = set(c.groups["cold"].tolist())
        u = next(int(x) for x in c.test[0] if int(x) not in cold)
        ids, sims = tm.pipeline.neighbors(u)
        assert len(ids) == c.num_users - 1 and (sims == 0.0).sum() >= len(cold)  # in the list ...
        for x, i, row in zip(c.test[0][:80].tolist(), c.test[1][:80].tolist(), rows):
            if x not in cold:
                assert not cold & set(row.raters.tolist())  # ... and never a term
    else:
        ties = 0
        for row in rows:
            mag = np.abs(row.terms(explain_model.BY_WEIGHT)[1])
            ties += int((mag[:-1] == mag[1:]).sum())
        assert ties > 0


@pytest.mark.parametrize("neighbours", [63, 64, 65, 128, 129, 512, 513, 1024, 1025, 2048])
def test_dense_train_fills_the_neighbour_list(oracle, neighbours):
    """the premise of the GPU class-edge test: more than 4 ratings per user, and on the common item's rows every other user is
    a term — U - 1 matches, the whole per-wave capacity at U - 1 = 64, 128, 512, 1024, 2048"""
    tr = explain_model.dense_train(neighbours + 1, seed=neighbours)
    assert np.bincount(np.unique(tr[0], return_inverse=True)[1]).min() > 4
    u, i = explain_model.dense_rows(tr)
    tm = explain_model.TermModel(oracle, oracle.Model(*tr), oracle.SIM_COSINE, 2048)
    rows = _check_rows(oracle, tm, u, i)
    assert [r.count for r in rows] == [neighbours] * 3 + [rows[3].count, 0] and 0 < rows[3].count < neighbours
