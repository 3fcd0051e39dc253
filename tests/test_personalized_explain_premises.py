"""What test_gpu_personalized_explain.py takes for granted, shown on the CPU: the fold of PersonalTermModel's terms IS the
oracle's weightedSumDeviation and its combine IS the oracle's Personalized prediction, bit for bit, on every input of the GPU
tests; and each input has the feature its GPU test relies on."""
import numpy as np
import pytest

from tests import personalized_explain_model as pm


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _sim(oracle, name):
    return {"cosine": oracle.SIM_COSINE, "jaccard": oracle.SIM_JACCARD}[name]


def _check(oracle, sim_name, train, users, items):
    """the model's rows, after comparing each with the oracle's own wsd and prediction"""
    tm = pm.PersonalTermModel(oracle, oracle.Model(*train), _sim(oracle, sim_name))
    want = tm.rows(users, items)
    for u, i, r in zip(users.tolist(), items.tolist(), want):
        if r.count:  # (the oracle's wsd of a row without terms is 0.0 by :527-529; its prediction is compared below)
            wsd = r.num / r.den if r.den > 0 else 0.0
            assert _bits(wsd) == _bits(tm.pipeline.wsd(u, i)), (u, i)
        else:
            assert (r.num, r.den) == (0.0, 0.0)
        assert _bits(r.prediction) == _bits(tm.pipeline.predict(u, i)), (u, i)
    return tm, want


def _more_than_four(train):
    return np.bincount(np.unique(train[0], return_inverse=True)[1]).min() > 4


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_small_case(oracle, sim_name):
    train, u, i = pm.small_case()
    assert _more_than_four(train)  # the fitted Personalized predictor accepts the train with the adjusted cosine
    tm, want = _check(oracle, sim_name, train, u, i)
    counts = np.array([r.count for r in want])
    assert counts.max() >= 40 and (counts == 0).sum() >= 2  # long rows; the absent user and the absent item
    assert len(set(zip(u.tolist(), i.tolist()))) < len(u)  # a row twice
    pairs = set(zip(train[0].tolist(), train[1].tolist()))
    own = [j for j in range(len(u)) if (int(u[j]), int(i[j])) in pairs]
    assert len(own) >= 2 and all(int(u[j]) in want[j].raters.tolist() for j in own)  # the own term is a term
    # the caps of the GPU test truncate the longest row, and below its cut two magnitudes share their first radix digit and
    # differ: the select has to descend
    big = want[int(np.argmax(counts))]
    caps = pm.caps_of(big.count)
    assert 1 < caps[2] < big.count
    mags = np.unique(np.abs(big.sims))
    assert len(mags) >= 2 and len({pm.top_byte(m) for m in mags}) < len(mags)
    if sim_name == "jaccard":  # rational similarities: exact ties, and some cap of the test ends inside a tie group
        cut = 0
        for r in want:
            s = np.abs(r.sims[r.by_weight])
            cut += sum(1 for cap in pm.caps_of(r.count) if 0 < cap < r.count and s[cap - 1] == s[cap])
        assert cut > 0


@pytest.mark.parametrize("n_users", [63, 64, 65, 255, 256, 257, 600])
def test_dense_case_has_one_term_per_user(oracle, n_users):
    train, u, i = pm.dense_case(n_users)
    assert _more_than_four(train)
    _, want = _check(oracle, "cosine", train, u, i)
    assert [r.count for r in want[:3]] == [n_users] * 3  # everybody, the user itself included
    assert all(int(u[j]) in want[j].raters.tolist() for j in range(3))


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_clone_case_has_ties_that_a_cap_cuts(oracle, sim_name):
    train, u, i = pm.clone_case()
    assert _more_than_four(train)
    _, want = _check(oracle, sim_name, train, u, i)
    cut = both = 0
    for r in want:
        s = r.sims[r.by_weight]
        for cap in range(1, r.count):
            if abs(s[cap - 1]) == abs(s[cap]):
                cut += 1
                both += int(s[cap - 1] != s[cap])
    assert cut > 0 and (sim_name == "jaccard" or both > 0)  # tie groups; with the cosine, of both signs


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_disjoint_case_has_raters_that_are_no_terms(oracle, sim_name):
    train, u, i, cold = pm.disjoint_case()
    assert _more_than_four(train)
    tm, want = _check(oracle, sim_name, train, u, i)
    cold = set(cold.tolist())
    lonely = [j for j in range(len(u)) if int(u[j]) in cold and want[j].count == 0]
    assert lonely and all(len(tm.item_rows[int(i[j])]) > 0 for j in lonely)  # raters, every one at similarity 0.0
    own = [j for j in range(len(u)) if want[j].count == 1 and want[j].raters[0] == u[j]]
    assert len(own) == len(cold)  # the own term alone


def test_negative_case(oracle):
    train, u, i, low = pm.negative_case()
    assert _more_than_four(train)
    tm, want = _check(oracle, "cosine", train, u, i)
    assert all(tm.model.users_avg(int(x)) < 0 for x in low)
    assert [want[0].count, want[1].count] == [0, 0] and want[0].prediction == tm.model.average()
    assert set(low.tolist()) <= set(want[2].raters.tolist())  # raters of a negative mean are terms of other users' rows
