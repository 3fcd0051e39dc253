"""The premises of tests/test_gpu_personalized_query_explain.py, from the oracle alone (no GPU).  For every input of those tests
the model's fold and combine ARE the oracle's Personalized prediction on aug, bit for bit, and every input has the feature its
GPU test relies on: the term counts around the 64-entry loads, the place of the own term, the forced radix descent, the ties."""
import numpy as np
import pytest

from tests import personalized_explain_model as pm
from tests import personalized_query_cases as pc
from tests import personalized_query_explain_cases as xc


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64).tolist()


def _sims(oracle):
    return {"cosine": oracle.SIM_COSINE, "jaccard": oracle.SIM_JACCARD}


def _check_against_predict(oracle, tag, train, query, sim, items):
    """model row == a fresh pipeline's predict on aug; the rows"""
    tm = xc.term_model(oracle, tag, train, query, sim)
    rows = xc.want_rows(oracle, tag, train, query, sim, items)
    fresh = tm.model.pipeline(sim, -1)
    q = query[0]
    assert _bits([r.prediction for r in rows]) == _bits([fresh.predict(q, int(i)) for i in items]), (tag, q)
    for r in rows:  # the caller's fold of the terms is the row's sums, and the combine with the query's mean its prediction
        assert _bits(pm.fold(r.sims, r.devs)) == _bits([r.num, r.den])
        assert _bits(pm.combine(oracle, tm.model.users_avg(q), r.num, r.den)) == _bits(r.prediction)
    return rows


def _own_place(row, q):
    at = np.flatnonzero(row.raters == q)
    return int(at[0]) if len(at) else None


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_edge_set(oracle, sim_name):
    sim = _sims(oracle)[sim_name]
    train, queries, items = xc.edge_cases()
    assert len(np.unique(train[0])) == 140 and len(np.unique(train[1])) == 6
    rows = {name: _check_against_predict(oracle, "edge", train, q, sim, items[name]) for name, q in queries.items()}
    at = lambda name, item: rows[name][items[name].tolist().index(item)]
    counts = {r.count for rs in rows.values() for r in rs}
    if sim_name == "jaccard":
        assert counts >= {0, 1, 2, 30, 63, 64, 65, 66, 129, 130}, sorted(counts)
    # the own term of a fitted user on the long item: first, in the middle, last; re-rated: moved to the end
    for name, q, place in (("first", pc.EDGE_FIRST, 0), ("middle", pc.EDGE_MIDDLE, None), ("last", pc.EDGE_LAST, 128)):
        r = at(f"update_{name}", pc.EDGE_LONG)
        own = _own_place(r, q)
        if sim_name == "jaccard":
            assert r.count == 129
            assert own == place if place is not None else own == 120
        else:
            assert own is not None and (0 < own < r.count - 1 if place is None else own == (0 if place == 0 else r.count - 1))
        r = at(f"revise_{name}_rerate_long", pc.EDGE_LONG)
        assert _own_place(r, q) == r.count - 1
        r = at(f"revise_{name}_drop_long", pc.EDGE_LONG) if f"revise_{name}_drop_long" in rows else None
        assert r is None or _own_place(r, q) is None
    # fold-in users: the own term last on every item they rate
    for name in ("new_4", "new_5", "new_6"):
        q, _, its, _ = queries[name]
        for i in its.tolist():
            r = at(name, i)
            assert r.count >= 1 and _own_place(r, q) == r.count - 1, (name, i)
    if sim_name == "jaccard":
        assert at("new_5", pc.EDGE_LONG).count == 130 and _own_place(at("new_5", pc.EDGE_LONG), 904) == 129
    # one term: the user's own; none: the item left aug
    r = at("lone_rerated", pc.EDGE_LONE_ITEM)
    assert r.count == 1 and r.raters.tolist() == [pc.EDGE_LONE_USER]
    for name in ("new_4", "new_6", "update_first"):
        r = at(name, pc.NEW_ITEM)
        assert r.count == 1 and r.raters.tolist() == [queries[name][0]]
    r = at("lone_removed", pc.EDGE_LONE_ITEM)
    assert r.count == 0 and _bits([r.num, r.den]) == [0, 0]
    for rs in rows.values():
        assert rs[-2].count == 0  # UNKNOWN_ITEM
    if sim_name == "cosine":  # S(u, u) == 0.0: no row has a term
        for name in ("new_1", "new_1_unknown"):
            tm = xc.term_model(oracle, "edge", train, queries[name], sim)
            assert tm.similarity(queries[name][0], queries[name][0]) == 0.0
            assert all(r.count == 0 for r in rows[name])
            assert _bits([r.prediction for r in rows[name]]) == _bits([tm.model.users_avg(queries[name][0])] * len(rows[name]))
    else:
        tm = xc.term_model(oracle, "edge", train, queries["new_4"], sim)
        assert tm.similarity(903, 903) == 1.0


@pytest.mark.parametrize("n", xc.DENSE_SIZES)
def test_dense_sets(oracle, n):
    train, queries, items = xc.dense_cases(n)
    ties = 0
    for name, query in queries:
        rows = _check_against_predict(oracle, f"dense{n}", train, query, oracle.SIM_COSINE, items)
        r = rows[0]  # item 1: everybody rates it
        assert items[0] == 1
        if name == "fold_in":
            assert r.count == n + 1 and _own_place(r, query[0]) == n
        else:
            assert r.count == n and 0 < _own_place(r, query[0]) < n - 1
        # one top byte: every cap < count descends past the first radix digit
        assert len({pm.top_byte(s) for s in r.sims}) == 1
        mags = np.abs(r.sims[r.by_weight])
        ties += int((mags[1:] == mags[:-1]).sum())
    assert ties >= {63: 40, 600: 500}.get(n, 1), ties


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_clone_queries(oracle, sim_name):
    sim = _sims(oracle)[sim_name]
    train, queries, items = xc.clone_cases()
    assert len(items) == 6
    pairs = opposite = 0
    for name, query in queries:
        rows = _check_against_predict(oracle, "clones", train, query, sim, items)
        assert xc.tie_cuts(rows), name
        for r in rows:
            s = r.sims[r.by_weight]
            tied = np.abs(s[1:]) == np.abs(s[:-1])
            pairs += int(tied.sum())
            opposite += int((tied & (np.sign(s[1:]) != np.sign(s[:-1]))).sum())
    assert pairs >= 170, pairs
    if sim_name == "cosine":
        assert opposite >= 100, opposite
    assert xc.family(train, queries[0][1]) == "query" and xc.family(train, queries[1][1]) == "update" and xc.family(train, queries[2][1]) == "revise"


def test_wide_set(oracle):
    train, queries, items = xc.wide_cases()
    assert len(np.unique(train[0])) == 2100
    for name, query in queries:
        rows = _check_against_predict(oracle, "wide", train, query, oracle.SIM_COSINE, items[name])
        assert max(r.count for r in rows) > 64 and rows[-1].count == 0  # several loads; UNKNOWN_ITEM
        assert rows[-2].count == (1 if name == "update" else 0)          # NEW_ITEM: the update query gives it
        own = [_own_place(r, query[0]) for r in rows]
        assert any(p is not None for p in own)
