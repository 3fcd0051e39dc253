"""The inputs of tests/bystander_cases.py reach the cases that bystander queries must get right, shown on the oracle alone (no
GPU): the newcomer displaces a last neighbour, ties with its copy on the cut in both set orders, changes predictions, is
summed in the bystander's order, is the only rater of an item, and shifts average(aug)."""
import numpy as np
import pytest

from tests import bystander_cases as bc
from tests.query_helpers import _bits


@pytest.fixture(scope="module")
def cases(synth, oracle):
    return {c.name: c for c in bc.all_cases(synth, oracle)}  # (no input raises OracleError)


def _lists(oracle, case, data, sim=None):
    m = oracle.Model(*data)
    return {v: m.pipeline(oracle.SIM_COSINE if sim is None else sim, case.k).neighbors(v) for v in case.others}


def test_every_case_is_there(cases):
    assert sorted(cases) == sorted(["near-clone", "tie-before", "tie-after", "short-59", "short-300", "tiny-1", "tiny-4", "tiny-5",
                                    "new-item", "off-scale"])
    base = cases["near-clone"].train
    assert (len(np.unique(base[0])), len(np.unique(base[1])), len(base[0])) == (60, 80, 1200)


def test_newcomer_displaces_a_last_neighbour_and_most_lists_stay(oracle, cases):
    c = cases["near-clone"]
    before, after = _lists(oracle, c, c.train), _lists(oracle, c, c.aug)
    entered = [v for v in c.others if c.q in after[v][0].tolist()]
    assert entered
    for v in entered:
        ids = after[v][0].tolist()
        assert len(ids) == c.k and before[v][0].tolist()[-1] not in ids, v  # the last entry dropped out
        assert [x for x in ids if x != c.q] == before[v][0].tolist()[:-1], v
    same = [v for v in c.others if after[v][0].tolist() == before[v][0].tolist() and _bits(after[v][1]) == _bits(before[v][1])]
    assert len(same) > len(c.others) // 2
    assert len(same) + len(entered) == len(c.others)


def test_tie_sits_on_the_cut_in_both_set_orders(oracle, cases):
    sides = set()
    for name in ("tie-before", "tie-after"):
        c = cases[name]
        w, v = c.note["copy_of"], c.note["bystander"]
        first = [x for x in oracle.Model(*c.aug).user_iteration_order().tolist() if x in (c.q, w)][0]
        sides.add(first == c.q)
        assert (first == c.q) == (c.note["side"] == "before")
        m = oracle.Model(*c.aug)
        assert _bits([m.fresh_similarity(oracle.SIM_COSINE, v, c.q)]) == _bits([m.fresh_similarity(oracle.SIM_COSINE, v, w)])
        ids = m.pipeline(oracle.SIM_COSINE, c.k).neighbors(v)[0].tolist()
        longer = m.pipeline(oracle.SIM_COSINE, c.k + 1).neighbors(v)[0].tolist()
        assert len(ids) == c.k and ids[-1] == first and longer[-1] == (w if first == c.q else c.q)
    assert sides == {True, False}


def test_short_lists_take_the_newcomer_everywhere(oracle, cases):
    for name in ("short-59", "short-300"):
        c = cases[name]
        for v, (ids, _) in _lists(oracle, c, c.aug).items():
            assert len(ids) == 60 - (c.k == 59) and c.q in ids.tolist(), (name, v)


def test_a_prediction_changes(oracle, cases):
    c = cases["near-clone"]
    m0, m1 = oracle.Model(*c.train), oracle.Model(*c.aug)
    changed = 0
    for v in c.others:
        for i in np.unique(c.train[1])[:20]:
            changed += _bits([m0.pipeline(oracle.SIM_COSINE, c.k).predict(v, int(i))]) != _bits([m1.pipeline(oracle.SIM_COSINE, c.k).predict(v, int(i))])
    assert changed > 0


def test_tiny_rows_fold_in_the_bystanders_order(oracle, cases):
    differs = 0
    for name, n in (("tiny-1", 1), ("tiny-4", 4), ("tiny-5", 5)):
        c = cases[name]
        assert len(c.items) == n
        if n > 1:  # the given order is not the ascending set order
            assert bc.trie_sorted(oracle, c.items) != c.items.tolist()
        m = oracle.Model(*c.aug)
        for v, size in c.note["tiny"].items():
            rows = c.train[1][c.train[0] == v]
            assert len(rows) == size
            if size > 1:  # the file order of a tiny row is not its trie order
                assert bc.trie_sorted(oracle, rows) != rows.tolist()
            differs += _bits([m.fresh_similarity(oracle.SIM_COSINE, v, c.q)]) != _bits([m.fresh_similarity(oracle.SIM_COSINE, c.q, v)])
    assert differs > 0


def test_item_only_the_newcomer_rates(oracle, cases):
    c = cases["new-item"]
    assert bc.NEW_ITEM in c.items.tolist() and bc.NEW_ITEM not in c.train[1].tolist()
    m = oracle.Model(*c.aug)
    lists = _lists(oracle, c, c.aug)
    off = on = 0
    for v in c.others:
        p = m.pipeline(oracle.SIM_COSINE, c.k).predict(v, bc.NEW_ITEM)
        mean = m.users_avg(v)
        if c.q in lists[v][0].tolist() and lists[v][1][lists[v][0].tolist().index(c.q)] != 0.0:
            on += _bits([p]) != _bits([mean])
        else:
            assert _bits([p]) == _bits([mean]), v
            off += 1
    assert on > 0 and off > 0


def test_average_shifts_and_answers_for_unknown_and_negative(oracle, cases):
    c = cases["off-scale"]
    m0, m1 = oracle.Model(*c.train), oracle.Model(*c.aug)
    assert _bits([m0.average()]) != _bits([m1.average()])
    neg = c.note["negative"]
    assert m1.users_avg(neg) < 0
    item = int(c.train[1][0])
    for v in (neg, bc.UNKNOWN_USER):
        assert _bits([m1.pipeline(oracle.SIM_COSINE, c.k).predict(v, item)]) == _bits([m1.average()]), v
    ids, sims = m1.pipeline(oracle.SIM_COSINE, c.k).neighbors(bc.UNKNOWN_USER)
    assert ids.tolist() == m1.user_iteration_order().tolist()[:c.k] and _bits(sims) == _bits(np.zeros(c.k))
    assert bc.UNKNOWN_USER in c.others and bc.UNKNOWN_USER not in c.aug[0].tolist()
