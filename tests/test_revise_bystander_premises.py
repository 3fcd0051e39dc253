"""The inputs of tests/revise_bystander_cases.py reach what they are named for — on the CPU, with the oracle alone, so that a case
that stops reaching its target fails here and not silently on the GPU."""
import numpy as np
import pytest

from tests import revise_bystander_cases as rc
from tests.bystander_cases import UNKNOWN_USER, _rows
from tests.query_helpers import _bits


@pytest.fixture(scope="module")
def cases(synth, oracle):
    return {c.name: c for c in rc.all_cases(synth, oracle)}


def test_the_names_are_the_cases(cases):
    assert list(cases) == rc.NAMES
    for c in cases.values():
        assert UNKNOWN_USER in c.others and c.q not in c.others and len(c.others) == 60
        mine = _rows(c.train, c.q)[0].tolist()
        assert len(c.removed) > 0 and all(int(x) in mine for x in c.removed) and len(set(c.removed.tolist())) == len(c.removed)
        assert len(c.aug[0]) == len(c.train[0]) - len(c.removed) + len(c.items)


def test_removes_3_takes_the_first_and_the_last_file_row(cases):
    for k in (5, 59, 300):
        c = cases[f"removes-3-k{k}"]
        mine = _rows(c.train, c.q)[0]
        assert c.k == k and len(c.items) == 0 and c.removed.tolist() == [mine[0], mine[len(mine) // 2], mine[-1]]
        assert rc.is_dyadic(c.train)


def test_re_rates_every_slip_changes_some_prediction(synth, oracle):
    case, found = rc.re_rates(synth, oracle)
    assert case.k == 59 and not rc.is_dyadic(case.train)
    rerated = set(case.removed.tolist()) & set(case.items.tolist())
    assert len(rerated) == 2 and len(case.removed) == 3 and len(case.items) == 3
    assert sorted(found) == sorted(rc.SLIPS)
    train_dev = oracle.Model(*case.train).normalized_deviations()
    m = oracle.Model(*case.aug)
    for slip, (v, item) in found.items():
        rows = rc.fold_terms(oracle, case, oracle.SIM_COSINE, v, item)
        want = m.pipeline(oracle.SIM_COSINE, 59).predict(v, item)
        assert _bits([rc.fold_predict(oracle, m.users_avg(v), [(dv, s) for (_, dv, s) in rows])]) == _bits([want])
        assert _bits([rc.fold_predict(oracle, m.users_avg(v), rc.slipped_terms(case, rows, item, slip, train_dev))]) != _bits([want]), slip
        assert (item in rerated) == (slip in ("rerated-at-train-row", "rerated-first")) or slip in ("removed-still-a-term", "train-deviation")


def test_re_rates_dyadic(cases):
    c = cases["re-rates-dyadic"]
    assert rc.is_dyadic(c.train) and set(c.removed.tolist()) < set(c.items.tolist()) and len(c.items) == 3
    u, i, r = c.train
    for it, rt in zip(c.items, c.ratings):
        old = r[(u == c.q) & (i == it)]
        assert len(old) == 0 or old[0] != rt


def test_off_scale_the_running_total_is_no_shortcut(cases, oracle):
    c = cases["off-scale"]
    at = np.flatnonzero(c.train[0] == c.q)
    assert c.removed.tolist() == [c.train[1][at[0]], c.train[1][at[-1]]] and len(c.items) == 2
    assert not rc.is_dyadic(c.train) and c.note["negative"] in c.others
    assert oracle.Model(*c.aug).users_avg(c.note["negative"]) < 0
    assert _bits([rc.shortcut_average(c)]) != _bits([oracle.Model(*c.aug).average()])
    for name in ("removes-3-k5", "re-rates-dyadic", "lone-item-rerated"):  # the same shortcut on the dyadic fit is exact
        d = cases[name]
        assert _bits([rc.shortcut_average(d)]) == _bits([oracle.Model(*d.aug).average()]), name
    # the oracle answers average(aug) for the bystander unknown to aug and for the negative-mean one
    m = oracle.Model(*c.aug)
    for v in (UNKNOWN_USER, c.note["negative"]):
        assert _bits([m.pipeline(oracle.SIM_COSINE, c.k).predict(v, int(c.train[1][0]))]) == _bits([m.average()])


def test_lone_item(cases, oracle):
    gone, again, kept = cases["lone-item-removed"], cases["lone-item-rerated"], cases["lone-item-kept"]
    train = gone.train
    assert (train[1] == rc.LONE_ITEM).sum() == 1 and train[0][train[1] == rc.LONE_ITEM][0] == gone.q
    at = int(np.flatnonzero(train[1] == rc.LONE_ITEM)[0])
    mine = np.flatnonzero(train[0] == gone.q)
    assert mine[0] < at < mine[-1]
    assert rc.LONE_ITEM not in gone.aug[1] and (again.aug[1] == rc.LONE_ITEM).sum() == 1 and again.aug[1][-1] == rc.LONE_ITEM
    assert rc.LONE_ITEM in kept.aug[1] and rc.LONE_ITEM not in kept.removed
    m = oracle.Model(*gone.aug)
    for sim in (oracle.SIM_COSINE, oracle.SIM_JACCARD):
        for v in gone.others[:20]:  # the item that left: the bystander's mean, bit for bit
            assert _bits([m.pipeline(sim, gone.k).predict(v, rc.LONE_ITEM)]) == _bits([m.users_avg(v)]), v
    # re-rated: the one-term fold where c is in v's list, v's mean otherwise
    ma = oracle.Model(*again.aug)
    dev = ma.normalized_deviations()[-1]
    inside = outside = 0
    for v in again.others[:-1]:
        p = ma.pipeline(oracle.SIM_COSINE, again.k)
        ids, sims = p.neighbors(v)
        got = ma.pipeline(oracle.SIM_COSINE, again.k).predict(v, rc.LONE_ITEM)
        if again.q in ids.tolist() and sims[ids.tolist().index(again.q)] != 0.0:
            s = float(sims[ids.tolist().index(again.q)])
            assert _bits([got]) == _bits([rc.fold_predict(oracle, ma.users_avg(v), [(float(dev), s)])]), v
            inside += 1
        else:
            assert _bits([got]) == _bits([ma.users_avg(v)]), v
            outside += 1
    assert inside > 0 and outside > 0


def test_membership_moves_both_ways(cases, oracle):
    c = cases["membership"]
    leaves, enters = rc.list_changes(oracle, c, oracle.SIM_COSINE)
    assert leaves and enters and leaves == c.note["leaves"] and enters == c.note["enters"]
    assert c.k == 5 and len(c.items) == 0


def test_tiny_leaves_the_changer_four_rows(cases):
    c = cases["tiny"]
    assert (c.aug[0] == c.q).sum() == 4 and (c.train[0] == c.q).sum() > 6
    sizes = sorted((c.train[0] == u).sum() for u in c.note["tiny"])
    assert sizes == [1, 3, 4] and all(u in c.others for u in c.note["tiny"])
