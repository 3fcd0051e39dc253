"""The inputs of tests/update_bystander_cases.py reach the cases that knncf_update_bystander_* must get right, shown on the
oracle alone (no GPU): a fitted changer leaves, enters and moves inside other users' lists, its terms have an observable place,
deviation and similarity in a bystander's fold, it is the only rater of an item, it is summed in the bystander's order, it ties
on the cut in both set orders, and it shifts average(aug)."""
import numpy as np
import pytest

from tests import bystander_cases as bc
from tests import update_bystander_cases as uc
from tests.query_helpers import UNKNOWN_ITEM, _bits

NAMES = ["adds-3", "leaves-short-59", "leaves-short-300", "new-item", "negative", "fold-place", "tiny-changer", "tiny-bystanders",
         "tie-before", "tie-after"]


@pytest.fixture(scope="module")
def cases(synth, oracle):
    return {c.name: c for c in uc.all_cases(synth, oracle)}


def test_every_case_is_there(cases):
    assert sorted(cases) == sorted(NAMES)
    assert set(uc.JACCARD_CASES) <= set(NAMES)
    base = cases["adds-3"].train
    assert (len(np.unique(base[0])), len(np.unique(base[1])), len(base[0])) == (60, 80, 1200)
    for c in cases.values():  # the changer is of the fit, its additional items are new to it, and it is no bystander
        assert c.q in set(c.train[0].tolist()) and c.q not in c.others and bc.UNKNOWN_USER in c.others
        assert not set(c.items.tolist()) & set(c.train[1][c.train[0] == c.q].tolist())
        assert len(c.others) == 60


@pytest.mark.parametrize("sim_name, figures", [("cosine", (7, 2, 5, 2)), ("jaccard", (2, 2, 7, 5))])
def test_adds_3_leaves_enters_moves_and_stays(oracle, cases, sim_name, figures):
    """user 5 adds three ratings of 5.0, k = 5: the table of the feature's description, recomputed"""
    c = cases["adds-3"]
    sim = oracle.SIM_COSINE if sim_name == "cosine" else oracle.SIM_JACCARD
    ch = uc.list_changes(oracle, c, sim)
    assert (len(ch["leaves"]), len(ch["enters"]), len(ch["stays"]), len(ch["moves"])) == figures
    for v in ch["leaves"]:  # a full list: the user that comes in was not in the train list — only the full row knows it
        ia, ib, _, _ = ch["lists"][v]
        assert len(ia) == len(ib) == c.k
        new = [x for x in ib if x not in ia]
        assert len(new) == 1 and [x for x in ia if x != c.q] == [x for x in ib if x != new[0]], v
    put = [v for v in ch["stays"] if v not in ch["moves"]]
    assert put
    for v in put:  # stays put with a changed similarity
        ia, ib, sa, sb = ch["lists"][v]
        assert _bits([sa[ia.index(c.q)]]) != _bits([sb[ib.index(c.q)]]), v
    # nobody else's quantities move: a list without c on either side is the train list
    for v, (ia, ib, sa, sb) in ch["lists"].items():
        if c.q not in ia and c.q not in ib:
            assert ia == ib and _bits(sa) == _bits(sb), v


@pytest.mark.parametrize("name", ["leaves-short-59", "leaves-short-300"])
def test_short_lists_keep_their_length(oracle, cases, name):
    c = cases[name]
    ch = uc.list_changes(oracle, c, oracle.SIM_COSINE)
    assert not ch["leaves"] and not ch["enters"] and len(ch["stays"]) == 59 and ch["moves"]
    assert all(len(ia) == len(ib) == 59 for ia, ib, _, _ in ch["lists"].values())


def test_fold_place_slips_are_observable(oracle, synth):
    """the pure-Python left fold over an item's aug rows is the oracle's prediction (fold_place asserts it for every row it
    tries), and each planted slip about c's term changes the bits of some prediction: the search ends"""
    case, found = uc.fold_place(synth, oracle)
    assert sorted(found) == sorted(uc.SLIPS)
    assert case.k == 59 and case.q == uc.CHANGER
    mt = oracle.Model(*case.train)
    m = oracle.Model(*case.aug)
    for slip, (v, item) in found.items():
        want = m.pipeline(oracle.SIM_COSINE, case.k).predict(v, item)
        plain = uc.fold_predict(oracle, m.users_avg(v), [(dv, s) for (_, _, dv, s) in uc.fold_rows(oracle, case, oracle.SIM_COSINE, v, item)])
        bad = uc.fold_predict(oracle, m.users_avg(v), uc.slipped_terms(oracle, case, oracle.SIM_COSINE, v, item, slip, mt.normalized_deviations(),
                                                                      mt.pipeline(oracle.SIM_COSINE, case.k).knn_similarity(v, case.q)))
        assert _bits([plain]) == _bits([want]) and _bits([bad]) != _bits([want]), slip
    # c's train rows keep their file place: some witness item has a rater behind c's train row
    v, item = found["train-term-last"]
    rows = uc.fold_rows(oracle, case, oracle.SIM_COSINE, v, item)
    at = [x for x, r in enumerate(rows) if r[0] == case.q][0]
    assert at < len(rows) - 1 and rows[at][1] < len(case.train[0])


def test_new_item_has_one_term_or_none(oracle, cases):
    c = cases["new-item"]
    assert c.items.tolist() == [bc.NEW_ITEM] and bc.NEW_ITEM not in set(c.train[1].tolist())
    m = oracle.Model(*c.aug)
    dev = m.normalized_deviations()[-1]
    inside, outside = [], []
    for v in c.others[:-1]:
        ids, sims = m.pipeline(oracle.SIM_COSINE, c.k).neighbors(v)
        got = m.pipeline(oracle.SIM_COSINE, c.k).predict(v, bc.NEW_ITEM)
        avg = m.users_avg(v)
        if c.q in ids.tolist():
            s = float(sims[ids.tolist().index(c.q)])
            assert _bits([got]) == _bits([uc.fold_predict(oracle, avg, [(dev, s)])]), v
            if _bits([got]) != _bits([avg]):
                inside.append(v)
        else:
            assert _bits([got]) == _bits([avg]), v
            outside.append(v)
    assert inside and outside


def test_tiny_users_on_both_sides(oracle, cases):
    small, big = cases["tiny-changer"], cases["tiny-bystanders"]
    sizes = small.note["tiny"]
    assert sorted(sizes.values()) == [1, 3, 4]
    assert sizes[small.q] == 1 and len(small.items) == 2  # 3 rows on aug: still a Set3
    assert big.q not in sizes and (big.train[0] == big.q).sum() > 4
    for v, n in sizes.items():  # the changer shares items with every tiny bystander on aug
        mine = set(big.train[1][big.train[0] == v].tolist())
        assert mine & (set(big.items.tolist()) | set(big.train[1][big.train[0] == big.q].tolist())), v
    m = oracle.Model(*big.aug)
    assert big.note["differs"]
    for v in big.note["differs"]:
        assert _bits([m.fresh_similarity(oracle.SIM_COSINE, v, big.q)]) != _bits([m.fresh_similarity(oracle.SIM_COSINE, big.q, v)])


def test_tie_sits_on_the_cut_in_both_set_orders(oracle, cases):
    sides = set()
    for name in ("tie-before", "tie-after"):
        c = cases[name]
        v, w = c.note["bystander"], c.note["tied_with"]
        first = [x for x in oracle.Model(*c.aug).user_iteration_order().tolist() if x in (c.q, w)][0]
        assert (first == c.q) == (c.note["side"] == "before")
        sides.add(c.note["side"])
        m = oracle.Model(*c.aug)
        assert _bits([m.fresh_similarity(oracle.SIM_JACCARD, v, c.q)]) == _bits([m.fresh_similarity(oracle.SIM_JACCARD, v, w)])
        assert _bits([m.fresh_similarity(oracle.SIM_JACCARD, v, c.q)]) != _bits([oracle.Model(*c.train).fresh_similarity(oracle.SIM_JACCARD, v, c.q)])
        ids = m.pipeline(oracle.SIM_JACCARD, c.k).neighbors(v)[0].tolist()
        assert len(ids) == c.k and ids[-1] == first and ((c.q in ids) != (w in ids))
        longer = m.pipeline(oracle.SIM_JACCARD, c.k + 1).neighbors(v)[0].tolist()
        assert set(longer[-2:]) == {c.q, w}
    assert sides == {"before", "after"}


def test_negative_mean_and_unknown_bystanders(oracle, cases):
    c = cases["negative"]
    neg = c.note["negative"]
    m, mt = oracle.Model(*c.aug), oracle.Model(*c.train)
    assert m.users_avg(neg) < 0 and neg in c.others
    assert _bits([m.average()]) != _bits([mt.average()])
    item = int(c.train[1][0])
    assert _bits([m.pipeline(oracle.SIM_COSINE, c.k).predict(neg, item)]) == _bits([m.average()])
    assert _bits([m.pipeline(oracle.SIM_COSINE, c.k).predict(bc.UNKNOWN_USER, item)]) == _bits([m.average()])
    ids, sims = m.pipeline(oracle.SIM_COSINE, c.k).neighbors(neg)
    assert len(ids) == c.k and any(s != 0.0 for s in sims)  # an ordinary list
    ids, sims = m.pipeline(oracle.SIM_COSINE, c.k).neighbors(bc.UNKNOWN_USER)
    assert ids.tolist() == m.user_iteration_order().tolist()[:c.k] and not sims.any()
    assert UNKNOWN_ITEM in c.pred_items.tolist()
