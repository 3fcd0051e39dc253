"""The premises of tests/test_gpu_revise.py, from the oracle alone (no GPU): the queries of tests/revise_cases.py mean
something.  For every removal case the oracle's answer on aug (the user's removed rows taken out) differs in at least one bit
from its answer on train ++ the additional rows — so an implementation that ignores the removals fails the GPU tests — and the
hand set holds the rows the row-size and lone-item cases claim."""
import numpy as np
import pytest

from tests import revise_cases as rc


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64).tolist()


def _answer(oracle, data, q, sim, k, items):
    """neighbour ids, similarity bits, prediction bits on `data`; None when the oracle refuses it (a repeated (user, item))"""
    try:
        p = oracle.Model(*data).pipeline(sim, k)
        ids, sims = p.neighbors(q)
    except oracle.OracleError:
        return None
    return ids.tolist(), _bits(sims), _bits([p.predict(q, int(i)) for i in items])


def _differs(oracle, train, q, removed, items, ratings, sim, k):
    probe = rc.pred_items(train, q, removed, items)[::5]
    want = _answer(oracle, rc.aug_of(train, q, removed, items, ratings), q, sim, k, probe)
    assert want is not None
    ignored = _answer(oracle, rc.appended(train, q, items, ratings), q, sim, k, probe)
    return ignored is None or ignored != want


def _sound(train, q, removed, items, ratings):
    """the query is answerable: no negative mean, no zero scale() (a rating equal to the mean of the user's rows in aug is fine:
    scale is 1 there; the deviations are finite whenever the ratings lie in the scale's range)"""
    u, i, r = rc.aug_of(train, q, removed, items, ratings)
    mine = r[u == q]
    assert len(mine) > 0 and np.isfinite(mine).all()
    avg = mine.sum() / len(mine)
    assert avg > 0
    for x in mine:  # scale(x, avg) :155-169
        s = 5.0 - avg if x > avg else (avg - 1.0 if x < avg else 1.0)
        assert s != 0.0, (q, x, avg)
    assert len(set(i[u == q].tolist())) == len(mine)  # no repeated item in aug


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("case", rc.CASES)
def test_removals_change_the_cosine_answer_syn100k(oracle, syn100k, case, shuffled):
    train = rc.syn100k(syn100k, shuffled)
    for q in rc.pick_users(train):
        assert int((train[0] == q).sum()) >= 6
        removed, items, ratings = rc.case_query(train, q, case, dyadic=not shuffled)
        _sound(train, q, removed, items, ratings)
        assert len(removed) == {"delete1": 1, "delete3": 3, "rerate": 2, "mixed": 3}[case]
        assert _differs(oracle, train, q, removed, items, ratings, oracle.SIM_COSINE, 10), (q, case)


def test_removals_change_the_jaccard_answer_syn100k(oracle, syn100k):
    train = rc.syn100k(syn100k)
    for n, q in enumerate(rc.pick_users(train)[:5]):
        removed, items, ratings = rc.case_query(train, q, "mixed", unknown=n == 2)
        _sound(train, q, removed, items, ratings)
        assert (rc.UNKNOWN_ITEM in items.tolist()) == (n == 2)
        assert _differs(oracle, train, q, removed, items, ratings, oracle.SIM_JACCARD, 50), q


def test_hand_set_rows(oracle):
    train = rc.small_set()
    u, i, r = train
    assert len(np.unique(u)) == 40
    # the item whose only rater is the query user
    assert u[i == rc.LONE_ITEM].tolist() == [rc.LONE_USER]
    qs = rc.small_queries(train)
    rows_in = lambda q: int((u == q).sum())
    rows_aug = lambda name: int((rc.aug_of(train, *qs[name])[0] == qs[name][0]).sum())
    # 6 train rows, 4 removed, 2 added: <= 4 rows in aug while > 4 in train; "2 train rows survive + 2 additional"
    for name in ("into_small_a", "into_small_b"):
        assert rows_in(8) == 6 and len(qs[name][1]) == 4 and len(qs[name][2]) == 2 and rows_aug(name) == 4
    assert qs["into_small_a"][2].tolist() == qs["into_small_b"][2][::-1].tolist()
    assert rows_in(7) == 3 and rows_aug("out_of_small") == 5
    assert rows_in(9) == len(qs["all_removed"][1]) == 4 and rows_aug("all_removed") == 2
    assert len(np.unique(rc.aug_of(train, *qs["all_removed"])[0])) == 40  # still a user of aug
    # the lone item leaves aug when removed, stays when re-rated
    assert rc.LONE_ITEM not in rc.aug_of(train, *qs["lone_item_removed"])[1].tolist()
    assert rc.LONE_ITEM in rc.aug_of(train, *qs["lone_item_rerated"])[1].tolist()
    # users with 1-5 ratings are among everybody's candidates
    assert sorted(rows_in(x) for x in (1, 2, 3, 4, 5, 6)) == [1, 2, 2, 3, 4, 4]
    for name, (q, removed, items, ratings) in qs.items():
        _sound(train, q, removed, items, ratings)
        assert set(removed.tolist()) <= set(i[u == q].tolist()), name
        for sim in (oracle.SIM_COSINE, oracle.SIM_JACCARD):
            assert _differs(oracle, train, q, removed, items, ratings, sim, 10), (name, sim)


def test_given_order_matters_in_the_small_class(oracle):
    """the two orders of the additional rows of the <= 4-row case are different inputs: the oracle's cosine similarities
    differ in at least one bit, so the given-order folding is observable"""
    train = rc.small_set()
    qs = rc.small_queries(train)
    a = _answer(oracle, rc.aug_of(train, *qs["into_small_a"]), 8, oracle.SIM_COSINE, 64, [1])
    b = _answer(oracle, rc.aug_of(train, *qs["into_small_b"]), 8, oracle.SIM_COSINE, 64, [1])
    assert a is not None and b is not None and a != b
