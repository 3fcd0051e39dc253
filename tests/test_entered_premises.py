"""The inputs of tests/entered_cases.py reach the cases that entered queries (knncf_query_entered*) must get right, shown on the
oracle alone (no GPU): the number of entered users of every case, the set-order tie at the cut on both sides, lists that are
full and lists that grow, the empty answer, a pair whose bits depend on who owns it, an item unknown to train, a fitted user
with a negative mean — and the premise of the whole path: without a train user of <= 4 ratings, the lists a handle has stored
after any call history are the fresh-closure lists."""
import numpy as np
import pytest

from tests import bystander_cases as bc
from tests import entered_cases as ec
from tests.query_helpers import _bits


@pytest.fixture(scope="module")
def cases(synth, oracle):
    return {c.name: c for c in ec.all_cases(synth, oracle)}  # (no input raises OracleError)


@pytest.fixture(scope="module")
def answers(oracle, cases):
    return {(name, sim): ec.expected(oracle, c, sim) for name, c in cases.items() for sim in c.note["sims"]}


def test_every_case_is_there(cases):
    assert sorted(cases) == sorted(ec.NAMES)
    for name, c in cases.items():
        assert (len(np.unique(c.train[0])), len(np.unique(c.train[1]))) == (60, 80), name
        assert c.q not in c.train[0].tolist(), name


def test_entered_counts(cases, answers):
    """the figures the builders state, every one"""
    for name, c in cases.items():
        for sim, want in c.note["count"].items():
            assert len(answers[name, sim][0]) == want, (name, sim)
    have = {(name, sim) for name, c in cases.items() for sim in c.note["count"]}
    assert {("near-clone", ec.COS), ("near-clone", ec.JAC), ("near-clone-k1", ec.COS), ("short-59", ec.COS), ("short-300", ec.COS),
            ("anti-clone", ec.COS), ("anti-clone", ec.JAC), ("anti-clone-59", ec.COS), ("new-item", ec.COS), ("off-scale", ec.COS),
            ("tiny-1", ec.JAC), ("tiny-4", ec.JAC), ("tiny-5", ec.JAC)} <= have


def test_near_clone_at_k1(answers):
    users, _, pos, _ = answers["near-clone-k1", ec.COS]
    assert users.tolist() == [5, 25] and pos.tolist() == [0, 0]


def test_tie_at_the_cut_on_both_sides(cases, answers):
    c = cases["tie-before"]
    users, _, pos, disp = answers["tie-before", ec.COS]
    at = users.tolist().index(c.note["bystander"])
    assert (c.k, c.note["bystander"], c.note["copy_of"]) == (36, 6, 11)
    assert pos[at] == 35 and disp[at] == 11  # the last position; the copied user, which ties bitwise, is pushed out
    c = cases["tie-after"]
    assert (c.k, c.note["bystander"]) == (55, 1)
    assert 1 not in answers["tie-after", ec.COS][0].tolist()  # the copied user keeps the last cell


def test_full_lists_and_lists_that_grow(answers):
    for sim in (ec.COS, ec.JAC):
        users, _, _, disp = answers["short-59", sim]
        assert len(users) == 60 and (disp >= 0).all()  # k = U - 1: every list is full and loses its last entry
        users, _, _, disp = answers["short-300", sim]
        assert len(users) == 60 and (disp == -1).all()  # k >= U: every list grows


def test_users_come_in_set_order(oracle, cases, answers):
    order = oracle.Model(*cases["near-clone"].train).user_iteration_order().tolist()
    assert order != sorted(order)
    for key in (("near-clone", ec.COS), ("anti-clone-59", ec.COS), ("short-59", ec.JAC)):
        got = answers[key][0].tolist()
        assert got == [v for v in order if v in set(got)], key


def test_empty_and_selective_answers(answers):
    assert len(answers["anti-clone", ec.COS][0]) == 0
    assert 0 < len(answers["anti-clone-59", ec.COS][0]) < 60  # selective although k = U - 1


def test_tiny_newcomer_pair_depends_on_its_owner(oracle, cases, answers):
    """the pair (27, q): folded in the fitted user's order it is not the bits of the newcomer's own fold"""
    c = cases["tiny-newcomer"]
    assert c.note["seed"] == 15 and len(c.items) == 4
    assert bc.trie_sorted(oracle, c.items)[::-1] == c.items.tolist()
    users, sims, pos, _ = answers["tiny-newcomer", ec.COS]
    at = users.tolist().index(27)
    m = oracle.Model(*c.aug)
    assert pos[at] == 4
    assert _bits([sims[at]]) == _bits([0.3266729181053223]) == _bits([m.fresh_similarity(oracle.SIM_COSINE, 27, c.q)])
    assert _bits([m.fresh_similarity(oracle.SIM_COSINE, c.q, 27)]) == _bits([0.32667291810532234]) != _bits([sims[at]])


def test_unknown_item_counts_in_the_jaccard_denominator(oracle, cases, answers):
    c = cases["new-item"]
    assert bc.NEW_ITEM in c.items.tolist() and bc.NEW_ITEM not in c.train[1].tolist()
    users, sims, _, _ = answers["new-item", ec.JAC]
    assert len(users) > 0
    for v, s in zip(users.tolist(), sims.tolist()):
        mine = set(c.train[1][c.train[0] == v].tolist())
        both = len(mine & set(c.items.tolist()))
        assert s == both / (len(mine) + len(c.items) - both), v


def test_negative_mean_user_is_reported_like_any_other(oracle, cases, answers):
    c = cases["off-scale-59"]
    neg = c.note["negative"]
    assert neg == 8 and oracle.Model(*c.aug).users_avg(neg) < 0
    assert neg in answers["off-scale-59", ec.COS][0].tolist()
    assert neg not in answers["off-scale", ec.COS][0].tolist()  # at k = 5 its list has closer users, nothing else keeps it out


def test_tiny_rows_trains_have_short_users(cases):
    for name in ("tiny-1", "tiny-4", "tiny-5"):
        c = cases[name]
        assert c.note["sims"] == (ec.JAC,)  # the adjusted cosine on these trains is the refusal case
        assert sorted(np.unique(c.train[0], return_counts=True)[1].tolist())[:3] == [1, 3, 4]


@pytest.mark.parametrize("k", [5, 59, 300])
def test_stored_lists_are_fresh_closure_lists(synth, oracle, k):
    """the memo premise: on a train set whose users all have > 4 ratings, the lists ONE pipeline answers after a shuffled
    history of neighbour calls are those of a fresh pipeline per user, ids and similarity bits"""
    train = bc.base_train(synth)
    assert np.unique(train[0], return_counts=True)[1].min() > 4
    m = oracle.Model(*train)
    users = bc._users(train)
    one = m.pipeline(oracle.SIM_COSINE, k)
    for v in np.random.default_rng(k).permutation(users).tolist():
        one.neighbors(v)
    for v in users:
        got, want = one.neighbors(v), m.pipeline(oracle.SIM_COSINE, k).neighbors(v)
        assert got[0].tolist() == want[0].tolist() and _bits(got[1]) == _bits(want[1]), v
