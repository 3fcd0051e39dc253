"""What knncf_append rests on, from the oracle alone (no GPU).  The S-rule of include/knncf.h "Append": for every fitted user v
outside S — the changers and the users knncf_update_entered_batch reports for each changer on its own — a fresh list of v on the
JOINT aug equals its list on train in ids and similarity bits.  And what the inputs of tests/append_cases.py reach: a user in
K; users dropped because a changer entered, left (always a tail row) or as a tail row that stays; a joint append in which a user
is reported for exactly one changer; a newcomer in the middle of the set order, so that dense ids shift; a new item; the
zero-weight user that stays in K at k = U - 1; the mask-word edges of the fixed-size fits."""
import numpy as np
import pytest

from tests import append_cases as ac
from tests import update_entered_cases as uc
from tests.bystander_cases import NEW_ITEM, _users

SIMS = (ac.COS, ac.JAC)


def _check_s_rule(oracle, case, sim):
    fitted = _users(case.train)
    rep = ac.reports(oracle, case, sim)
    s = ac.stale(oracle, case, sim, rep)
    quiet = [v for v in fitted if v not in s]
    before, after = ac.fresh_lists(oracle, case.train, quiet, case.k, sim), ac.fresh_lists(oracle, case.aug, quiet, case.k, sim)
    for v in quiet:
        assert before[v] == after[v], (case.name, sim, v)
    return rep, s, quiet


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("k", [5, 20])
def test_s_rule_single_changer(synth, oracle, k, sim):
    case = ac.adds_3(synth, k)
    rep, s, quiet = _check_s_rule(oracle, case, sim)
    kinds = set(rep[case.changers[0][0]].values())
    assert {"entered", "left"} <= kinds and len(quiet) > 10  # (a user that the changer left is a tail row: test_update_entered_premises)
    keep, gone = ac.split(oracle, case, sim, _users(case.train))
    assert keep == sorted(quiet) and set(gone) == s and len(keep) + len(gone) == 60


def test_a_tail_row_that_stays_is_dropped(synth, oracle):
    """adds-3 at k = 20 has a reported user in whose list the changer keeps the last cell (ADDS_COUNTS of
    test_update_entered_premises): the stored list cannot tell, the row is in S"""
    case = ac.adds_3(synth, 20)
    c, it, rt = case.changers[0]
    out, kinds, _ = uc.expected_for(oracle, case.train, c, it, rt, 20, ac.COS, with_kinds=True)
    rows, _ = uc.lists_of(oracle, case.train, c, it, rt, 20, ac.COS)
    lists = {v: (a, b) for v, a, b in rows}
    stay = [int(v) for v, p, pr in zip(out[0], out[2], out[3]) if p >= 0 and uc.is_tail(20, int(pr), int(p), *lists[int(v)], c)]
    assert stay and set(stay) <= ac.stale(oracle, case, ac.COS)


@pytest.mark.parametrize("sim", SIMS)
def test_s_rule_joint(synth, oracle, sim):
    case = ac.joint(synth)
    rep, s, quiet = _check_s_rule(oracle, case, sim)
    assert [c for c, _, _ in case.changers] == [5, ac.NEWCOMER, ac.SECOND] and not ac.is_plain(case, sim)
    # the rows interleave
    assert len(set(case.users[:3].tolist())) == 3
    # some user is reported for exactly one changer, and some user for none
    once = [v for v in _users(case.train) if sum(v in r for r in rep.values()) == 1 and v not in rep]
    assert once and len(quiet) > 5
    # the newcomer stands in the middle of the set order: the dense ids behind it shift
    order = oracle.Model(*case.aug).user_iteration_order().tolist()
    at = order.index(ac.NEWCOMER)
    assert 0 < at < len(order) - 1 and [v for v in order if v != ac.NEWCOMER] == oracle.Model(*case.train).user_iteration_order().tolist()
    assert any(order.index(v) > at for v in quiet) and any(order.index(v) < at for v in quiet)
    # a new item, rated by a newcomer and by a fitted changer
    assert NEW_ITEM not in set(case.train[1].tolist()) and sorted(set(case.users[case.items == NEW_ITEM].tolist())) == [ac.SECOND, ac.NEWCOMER]


@pytest.mark.parametrize("sim", SIMS)
def test_zero_weight_user_is_kept(synth, oracle, sim):
    case = ac.zero_weight(synth)
    assert case.k == len(_users(case.train)) - 1 and not ac.is_plain(case, sim)
    rep, s, quiet = _check_s_rule(oracle, case, sim)
    assert quiet == [case.note["planted"]]


def test_plain_refit_inputs(synth):
    train = ac.base_train(synth)
    assert ac.is_plain(ac.with_newcomer(synth, train, 60), ac.JAC) and ac.is_plain(ac.with_newcomer(synth, train, 300), ac.JAC)
    assert not ac.is_plain(ac.with_newcomer(synth, train, 59), ac.JAC)  # (lists of 59 stay lists of 59 among 60 others)
    four = ac.with_newcomer(synth, train, 5, n=4)
    assert ac.is_plain(four, ac.COS) and not ac.is_plain(four, ac.JAC)


@pytest.mark.parametrize("n_users", uc.EDGE_FITS)
def test_edge_fits(synth, oracle, n_users):
    """the changers stand at dense 63, 64 and last of the old fit; the newcomer goes in front of some of them, so their rows move
    by one — across the 64-user word where the fit has that many; and the S-rule holds at a selective k"""
    case = ac.edge_fit(synth, oracle, n_users, 7)
    old = uc.dense_order(oracle, case.train)
    new = oracle.Model(*case.aug).user_iteration_order().tolist()
    assert [old.index(c) for c in case.note["at"]] == uc.edge_indices(n_users) and len(new) == n_users + 1
    at = new.index(ac.NEWCOMER)
    assert at < n_users - 1 and new.index(old[-1]) == n_users  # the last user moved; n_users = 64, 128: into a new word
    _, s, quiet = _check_s_rule(oracle, case, ac.COS)
    assert len(quiet) > 0 and set(case.note["at"]) <= s
