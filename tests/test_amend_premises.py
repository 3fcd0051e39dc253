"""What knncf_amend rests on, from the oracle alone (no GPU).  The S-rule of include/knncf.h "Amend": for every fitted user v
outside S — the changers and the users knncf_revise_entered_batch reports for each changer on its own, with its removals — a
fresh list of v on the JOINT aug equals its list on train in ids and similarity bits, although the removals shift the file rows
of everyone behind them and move the global and the item averages.  And what the inputs of tests/amend_cases.py reach: a
carried and a dropped list in every carrying case; the lone item that leaves aug; the changer that falls to 4 rows; the user
that leaves the fit; the joint call's four kinds of changer."""
import numpy as np
import pytest

from tests import amend_cases as am
from tests import update_entered_cases as uc
from tests.bystander_cases import NEW_ITEM, _rows, _users
from tests.revise_bystander_cases import LONE_ITEM

SIMS = (am.COS, am.JAC)


def _check_s_rule(oracle, case, sim):
    fitted = _users(case.train)
    rep = am.reports(oracle, case, sim)
    s = am.stale(oracle, case, sim, rep)
    quiet = [v for v in fitted if v not in s]
    before, after = am.fresh_lists(oracle, case.train, quiet, case.k, sim), am.fresh_lists(oracle, case.aug, quiet, case.k, sim)
    for v in quiet:
        assert before[v] == after[v], (case.name, sim, v)
    return rep, s, quiet


def test_aug_is_train_without_the_removed_rows_then_the_rows(synth):
    case = am.joint(synth)
    u, i, r = case.aug
    n_kept = len(case.train[0]) - len(case.removed_users)
    assert len(u) == n_kept + len(case.users) and u[n_kept:].tolist() == case.users.tolist()
    pairs = list(zip(u[:n_kept].tolist(), i[:n_kept].tolist()))
    gone = set(zip(*(a.tolist() for a in case.removals)))
    assert pairs == [p for p in zip(case.train[0].tolist(), case.train[1].tolist()) if p not in gone] and len(gone) == 5


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("build", [am.removes_3, am.re_rates, am.same_value])
@pytest.mark.parametrize("k", [5, 20])
def test_s_rule_single_changer(synth, oracle, k, build, sim):
    case = build(synth, k)
    rep, s, quiet = _check_s_rule(oracle, case, sim)
    keep, gone = am.split(oracle, case, sim, _users(case.train), rep)
    # a carried list and a dropped list both exist; same-value is an ordinary change: lists are dropped there too
    assert keep == sorted(quiet) and set(gone) == s and len(keep) > 5 and len(gone) > 1 and len(keep) + len(gone) == 60
    assert not am.is_plain(case, sim)


@pytest.mark.parametrize("sim", SIMS)
def test_s_rule_joint(synth, oracle, sim):
    case = am.joint(synth)
    rep, s, quiet = _check_s_rule(oracle, case, sim)
    assert [c for c, _, _, _ in case.changers] == [5, am.NEWCOMER, am.THIRD, am.SECOND] and not am.is_plain(case, sim)
    kinds = {c: (len(rm) > 0, len(it) > 0) for c, rm, it, _ in case.changers}
    assert kinds == {5: (True, True), am.SECOND: (True, False), am.THIRD: (False, True), am.NEWCOMER: (False, True)}
    assert am.NEWCOMER not in _users(case.train) and {5, am.SECOND, am.THIRD} <= set(_users(case.train))
    # user 5 rates one of its removed items again, the rows interleave, the removals alternate between the removers
    mine = case.changers[0]
    assert len(set(mine[1].tolist()) & set(mine[2].tolist())) == 1 and len(set(case.users[:3].tolist())) == 3
    assert case.removed_users.tolist() == [5, am.SECOND, 5, am.SECOND, 5]
    assert NEW_ITEM not in set(case.train[1].tolist()) and NEW_ITEM in set(case.aug[1].tolist())
    assert len(quiet) > 5 and len(s) > 8


@pytest.mark.parametrize("sim", SIMS)
def test_zero_weight_user_is_kept(synth, oracle, sim):
    case = am.zero_weight(synth)
    assert case.k == len(_users(case.train)) - 1 and not am.is_plain(case, sim)
    rep, s, quiet = _check_s_rule(oracle, case, sim)
    assert quiet == [case.note["planted"]]


@pytest.mark.parametrize("sim", SIMS)
def test_the_lone_item_leaves_and_changes_no_list(synth, oracle, sim):
    removed, rerated, kept = am.lone_item(synth, 5)
    items = set(np.unique(removed.train[1]).tolist())
    assert LONE_ITEM in items and (removed.train[1] == LONE_ITEM).sum() == 1
    assert set(np.unique(removed.aug[1]).tolist()) == items - {LONE_ITEM}
    assert set(np.unique(rerated.aug[1]).tolist()) == items and rerated.aug[1][-1] == LONE_ITEM
    assert set(np.unique(kept.aug[1]).tolist()) == items
    for case in (removed, rerated, kept):
        _, s, quiet = _check_s_rule(oracle, case, sim)
        assert quiet and not am.is_plain(case, sim)


def test_keeps_4_falls_to_four_rows(synth, oracle):
    case = am.keeps_4(synth, 5)
    c = case.note["changer"]
    assert len(_rows(case.train, c)[0]) > 8 and len(_rows(case.aug, c)[0]) == 4
    assert am.is_plain(case, am.COS) and not am.is_plain(case, am.JAC)
    _, s, quiet = _check_s_rule(oracle, case, am.JAC)
    assert quiet and len(s) > 1


def test_the_leaver_shrinks_the_user_set(synth):
    case = am.leaver(synth, 5)
    who = case.note["leaver"]
    assert who in _users(case.train) and _users(case.aug) == [v for v in _users(case.train) if v != who]
    assert len(case.users) == 0 and am.is_plain(case, am.JAC) and am.is_plain(case, am.COS)


def test_plain_refit_inputs(synth):
    train = am.base_train(synth)
    assert am.is_plain(am.with_newcomer(synth, train, 60), am.JAC) and not am.is_plain(am.with_newcomer(synth, train, 59), am.JAC)
    crowd = am.crowd(synth, 129)
    assert len(crowd.removers) == 129 == len(crowd.changers) and not am.is_plain(crowd, am.COS)  # (the changer count decides, not the inputs' shape)


@pytest.mark.parametrize("n_users", uc.EDGE_FITS)
def test_edge_fits(synth, oracle, n_users):
    """the removers stand at dense 63, 64 and last of the old fit, the newcomer moves the last user by one — into a new 64-user word
    where the fit has 64 or 128 — and the S-rule holds at a selective k"""
    case = am.edge_fit(synth, oracle, n_users, 7)
    old = uc.dense_order(oracle, case.train)
    new = oracle.Model(*case.aug).user_iteration_order().tolist()
    assert [old.index(c) for c in case.note["at"]] == uc.edge_indices(n_users) == [old.index(c) for c in case.removers]
    assert len(new) == n_users + 1 and new.index(old[-1]) == n_users
    assert np.unique(case.aug[0], return_counts=True)[1].min() > 4
    _, s, quiet = _check_s_rule(oracle, case, am.COS)
    assert len(quiet) > 0 and set(case.note["at"]) <= s
