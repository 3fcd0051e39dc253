"""What knncf_remove_users rests on, from the oracle alone (no GPU).  The S-rule of include/knncf.h "Remove users": for every
fitted user v outside S — the leavers and every user whose list on train holds one — a fresh list of v on aug (train without
the leavers' rows) equals its list on train in ids and similarity bits, although the users behind a leaver move up by a dense
index, items may leave with it, and the file rows and the global and item averages move.  And what the inputs of
tests/remove_users_cases.py reach: a holder with the leaver in its first and one with it in its last cell, a cell beyond the
first 64, leavers at the edges of the 64-user words, an adjacent pair, the lone item that leaves, and the plain refits."""
import numpy as np
import pytest

from tests import remove_users_cases as ru
from tests import update_entered_cases as uc
from tests.bystander_cases import _users

SIMS = (ru.COS, ru.JAC)


def _check_s_rule(oracle, case, sim):
    """the holders, S and the quiet users of the case, whose lists on aug must be those on train"""
    before = ru.train_lists(oracle, case, sim)
    held = ru.holders(oracle, case, sim, before)
    s = ru.stale(oracle, case, sim, before)
    quiet = [v for v in _users(case.train) if v not in s]
    after = ru.ac.fresh_lists(oracle, case.aug, quiet, case.k, sim)
    for v in quiet:
        assert before[v] == after[v], (case.name, sim, v)
        assert not set(before[v][0]) & set(case.note["leavers"])
    return held, s, quiet


def test_aug_is_train_without_the_leavers_rows(synth):
    case = ru.two(synth, 5)
    gone = set(case.note["leavers"])
    keep = [x for x, u in enumerate(case.train[0].tolist()) if u not in gone]
    assert gone == {23, 41} and case.note["leavers"] == [41, 23] and len(case.users) == 0
    for a, b in zip(case.aug, case.train):
        assert a.tolist() == b[keep].tolist()
    assert _users(case.aug) == [v for v in _users(case.train) if v not in gone]
    # the removals are what knncf_amend needs for the same aug: every row of the leavers, nothing else
    assert sorted(zip(*(a.tolist() for a in case.removals))) == sorted((u, i) for u, i in zip(case.train[0].tolist(), case.train[1].tolist()) if u in gone)


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("who", [23, 5, 41])
def test_s_rule_one_leaver(synth, oracle, who, k, sim):
    case = ru.one(synth, who, k)
    held, s, quiet = _check_s_rule(oracle, case, sim)
    keep, gone = ru.split(oracle, case, sim, _users(case.train))
    assert keep == sorted(quiet) and set(gone) == s and keep and held and len(keep) + len(gone) == 60 and not ru.is_plain(case, sim)
    # the dropped ids stand in the old fit's set order, the leaver among them
    order = uc.dense_order(oracle, case.train)
    assert gone == [v for v in order if v in s] and who in gone


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("k", [5, 20, 57, 58])
def test_s_rule_two_leavers(synth, oracle, k, sim):
    """at k = 57 and 58 every list of the 60 users holds one of the two: nothing is quiet.  k = 57 is still no plain refit (58 users
    stay, the lists keep 57 cells); at k = 58 the stored length changes"""
    case = ru.two(synth, k)
    held, s, quiet = _check_s_rule(oracle, case, sim)
    assert ru.is_plain(case, sim) == (k == 58) and len(held) == len(s) - 2
    assert (quiet == []) if k >= 57 else len(quiet) > 5


@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("k", [5, 20])
def test_s_rule_random_leaver_sets(synth, oracle, k, sim):
    """a seeded loop of 40 leaver sets of 1 to 6 users"""
    rng = np.random.default_rng(20 + k)
    train = ru.base_train(synth)
    m = oracle.Model(*train)
    kind = ru.sim_kind(oracle, sim)
    before = {}
    for v in _users(train):  # (fresh pipelines, once for the 40 sets)
        ids, sims = m.pipeline(kind, k).neighbors(v)
        before[v] = (ids.tolist(), ru.ac._bits(sims))
    sizes = set()
    for n in range(40):
        case = ru.leaving(f"random-{n}", train, ru.random_leavers(rng, train), k)
        sizes.add(len(case.note["leavers"]))
        s = ru.stale(oracle, case, sim, before)
        quiet = [v for v in _users(train) if v not in s]
        after = ru.ac.fresh_lists(oracle, case.aug, quiet, k, sim)
        for v in quiet:
            assert before[v] == after[v], (case.name, sim, v, case.note["leavers"])
    assert sizes == {1, 2, 3, 4, 5, 6}


# ---- what the inputs reach ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("k", [5, 20])
def test_first_and_last_cell(synth, oracle, k, sim):
    """CELL_LEAVER stands in the first cell of one holder's list and in the last cell, kcap - 1, of another's"""
    case = ru.one(synth, ru.CELL_LEAVER, k)
    held, s, quiet = _check_s_rule(oracle, case, sim)
    cells = {p for at in held.values() for p in at}
    assert 0 in cells and k - 1 in cells and min(k, 59) == k and quiet


def test_long_lists_hold_the_leaver_beyond_the_first_64_cells(synth, oracle):
    case = ru.long_lists(synth, oracle)
    assert case.k == 100 and len(_users(case.train)) == 140 and len(case.note["leavers"]) == 1
    held, s, quiet = _check_s_rule(oracle, case, ru.COS)
    assert any(at == [p] and p >= 64 for at in held.values() for p in at) and any(at[0] < 64 for at in held.values())
    assert quiet and not ru.is_plain(case, ru.COS)


@pytest.mark.parametrize("n_users", ru.EDGE_NS)
def test_edge_fits(synth, oracle, n_users):
    """the leavers at dense 0, 63, 64 and last of fits of 63, 64, 65 and 129 users; 63 and 64 are adjacent where the fit has both"""
    case = ru.edge(synth, oracle, n_users)
    order = uc.dense_order(oracle, case.train)
    at = sorted(order.index(c) for c in case.note["leavers"])
    assert at == sorted({0, n_users - 1} | {x for x in (63, 64) if x < n_users}) and len(order) == n_users
    if n_users in (65, 129):
        assert 63 in at and 64 in at
    held, s, quiet = _check_s_rule(oracle, case, ru.COS)
    assert quiet and held and not ru.is_plain(case, ru.COS)
    # the users that stay keep their relative order, each moved up by the leavers in front of it
    new = uc.dense_order(oracle, case.aug)
    assert new == [v for v in order if v not in set(case.note["leavers"])]


def test_adjacent_pair(synth, oracle):
    case = ru.adjacent(synth, oracle)
    order = uc.dense_order(oracle, case.train)
    assert sorted(order.index(c) for c in case.note["leavers"]) == [30, 31]
    held, s, quiet = _check_s_rule(oracle, case, ru.COS)
    assert quiet and held and order[0] not in case.note["leavers"]


@pytest.mark.parametrize("sim", SIMS)
def test_the_lone_item_leaves_with_its_rater(synth, oracle, sim):
    case = ru.lone_rater(synth)
    items = set(np.unique(case.train[1]).tolist())
    assert (case.train[1] == ru.LONE_ITEM).sum() == 1 and case.train[0][case.train[1] == ru.LONE_ITEM].tolist() == case.note["leavers"]
    assert set(np.unique(case.aug[1]).tolist()) == items - {ru.LONE_ITEM}
    held, s, quiet = _check_s_rule(oracle, case, sim)
    assert quiet and held and not ru.is_plain(case, sim)


def test_carrying_cases_carry(synth, oracle):
    """every carrying case of test_gpu_remove_users.py has a kept list and a holder's dropped list (but k = 57 of its first group,
    where a list of 57 leaves out two of the 59 others: whatever is quiet there is carried, and nothing is asked of its number)"""
    cases = [ru.one(synth, 23, 5), ru.one(synth, 23, 20), ru.two(synth, 5), ru.two(synth, 20), ru.adjacent(synth, oracle),
             ru.long_lists(synth, oracle), ru.lone_rater(synth)] + [ru.edge(synth, oracle, n) for n in ru.EDGE_NS]
    for case in cases:
        keep, gone = ru.split(oracle, case, ru.COS, _users(case.train))
        assert keep and len(gone) > len(case.note["leavers"]) and not ru.is_plain(case, ru.COS), case.name
    keep, gone = ru.split(oracle, ru.short_row_fit(synth), ru.JAC, _users(ru.short_row_fit(synth).train))
    assert keep and len(gone) > 1


def test_plain_refit_inputs(synth):
    """each plain case is plain by the header's rule, and by that rule alone"""
    full = ru.one(synth, 23, 59)                                   # k = U - 1: the stored length changes
    assert ru.is_plain(full, ru.JAC) and not ru.is_plain(ru.one(synth, 23, 58), ru.JAC)
    short = ru.short_row_fit(synth)                                # a cosine fit with a user of 4 ratings, who stays
    counts = dict(zip(*np.unique(short.train[0], return_counts=True)))
    assert counts[ru.SHORT_USER] == 4 and ru.SHORT_USER in _users(short.aug) and min(c for u, c in counts.items() if u != ru.SHORT_USER) > 4
    assert ru.is_plain(short, ru.COS) and not ru.is_plain(short, ru.JAC)
    crowd = ru.crowd(synth)                                        # one leaver too many
    assert len(crowd.note["leavers"]) == ru.MAX_LEAVERS + 1 and len(_users(crowd.aug)) == 11 and ru.is_plain(crowd, ru.JAC)
    assert not ru.is_plain(ru.crowd(synth, ru.MAX_LEAVERS), ru.JAC) and not ru.is_plain(crowd, ru.JAC, max_leavers=10**6)
    four = ru.to_four_users()                                      # aug of 4 users
    assert len(_users(four.train)) == 5 and len(_users(four.aug)) == 4 and len(np.unique(four.aug[1])) >= 5
    assert np.unique(four.train[0], return_counts=True)[1].min() > 4 and ru.is_plain(four, ru.JAC)
    assert four.k == 2 and min(four.k, 3) == min(four.k, 4)        # (not through the stored length)
