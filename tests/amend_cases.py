"""Inputs and expected answers of the tests of knncf_amend (removals and re-ratings into the fit, the unchanged kNN lists kept),
shared by test_amend_premises.py (CPU, oracle only: the inputs reach the cases and the S-rule holds) and test_gpu_amend.py.

A case is an Amend: the train set, the removals (user, item) in the given order, the rows in file order (rows of several users
may interleave), and the handle's k.  aug = train in file order without the removed rows ++ the rows: revise_cases.aug_of for
several changers.  The builders are those of revise_entered_cases (one changer with removals) and append_cases (several
changers, a newcomer, the fixed-size fits), put into one call."""
import sys
from dataclasses import dataclass, field

import numpy as np

from tests import append_cases as ac
from tests import bystander_cases as bc
from tests import revise_entered_cases as rc
from tests import update_bystander_cases as ub
from tests import update_entered_cases as uc
from tests.append_cases import NEWCOMER, SECOND, fresh_lists, interleave  # noqa: F401  (re-exported)
from tests.bystander_cases import NEW_ITEM, _rows, _users, base_train
from tests.entered_cases import COS, JAC, sim_kind  # noqa: F401  (re-exported)

THIRD = 41  # the fitted changer of the joint case that only adds


@dataclass
class Amend:
    name: str
    train: tuple               # (users, items, ratings), file order
    removed_users: np.ndarray  # the removals, in the order the call gives them
    removed_items: np.ndarray
    users: np.ndarray          # the rows, file order
    items: np.ndarray
    ratings: np.ndarray
    k: int
    note: dict = field(default_factory=dict)

    @property
    def removals(self):
        return self.removed_users, self.removed_items

    @property
    def rows(self):
        return self.users, self.items, self.ratings

    @property
    def call(self):
        """the arguments of amend() below"""
        return (*self.removals, *self.rows)

    @property
    def kept(self):
        """the train rows that go into aug, as a mask over the file"""
        gone = set(zip(self.removed_users.tolist(), self.removed_items.tolist()))
        return np.asarray([(u, i) not in gone for u, i in zip(self.train[0].tolist(), self.train[1].tolist())], dtype=bool)

    @property
    def aug(self):
        keep = self.kept
        return (np.concatenate([self.train[0][keep], self.users]).astype(np.int32),
                np.concatenate([self.train[1][keep], self.items]).astype(np.int32),
                np.concatenate([self.train[2][keep], self.ratings]).astype(np.float64))

    @property
    def changers(self):
        """the distinct users of the rows and of the removals, each as its revise query (c, removed items, items, ratings)"""
        out = []
        for c in dict.fromkeys(self.users.tolist() + self.removed_users.tolist()):
            at = self.users == c
            out.append((int(c), self.removed_items[self.removed_users == c].copy(), self.items[at].copy(), self.ratings[at].copy()))
        return out

    @property
    def removers(self):
        return [c for c, rm, _, _ in self.changers if len(rm)]


def _amend(name, train, removals, rows, k, **note):
    ru, ri = removals
    u, i, r = rows
    return Amend(name, train, np.asarray(ru, dtype=np.int32), np.asarray(ri, dtype=np.int32), np.asarray(u, dtype=np.int32),
                 np.asarray(i, dtype=np.int32), np.asarray(r, dtype=np.float64), k, dict(note))


def of_case(case):
    """a revise_bystander_cases.RCase (one changer q with its removals and rows) as an Amend"""
    return _amend(case.name, case.train, (np.full(len(case.removed), case.q), case.removed),
                  (np.full(len(case.items), case.q), case.items, case.ratings), case.k, changer=case.q, **case.note)


def removes_3(synth, k):
    return of_case(rc.removes_3(synth, k))


def re_rates(synth, k):
    return of_case(rc.re_rates(synth, k))


def same_value(synth, k):
    return of_case(rc.same_value(synth, k))


def keeps_4(synth, k):
    return of_case(rc.keeps_4(synth, k))


def lone_item(synth, k):
    """[removed, re-rated, kept] of revise_entered_cases.lone_item"""
    return [of_case(c) for c in rc.lone_item(synth, k)]


def zero_weight(synth):
    return of_case(rc.zero_weight(synth))


def joint(synth, k=5):
    """four changers in one call: user 5 removes three train rows and rates one of them again, user 23 only removes, user 41 only
    adds (one of its rows on an item unknown to train) and a newcomer joins (append_cases.joint's).  The rows interleave and the
    removals come in a shuffled order"""
    train = base_train(synth)
    nc = bc.near_clone(synth, k=k, q=NEWCOMER, train=train)
    mine, vals = _rows(train, ub.CHANGER)
    gone_a = mine[[1, 4, len(mine) - 2]]
    a = (ub.CHANGER, np.concatenate([gone_a[:1], ub.unrated(train, ub.CHANGER, 1)]).astype(np.int32), np.asarray([float(vals[1] - 2 if vals[1] >= 3 else vals[1] + 2), 4.5]))
    gone_b = rc.removed_rows(train, SECOND, 2)
    c = (THIRD, np.concatenate([ub.unrated(train, THIRD, 2), [NEW_ITEM]]).astype(np.int32), np.asarray([1.0, 5.0, 3.5]))
    q = (NEWCOMER, nc.items, nc.ratings)
    removals = [(ub.CHANGER, int(gone_a[2])), (SECOND, int(gone_b[1])), (ub.CHANGER, int(gone_a[0])), (SECOND, int(gone_b[0])), (ub.CHANGER, int(gone_a[1]))]
    return _amend(f"joint-k{k}", train, tuple(zip(*removals)), interleave([a, q, c]), k, newcomer=NEWCOMER, fitted=[ub.CHANGER, SECOND, THIRD])


def edge_fit(synth, oracle, n_users, k):
    """uc.scaled(n_users) with the removers at dense 63, 64 (where the fit has it) and last: each removes three train rows, the first
    of them rates one again; plus append_cases.edge_fit's newcomer, so that the table moves across the 64-user words"""
    train = uc.scaled(synth, n_users)
    order = uc.dense_order(oracle, train)
    at = [order[x] for x in uc.edge_indices(n_users)]
    removals = [(c, int(i)) for c in at for i in rc.removed_rows(train, c, 3)]
    nc = bc.near_clone(synth, k=k, q=NEWCOMER, train=train)
    parts = [(at[0], np.asarray([removals[0][1]], dtype=np.int32), np.asarray([2.5])), (NEWCOMER, nc.items, nc.ratings)]
    return _amend(f"edge-{n_users}", train, tuple(zip(*removals)), interleave(parts), k, newcomer=NEWCOMER, at=at)


def with_newcomer(synth, train, k, n=None):
    """append_cases.with_newcomer beside one removal of user 5"""
    base = ac.with_newcomer(synth, train, k, n=n)
    return _amend(base.name + "-and-a-removal", train, ([ub.CHANGER], [int(_rows(train, ub.CHANGER)[0][2])]), base.rows, k, newcomer=NEWCOMER)


def leaver(synth, k, who=SECOND):
    """every train row of a fitted user removed, no row given: the user leaves the fit"""
    train = base_train(synth)
    mine = _rows(train, who)[0]
    return _amend(f"leaver-{who}", train, (np.full(len(mine), who), mine), ([], [], []), k, leaver=who)


def crowd(synth, n_removers, k=5):
    """n_removers fitted users (update_entered_cases.scaled(EDGE_USERS)) with one removal each"""
    train = uc.scaled(synth, uc.EDGE_USERS)
    who = _users(train)[:n_removers]
    assert len(who) == n_removers
    return _amend(f"crowd-{n_removers}", train, (who, [int(_rows(train, c)[0][1]) for c in who]), ([], [], []), k)


# ---- the call --------------------------------------------------------------------------------------------------------------------
def amend(e, removed_users, removed_items, users, items, ratings, return_dropped=False):
    """knncf_amend on Engine e through the binding's Appends.amend: (carried, dropped_count[, the dropped raw ids]); a refusal
    raises the binding's error"""
    kn = sys.modules[type(e).__module__]
    return kn.Appends(e).amend(removed_users, removed_items, users, items, ratings, return_dropped=return_dropped)


# ---- the oracle's side -----------------------------------------------------------------------------------------------------------
def reports(oracle, case, sim):
    """{changer: the fitted users knncf_revise_entered_batch reports for (changer, its removals, its rows of the call in order) on
    train}, each changer on its own, with the kind of every reported row"""
    out = {}
    for c, rm, it, rt in case.changers:
        rows, kinds, _ = rc.expected_for(oracle, case.train, c, rm, it, rt, case.k, sim, with_kinds=True)
        out[c] = dict(zip(rows[0].tolist(), kinds))
    return out


def stale(oracle, case, sim, rep=None):
    """S: the changers and every reported fitted user"""
    return ac.stale(oracle, case, sim, reports(oracle, case, sim) if rep is None else rep)


def split(oracle, case, sim, built, rep=None):
    """(K in ascending raw id, B ∩ S in the new fit's set order) for B = built"""
    return ac.split(oracle, case, sim, built, reports(oracle, case, sim) if rep is None else rep)


def is_plain(case, sim):
    """the plain-refit cases that the inputs decide (knncf.h "Amend"): a user leaves; the stored length changes; a cosine fit with
    a user of 4 or fewer ratings in aug"""
    if set(_users(case.train)) - set(_users(case.aug)):
        return True
    return ac.is_plain(case, sim)
