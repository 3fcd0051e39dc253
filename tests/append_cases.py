"""Inputs and expected answers of the tests of knncf_append (new ratings into the fit, the unchanged kNN lists kept), shared by
test_append_premises.py (CPU, oracle only: the inputs reach the cases and the S-rule holds) and test_gpu_append.py.

A case is an Append: the train set, the appended rows in file order (rows of several users may interleave), and the handle's k.
aug = train ++ rows.  The base fit is bystander_cases.base_train: 60 users, 80 items, rows of 11-39."""
from dataclasses import dataclass, field

import numpy as np

from tests import bystander_cases as bc
from tests import update_bystander_cases as ub
from tests import update_entered_cases as uc
from tests.bystander_cases import NEW_ITEM, _rows, _users, base_train
from tests.entered_cases import COS, JAC, sim_kind  # noqa: F401  (re-exported)
from tests.query_helpers import _bits

NEWCOMER = 1000
SECOND = 23  # the second fitted changer of the joint case


@dataclass
class Append:
    name: str
    train: tuple          # (users, items, ratings), file order
    users: np.ndarray     # the appended rows, file order
    items: np.ndarray
    ratings: np.ndarray
    k: int
    note: dict = field(default_factory=dict)

    @property
    def rows(self):
        return self.users, self.items, self.ratings

    @property
    def aug(self):
        return (np.concatenate([self.train[0], self.users]).astype(np.int32), np.concatenate([self.train[1], self.items]).astype(np.int32),
                np.concatenate([self.train[2], self.ratings]).astype(np.float64))

    @property
    def changers(self):
        """the distinct users of the rows in the order of their first row, each with its rows in file order"""
        out = []
        for c in dict.fromkeys(self.users.tolist()):
            at = self.users == c
            out.append((int(c), self.items[at].copy(), self.ratings[at].copy()))
        return out


def _append(name, train, rows, k, **note):
    u, i, r = rows
    return Append(name, train, np.asarray(u, dtype=np.int32), np.asarray(i, dtype=np.int32), np.asarray(r, dtype=np.float64), k, note)


def of_case(case):
    """a bystander_cases.Case (one changer q with its rows) as an Append"""
    return _append(case.name, case.train, (np.full(len(case.items), case.q), case.items, case.ratings), case.k, **case.note)


def adds_3(synth, k):
    return of_case(uc.adds_3(synth, k))


def zero_weight(synth):
    return of_case(uc.zero_weight(synth))


def interleave(parts):
    """rows of several (user, items, ratings) dealt round-robin: the users' rows interleave, each user's order is kept"""
    u, i, r = [], [], []
    for j in range(max(len(p[1]) for p in parts)):
        for c, it, rt in parts:
            if j < len(it):
                u.append(c); i.append(int(it[j])); r.append(float(rt[j]))
    return u, i, r


def joint(synth, k=5, train=None, newcomer=NEWCOMER):
    """two fitted changers and one newcomer, rows interleaved.  The newcomer is bystander_cases.near_clone's (a fitted user's
    rows with one rating changed) and also rates an item unknown to train; changer 5 adds three ratings of 5.0, changer 23 two
    of 1.0 and the same new item"""
    train = base_train(synth) if train is None else train
    nc = bc.near_clone(synth, k=k, q=newcomer, train=train)
    a = (ub.CHANGER, ub.unrated(train, ub.CHANGER, 3), np.full(3, 5.0))
    b = (SECOND, np.concatenate([ub.unrated(train, SECOND, 2, skip=3), [NEW_ITEM]]).astype(np.int32), np.asarray([1.0, 1.0, 3.5]))
    q = (newcomer, np.concatenate([nc.items[:4], [NEW_ITEM], nc.items[4:]]).astype(np.int32), np.concatenate([nc.ratings[:4], [4.5], nc.ratings[4:]]))
    return _append(f"joint-k{k}", train, interleave([a, q, b]), k, newcomer=newcomer, fitted=[ub.CHANGER, SECOND])


def with_newcomer(synth, train, k, newcomer=NEWCOMER, n=None):
    """one newcomer whose rows are a fitted user's with one rating changed (n: only the first n of them)"""
    nc = bc.near_clone(synth, k=k, q=newcomer, train=train)
    it, rt = (nc.items, nc.ratings) if n is None else (nc.items[:n], nc.ratings[:n])
    return _append(f"newcomer-{len(it)}", train, (np.full(len(it), newcomer), it, rt), k, newcomer=newcomer)


def edge_fit(synth, oracle, n_users, k):
    """uc.scaled(n_users) with the changers at dense 63, 64 (where the fit has it) and last, one added row each, plus one
    newcomer: the mask words of 64 users at their edges, and a dense index that shifts across one"""
    train = uc.scaled(synth, n_users)
    order = uc.dense_order(oracle, train)
    parts = [(order[at], *uc.added_rows(train, order[at], n=1)) for at in uc.edge_indices(n_users)]
    nc = bc.near_clone(synth, k=k, q=NEWCOMER, train=train)
    parts.append((NEWCOMER, nc.items, nc.ratings))
    return _append(f"edge-{n_users}", train, interleave(parts), k, newcomer=NEWCOMER, at=[order[x] for x in uc.edge_indices(n_users)])


# ---- the oracle's side -----------------------------------------------------------------------------------------------------------
def reports(oracle, case, sim):
    """{changer: the fitted users knncf_update_entered_batch reports for (changer, its rows of the append in order) on train}, each
    changer on its own, with the kind of every reported row"""
    out = {}
    for c, it, rt in case.changers:
        rows, kinds, _ = uc.expected_for(oracle, case.train, c, it, rt, case.k, sim, with_kinds=True)
        out[c] = dict(zip(rows[0].tolist(), kinds))
    return out


def stale(oracle, case, sim, rep=None):
    """S: the changers and every reported fitted user"""
    rep = reports(oracle, case, sim) if rep is None else rep
    s = set(rep)
    for users in rep.values():
        s |= set(users)
    return s


def split(oracle, case, sim, built, rep=None):
    """(K in ascending raw id, B ∩ S in the new fit's set order) for B = built"""
    s = stale(oracle, case, sim, rep)
    order = oracle.Model(*case.aug).user_iteration_order().tolist()
    b = set(int(x) for x in built)
    return sorted(b - s), [v for v in order if v in b and v in s]


def fresh_lists(oracle, data, users, k, sim):
    """{v: (ids, similarity bits)} of a fresh pipeline per user on `data`"""
    m = oracle.Model(*data)
    kind = sim_kind(oracle, sim)
    out = {}
    for v in users:
        ids, sims = m.pipeline(kind, k).neighbors(int(v))
        out[int(v)] = (ids.tolist(), _bits(sims))
    return out


def is_plain(case, sim):
    """the plain-refit cases that the inputs decide (knncf.h "Append"): the stored length changes; a cosine fit with a user of 4
    or fewer ratings in aug"""
    n_old, n_new = len(_users(case.train)), len(_users(case.aug))
    if min(case.k, n_new - 1) != min(case.k, n_old - 1):
        return True
    return sim == COS and np.unique(case.aug[0], return_counts=True)[1].min() <= 4
