"""Inputs and expected answers of the tests of knncf_remove_users (users leave the fit, the kNN lists that do not hold them kept),
shared by test_remove_users_premises.py (CPU, oracle only: the inputs reach the cases and the S-rule holds) and
test_gpu_remove_users.py.

A case is an amend_cases.Amend without rows whose removals are EVERY train row of the leavers, in file order: its aug is train
without those users' rows, its `call` is what knncf_amend needs to do the same (the plain refit the new call replaces), and
note["leavers"] is what knncf_remove_users gets.  The fits are those of the amend and append tests: bystander_cases.base_train
(60 users), update_entered_cases.scaled(n), revise_bystander_cases.lone_train."""
import sys

import numpy as np

from tests import amend_cases as am
from tests import append_cases as ac
from tests import revise_bystander_cases as rb
from tests import update_entered_cases as uc
from tests.amend_cases import COS, JAC, sim_kind  # noqa: F401  (re-exported)
from tests.bystander_cases import _rows, _users, base_train  # noqa: F401  (re-exported)
from tests.revise_bystander_cases import LONE_ITEM  # noqa: F401  (re-exported)

MAX_LEAVERS = 128    # KNNCF_APPEND_MAX_CHANGERS
SHORT_USER = 900     # the planted user of 4 ratings
LONE_RATER = rb.CHANGER
CELL_LEAVER = 22     # stands in the first cell of one list and in the last cell of another at k = 5 and at k = 20, both similarities
EDGE_NS = (63, 64, 65, 129)
LONG_N, LONG_K = 140, 100


def leaving(name, train, leavers, k, **note):
    """the Amend whose removals are every train row of `leavers` (given in any order, kept in note["leavers"] as given)"""
    leavers = [int(c) for c in leavers]
    at = np.isin(train[0], np.asarray(leavers, dtype=np.int64))
    return am._amend(name, train, (train[0][at], train[1][at]), ([], [], []), k, leavers=leavers, **note)


def one(synth, who, k):
    return leaving(f"one-{who}-k{k}", base_train(synth), [who], k)


def two(synth, k, who=(41, 23)):
    """two leavers in one call, given in descending order"""
    return leaving(f"two-k{k}", base_train(synth), who, k)


def edge_leavers(oracle, train):
    """the users at dense 0, 63, 64 (where the fit has them) and last"""
    order = uc.dense_order(oracle, train)
    return [order[x] for x in sorted({0} | set(uc.edge_indices(len(order))))]


def edge(synth, oracle, n_users, k=5):
    """uc.scaled(n_users) with the leavers at dense 0, the 64-user word's edges and last; at 65 and 129 users dense 63 and 64 are a
    pair of leavers adjacent in dense order"""
    train = uc.scaled(synth, n_users)
    return leaving(f"edge-{n_users}", train, edge_leavers(oracle, train), k)


def adjacent(synth, oracle, n_users=64, k=5):
    """two leavers adjacent in dense order inside one 64-user word, and the user at dense 0 stays"""
    train = uc.scaled(synth, n_users)
    order = uc.dense_order(oracle, train)
    return leaving(f"adjacent-{n_users}", train, [order[31], order[30]], k, dense=[30, 31])


def long_lists(synth, oracle, k=LONG_K):
    """uc.scaled(140) at k = 100: the lists take two 64-cell steps of a wave.  The leaver is the first user, in set order, that some
    other user holds ONLY at a cell >= 64 (one leaver: every cell of it is the only one) while some list does not hold it"""
    train = uc.scaled(synth, LONG_N)
    m = oracle.Model(*train)
    order = m.user_iteration_order().tolist()
    lists = {v: m.pipeline(oracle.SIM_COSINE, k).neighbors(v)[0].tolist() for v in order}
    for c in order:
        at = [ids.index(c) for v, ids in lists.items() if v != c and c in ids]
        if any(p >= 64 for p in at) and any(p < 64 for p in at) and len(at) < len(order) - 1:
            return leaving(f"long-{c}", train, [c], k)
    raise AssertionError("no user is held at a cell >= 64")


def lone_rater(synth, k=5):
    """revise_bystander_cases.lone_train: the leaver is the only rater of LONE_ITEM, so the item leaves aug with it"""
    return leaving("lone-rater", rb.lone_train(synth), [LONE_RATER], k)


def short_row_fit(synth, k=5, who=23):
    """base_train with a planted user of 4 ratings, who stays: KNNCF_SIM_COSINE refits plainly, Jaccard carries"""
    u, i, r = base_train(synth)
    items = np.unique(i)[[3, 17, 40, 66]].astype(np.int32)
    train = (np.concatenate([u, np.full(4, SHORT_USER, dtype=np.int32)]).astype(np.int32), np.concatenate([i, items]).astype(np.int32),
             np.concatenate([r, [4.0, 2.5, 1.0, 5.0]]))
    return leaving("short-row-fit", train, [who], k)


def crowd(synth, n_leavers=MAX_LEAVERS + 1, k=5):
    """n_leavers of the 140 users of uc.scaled(140) leave"""
    train = uc.scaled(synth, uc.EDGE_USERS)
    return leaving(f"crowd-{n_leavers}", train, _users(train)[:n_leavers], k)


def five_users():
    """five users over 7 items, every user with more than 4 rows"""
    users = [40, 12, 77, 3, 58]
    rows = [(u, 10 * i + 1, float(1 + (3 * x + 2 * i) % 9) / 2) for i in range(7) for x, u in enumerate(users) if (x + i) % 5]
    return tuple(np.asarray(a, dtype=t) for a, t in zip(zip(*rows), (np.int32, np.int32, np.float64)))


def to_four_users(k=2, who=77):
    return leaving("shrinks-to-4", five_users(), [who], k)


def random_leavers(rng, train, lo=1, hi=6):
    users = _users(train)
    return [int(c) for c in rng.choice(users, size=int(rng.integers(lo, hi + 1)), replace=False)]


# ---- the call --------------------------------------------------------------------------------------------------------------------
def remove_users(e, users, return_dropped=False):
    """knncf_remove_users on Engine e through the binding's module-level remove_users"""
    kn = sys.modules[type(e).__module__]
    return kn.remove_users(e, users, return_dropped=return_dropped)


# ---- the oracle's side -----------------------------------------------------------------------------------------------------------
def train_lists(oracle, case, sim, users=None):
    """{v: (ids, similarity bits)}: the fresh lists on train, which are the stored ones wherever the call carries"""
    return ac.fresh_lists(oracle, case.train, _users(case.train) if users is None else users, case.k, sim)


def holders(oracle, case, sim, lists=None):
    """{v: the cells of v's list on train that hold a leaver}, for every fitted v that is no leaver and holds one"""
    gone = set(case.note["leavers"])
    lists = train_lists(oracle, case, sim) if lists is None else lists
    out = {}
    for v, (ids, _) in lists.items():
        at = [p for p, x in enumerate(ids) if x in gone]
        if at and v not in gone:
            out[v] = at
    return out


def stale(oracle, case, sim, lists=None):
    """S: the leavers and the holders"""
    return set(case.note["leavers"]) | set(holders(oracle, case, sim, lists))


def is_plain(case, sim, max_leavers=MAX_LEAVERS):
    """the plain refits of knncf.h "Remove users" that the inputs decide"""
    old, new = _users(case.train), _users(case.aug)
    if min(case.k, len(new) - 1) != min(case.k, len(old) - 1) or len(case.note["leavers"]) > max_leavers:
        return True
    if min(len(old), len(new), len(np.unique(case.train[1])), len(np.unique(case.aug[1]))) < 5:
        return True
    return sim == COS and np.unique(case.train[0], return_counts=True)[1].min() <= 4


def dropped_order(oracle, case, ids):
    """ids in the new fit's set order, a leaver where its id would stand: the old fit's set order — but where the new fit has fewer
    than 5 users, which iterate in the order of their first row, the leavers stand behind them"""
    new = oracle.Model(*case.aug).user_iteration_order().tolist()
    old = oracle.Model(*case.train).user_iteration_order().tolist() if len(_users(case.train)) >= 5 else _users(case.train)
    if len(new) >= 5:
        return [v for v in old if v in set(ids)]
    return [v for v in new if v in set(ids)] + [v for v in old if v in set(ids) and v not in set(new)]


def split(oracle, case, sim, built, plain=None, lists=None):
    """(K in ascending raw id, B ∩ S in the new fit's set order) for B = built; a plain refit keeps nothing"""
    b = set(int(x) for x in built)
    plain = is_plain(case, sim) if plain is None else plain
    s = b if plain else stale(oracle, case, sim, lists)
    return sorted(b - s), dropped_order(oracle, case, b & s)
