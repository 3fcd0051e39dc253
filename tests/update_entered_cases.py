"""Inputs and expected answers of the tests of knncf_update_entered* (whose kNN lists a user's additional ratings change), shared
by test_update_entered_premises.py (CPU, oracle only: the inputs reach the cases) and test_gpu_update_entered.py.

A case is a bystander_cases.Case whose `q` is the changer c — a user of the train set unless said otherwise — and whose rows are
c's ADDITIONAL rows (query_helpers._aug appends them to the file, which is aug).  The base fit is bystander_cases.base_train:
60 users, 80 items, rows of 11-39."""
import numpy as np

from tests import bystander_cases as bc
from tests import update_bystander_cases as ub
from tests.bystander_cases import Case, _rows, _users, base_train, trie_sorted
from tests.entered_cases import COS, JAC, sim_kind
from tests.query_helpers import _aug, _bits

ADDS_KS = (5, 20, 59, 300)
ZERO_USER = 900   # the planted user of the zero-weight case
TIE_IDS = range(1000, 1400)


def adds_3(synth, k):
    return ub.adds_3(synth, k=k, name=f"adds-3-k{k}")


def zero_weight(synth):
    """a planted user that shares no item with c nor with c's additional items, at k = U - 1: c stands in its list with +0.0 on
    train and on aug, at the same position (no other pair moves)"""
    u, i, r = base_train(synth)
    add = ub.unrated((u, i, r), ub.CHANGER, 3)
    taken = set(_rows((u, i, r), ub.CHANGER)[0].tolist()) | set(add.tolist())
    free = np.asarray([int(x) for x in np.unique(i) if int(x) not in taken][:6], dtype=np.int32)
    assert len(free) == 6
    train = (np.concatenate([u, np.full(6, ZERO_USER, dtype=np.int32)]).astype(np.int32), np.concatenate([i, free]).astype(np.int32),
             np.concatenate([r, [4.0, 2.5, 3.0, 5.0, 1.5, 3.5]]))
    users = _users(train)
    return Case("zero-weight", train, ub.CHANGER, add, np.full(3, 5.0), len(users) - 1, [v for v in users if v != ub.CHANGER],
                {"planted": ZERO_USER})


def tie(synth, oracle):
    """c is a fitted user whose train rows are the first rows of fitted user x and whose additional rows are x's last three: on
    aug c is a row-for-row copy of x in the same file order, so the means agree bitwise.  As in bystander_cases.tie the norm's
    fold order depends on the raw id, so the builder searches ids until it has one c BEFORE x in set order and one AFTER, each
    with a bystander v in whose full list on aug c and x tie bitwise and stand next to each other: k puts the cut between them."""
    base = base_train(synth)
    users = _users(base)
    x = users[10]
    it, rt = _rows(base, x)
    n = len(it) - 3
    assert n > 4
    found = {}
    for c in TIE_IDS:
        side = "before" if trie_sorted(oracle, [c, x])[0] == c else "after"
        if side in found:
            continue
        train = (np.concatenate([base[0], np.full(n, c, dtype=np.int32)]).astype(np.int32),
                 np.concatenate([base[1], it[:n]]).astype(np.int32), np.concatenate([base[2], rt[:n]]))
        m = oracle.Model(*_aug(train, c, it[n:], rt[n:]))
        for v in users:
            if v == x or _bits([m.fresh_similarity(oracle.SIM_COSINE, v, c)]) != _bits([m.fresh_similarity(oracle.SIM_COSINE, v, x)]):
                continue
            ids = m.pipeline(oracle.SIM_COSINE, len(users) + 1).neighbors(v)[0].tolist()
            a, b = sorted((ids.index(c), ids.index(x)))
            if b == a + 1 and b >= 2:
                found[side] = Case(f"tie-{side}", train, c, it[n:].copy(), rt[n:].copy(), b, [u for u in _users(train) if u != c],
                                   {"copy_of": x, "bystander": v, "side": side})
                break
        if len(found) == 2:
            break
    assert len(found) == 2, found.keys()
    return [found["before"], found["after"]]


def scaled(synth, n_users):
    """a synthetic fit of n_users users over 90 items, every user with more than 4 ratings"""
    t = synth.syn_scaled(n_users, 90, 24 * n_users, 11).train
    train = (t.users.copy(), t.items.copy(), t.ratings.copy())
    assert len(np.unique(train[0])) == n_users and np.unique(train[0], return_counts=True)[1].min() > 4
    return train


def dense_order(oracle, train):
    """the raw ids of the fit in set order: dense index -> raw id"""
    return oracle.Model(*train).user_iteration_order().tolist()


def added_rows(train, c, n=3, rating=5.0, skip=0):
    """n additional rows of c on train items it has not rated"""
    return ub.unrated(train, c, n, skip=skip), np.full(n, rating)


# ---- fixed-size edges: 64 cells of a list per wave step, 64 users per bitmap word ----------------------------------------------
EDGE_USERS = 140
EDGE_KS = (63, 64, 65, 128, 129)
EDGE_FITS = (64, 65, 128, 129)


def edge_positions(k):
    """the positions of a full list of k cells at which the changer must be stored: first, last, and both sides of the 64-cell
    step where the list reaches them"""
    return {0, k - 1} | {p for p in (63, 64) if p < k}


def edge_changer(oracle, train, k):
    """the first user of the fit, in set order, that stands at every position of edge_positions(k) in some list on train"""
    m = oracle.Model(*train)
    order = m.user_iteration_order().tolist()
    lists = {v: m.pipeline(oracle.SIM_COSINE, k).neighbors(v)[0].tolist() for v in order}
    want = edge_positions(k)
    for c in order:
        if want <= {ids.index(c) for v, ids in lists.items() if v != c and c in ids}:
            return c
    raise AssertionError(("no user stands at every edge position", k))


def edge_indices(n_users):
    """the dense indices around the 64-user word of the report bitmap that a fit of n_users has, and its last"""
    return sorted({x for x in (63, 64, n_users - 1) if x < n_users})


# ---- the oracle's answer ---------------------------------------------------------------------------------------------------------
def lists_of(oracle, train, c, items, ratings, k, sim):
    """per fitted v != c in set order: (v, L0, L1) with L = (ids list, sims array) of a fresh pipeline on train and on aug, and the
    model on aug"""
    kind = sim_kind(oracle, sim)
    m0 = oracle.Model(*train)
    m1 = oracle.Model(*_aug(train, c, items, ratings)) if len(items) else m0
    out = []
    for v in m0.user_iteration_order().tolist():
        if v == c:
            continue
        a, b = m0.pipeline(kind, k).neighbors(v), m1.pipeline(kind, k).neighbors(v)
        out.append((v, (a[0].tolist(), a[1]), (b[0].tolist(), b[1])))
    return out, m1


def classify(c, L0, L1):
    """the report rule of one fitted user: None (not reported), or (kind, pos, prev) with kind one of "entered", "left", "moved",
    "same" (same position; its similarity bits may have changed)"""
    p0 = L0[0].index(c) if c in L0[0] else -1
    p1 = L1[0].index(c) if c in L1[0] else -1
    if p0 < 0 and p1 < 0:
        return None
    if p0 >= 0 and p0 == p1 and L1[1][p1] == 0.0 and _bits([L0[1][p0]]) == _bits([L1[1][p1]]):
        return None  # exception (b): a zero weight that stays
    kind = "entered" if p0 < 0 else "left" if p1 < 0 else "same" if p0 == p1 else "moved"
    return kind, p1, p0


def expected_for(oracle, train, c, items, ratings, k, sim, with_kinds=False):
    """(users, sims, positions, previous, other) of the oracle under the report rule of knncf.h "Entered queries of update
    queries"; with_kinds: also the kind of every reported row and the unreported (v, L0, L1)"""
    kind_of = sim_kind(oracle, sim)
    fitted = c in set(np.asarray(train[0]).tolist())
    users, sims, pos, prev, other, kinds, quiet = [], [], [], [], [], [], []
    if fitted and len(items) == 0:  # exception (a): aug is train
        rows = []
    else:
        rows, m1 = lists_of(oracle, train, c, items, ratings, k, sim)
    for v, L0, L1 in rows:
        got = classify(c, L0, L1)
        if got is None:
            quiet.append((v, L0, L1))
            continue
        kind, p1, p0 = got
        users.append(v); pos.append(p1); prev.append(p0); kinds.append(kind)
        sims.append(float(L1[1][p1]) if p1 >= 0 else m1.fresh_similarity(kind_of, v, c))
        if kind == "entered":
            gone = [x for x in L0[0] if x not in L1[0]]
            assert len(gone) <= 1, (v, gone)
            other.append(gone[0] if gone else -1)
        elif kind == "left":
            assert [x for x in L1[0] if x not in L0[0]] == [L1[0][-1]], v
            other.append(L1[0][-1])
        else:
            other.append(-1)
    out = (np.asarray(users, dtype=np.int32), np.asarray(sims, dtype=np.float64), np.asarray(pos, dtype=np.int32),
           np.asarray(prev, dtype=np.int32), np.asarray(other, dtype=np.int32))
    return (out, kinds, quiet) if with_kinds else out


def expected(oracle, case, sim, with_kinds=False):
    return expected_for(oracle, case.train, case.q, case.items, case.ratings, case.k, sim, with_kinds)


def is_tail(k, row_prev, row_pos, L0, L1, c):
    """a tail row as the device path meets it: v's list on train is full, c stands in it, and on aug c sorts behind every OTHER
    entry of the train list — it either keeps the last cell (stays) or leaves"""
    if len(L0[0]) < k or row_prev < 0:
        return False
    rest = [x for x in L0[0] if x != c]
    if row_pos >= 0:
        return row_pos == k - 1 and L1[0][:k - 1] == rest
    return L1[0][:k - 1] == rest


def same_answer(got, want, what):
    assert got[0].tolist() == want[0].tolist(), what
    assert _bits(got[1]) == _bits(want[1]), what
    for x in (2, 3, 4):
        assert got[x].tolist() == want[x].tolist(), (what, x)
