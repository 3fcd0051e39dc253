"""Inputs and expected answers of the tests of knncf_revise_entered* (whose kNN lists a user's removals change), shared by
test_revise_entered_premises.py (CPU, oracle only: the inputs reach the cases) and test_gpu_revise_entered.py.

A case is a revise_bystander_cases.RCase: `q` is the changer c, `removed` the train items it takes out, (`items`, `ratings`) its
ADDITIONAL rows; aug = revise_cases.aug_of.  The base fit is bystander_cases.base_train (60 users, 80 items, 1 200 ratings; the
changer is user 5 with 17 train rows); update_entered_cases.scaled gives the fits of the fixed-size edges."""
import numpy as np

from tests import revise_bystander_cases as rb
from tests import update_entered_cases as uc
from tests.bystander_cases import _rows, _users, base_train
from tests.entered_cases import COS, JAC, sim_kind
from tests.query_helpers import _bits
from tests.revise_cases import aug_of
from tests.update_bystander_cases import CHANGER
from tests.update_entered_cases import classify, is_tail, same_answer  # noqa: F401  (the tests take them from here)

KS = (5, 20, 59, 300)
KEPT = 4  # keeps-4: the train rows the changer is left with
# keeps-4 at k = 5: neither of user 5's two pairs whose bits depend on the owner is a reported row there, so the case has a
# changer of its own — the first user, in ascending raw id, keeping 4 and then 3 rows, with such a row reported at k = 5
# (test_revise_entered_premises.py repeats the search)
KEEPS_4_K5_CHANGER = 24


def removes_3(synth, k):
    """the first, the middle and the last train row of user 5 removed, nothing added"""
    return rb.removes_3(synth, k=k, name=f"removes-3-k{k}")


def keeps_4(synth, k, changer=CHANGER, kept=KEPT):
    """all but the first four train rows of user 5 removed, nothing added: c falls to <= 4 rows on aug, where its own closure
    folds a pair in c's given order and a bystander's folds it in dense-item order"""
    train = base_train(synth)
    mine = _rows(train, changer)[0]
    assert len(mine) > 2 * kept
    return rb._case(f"keeps-{kept}-of-{changer}-k{k}", train, changer, mine[kept:], [], [], k)


def re_rates(synth, k):
    """two train items of user 5 removed and given again with another value: their rows move behind every train row"""
    train = base_train(synth)
    mine, vals = _rows(train, CHANGER)
    pick = [1, len(mine) - 2]
    return rb._case(f"re-rates-k{k}", train, CHANGER, mine[pick], mine[pick], [rb._other_value(vals[p], True) for p in pick], k)


def same_value(synth, k):
    """two train items removed and given again with the SAME value: an ordinary query"""
    train = base_train(synth)
    mine, vals = _rows(train, CHANGER)
    pick = [1, len(mine) - 2]
    return rb._case(f"same-value-k{k}", train, CHANGER, mine[pick], mine[pick], vals[pick], k)


def tiny_changer(synth, oracle):
    """on the train set of bystander_cases.tiny_rows (Jaccard accepts it): the fitted user of 4 ratings removes its second row"""
    from tests import bystander_cases as bc
    base = bc.tiny_rows(synth, oracle)[1]
    u4 = next(u for u, n in base.note["tiny"].items() if n == 4)
    return rb._case("tiny-changer", base.train, u4, _rows(base.train, u4)[0][[1]], [], [], base.k)


def lone_item(synth, k):
    """revise_bystander_cases.lone_item: c's removed item leaves aug (removed), has c as its only rater behind every train row
    (rerated), or another row of c goes instead (kept)"""
    return rb.lone_item(synth, k=k)


def zero_weight(synth):
    """the planted user of update_entered_cases.zero_weight shares no item with c: a removal of c keeps c in its list of U - 1
    at the same place with +0.0 of the same bits"""
    base = uc.zero_weight(synth)
    mine = _rows(base.train, base.q)[0]
    return rb._case("zero-weight-removal", base.train, base.q, mine[[2]], [], [], base.k, planted=base.note["planted"])


def removed_rows(train, c, n, skip=0):
    """n train items of c, every other one from position `skip` on in file order (c keeps more than 4 rows)"""
    mine = _rows(train, c)[0]
    pick = mine[skip::2][:n]
    assert len(pick) == n and len(mine) - n > 4, (c, len(mine), n)
    return pick.astype(np.int32)


def edge_removals(train, c):
    """how many rows the changer of a fixed-size edge case removes: half of them, and three"""
    return (len(_rows(train, c)[0]) // 2, 3)


# ---- the oracle's answer ---------------------------------------------------------------------------------------------------------
def lists_of(oracle, train, c, removed, items, ratings, k, sim):
    """update_entered_cases.lists_of with aug = revise_cases.aug_of"""
    kind = sim_kind(oracle, sim)
    m0 = oracle.Model(*train)
    m1 = oracle.Model(*aug_of(train, c, removed, items, ratings)) if len(items) or len(removed) else m0
    out = []
    for v in m0.user_iteration_order().tolist():
        if v == c:
            continue
        a, b = m0.pipeline(kind, k).neighbors(v), m1.pipeline(kind, k).neighbors(v)
        out.append((v, (a[0].tolist(), a[1]), (b[0].tolist(), b[1])))
    return out, m1


def expected_for(oracle, train, c, removed, items, ratings, k, sim, with_kinds=False):
    """(users, sims, positions, previous, other) of the oracle under the report rule of knncf.h "Entered queries of revise
    queries": update_entered_cases.expected_for on aug_of, exception (a) being a fitted c without removals AND without rows"""
    kind_of = sim_kind(oracle, sim)
    fitted = c in set(np.asarray(train[0]).tolist())
    users, sims, pos, prev, other, kinds, quiet = [], [], [], [], [], [], []
    if fitted and len(items) == 0 and len(removed) == 0:  # exception (a): aug is train
        rows = []
    else:
        rows, m1 = lists_of(oracle, train, c, removed, items, ratings, k, sim)
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
    return expected_for(oracle, case.train, case.q, case.removed, case.items, case.ratings, case.k, sim, with_kinds)


def tail_rows(oracle, case, sim):
    """the reported rows that the stored list cannot decide (update_entered_cases.is_tail): their positions on aug, -1 = left"""
    out = expected(oracle, case, sim)
    rows, _ = lists_of(oracle, case.train, case.q, case.removed, case.items, case.ratings, case.k, sim)
    lists = {v: (a, b) for v, a, b in rows}
    return [int(p) for v, p, pr in zip(out[0], out[2], out[3]) if is_tail(case.k, int(pr), int(p), *lists[int(v)], case.q)]


def pair_order_rows(oracle, case):
    """the REPORTED rows (v, S(v, c) as v folds it) of a cosine case whose similarity bits differ from S(c, v) as c's own closure
    folds it on aug: what the pair stage of the device path has to compute anew for a changer of <= 4 rows on aug"""
    out = expected(oracle, case, COS)
    m1 = oracle.Model(*case.aug)
    return [(int(v), float(s)) for v, s in zip(out[0], out[1]) if _bits([m1.fresh_similarity(oracle.SIM_COSINE, case.q, int(v))]) != _bits([s])]
