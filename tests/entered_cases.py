"""Inputs of the entered-query tests (knncf_query_entered*: which fitted users' neighbour lists a newcomer joins), shared by
test_entered_premises.py (CPU, oracle only: the inputs reach the cases) and test_gpu_entered.py.

A case is a bystander_cases.Case (the train set, the newcomer q with its rows, the handle's k) with the similarities it is
asked under in note["sims"] and, where the builder knows it, the number of entered users per similarity in note["count"].
Most build on bystander_cases.base_train: 60 users, 80 items, rows of 11-39."""
import numpy as np

from tests import bystander_cases as bc
from tests.query_helpers import _aug, _bits

COS, JAC = "cosine", "jaccard"
TINY_Q = 3000
TINY_SEEDS = (15, 17, 19, 21)  # the first whose ratings the reference can scale (scale() != 0) is taken


def _with(case, name, sims, count):
    case.name = name
    case.note = dict(case.note, sims=tuple(sims), count=dict(count))
    return case


def sim_kind(mod, sim):
    """the SIM_COSINE / SIM_JACCARD constant of the oracle or of the binding"""
    return mod.SIM_COSINE if sim == COS else mod.SIM_JACCARD


def near_clones(synth):
    return [_with(bc.near_clone(synth, k=5), "near-clone", (COS, JAC), {COS: 11, JAC: 7}),
            _with(bc.near_clone(synth, k=1), "near-clone-k1", (COS,), {COS: 2})]


def ties(synth, oracle):
    """the set-order tie at the cut: q ties bitwise with the user it copies in the bystander's list; before it in set order q
    is entered at the last position and displaces the copied user, after it q stays out"""
    return [_with(c, c.name, (COS,), {}) for c in bc.tie(synth, oracle)]


def short_lists(synth):
    """k = U - 1: full lists, everybody entered; k >= U: the lists grow, nobody displaced"""
    return [_with(c, c.name, (COS, JAC), {COS: 60, JAC: 60}) for c in bc.short_lists(synth)]


def anti_clones(synth):
    """near_clone with every rating r replaced by round(6 - r, 2): the empty answer at k = 5, a selective one at k = U - 1"""
    out = []
    for k, name, sims, count in ((5, "anti-clone", (COS, JAC), {COS: 0, JAC: 7}), (59, "anti-clone-59", (COS,), {COS: 43})):
        c = bc.near_clone(synth, k=k)
        c.ratings = np.round(6.0 - c.ratings, 2)
        out.append(_with(c, name, sims, count))
    return out


def _tiny_newcomer(synth, oracle, seed):
    train = bc.base_train(synth)
    users = bc._users(train)
    rng = np.random.default_rng(seed)
    n = 3 + seed % 2
    row = bc._rows(train, users[seed % 60])[0]
    items = rng.choice(row, n, replace=False)
    items = np.asarray(bc.trie_sorted(oracle, items)[::-1], dtype=np.int32)
    ratings = np.round(rng.uniform(1.0, 5.0, n), 2)
    return bc.Case("tiny-newcomer", train, TINY_Q, items, ratings, 5, users, {"seed": seed})


def tiny_newcomer(synth, oracle):
    """a newcomer of 3 or 4 rows in REVERSE trie order: the fold-in kernels fold its pairs in the given order (Set1..Set4), the
    fitted user that owns the pair folds in trie order.  A seed whose ratings the reference cannot scale is replaced by the next."""
    for seed in TINY_SEEDS:
        c = _tiny_newcomer(synth, oracle, seed)
        try:
            oracle.Model(*c.aug).pipeline(oracle.SIM_COSINE, c.k).neighbors(c.others[0])
        except oracle.OracleError:
            continue
        return _with(c, c.name, (COS, JAC), {})
    raise AssertionError("no seed of TINY_SEEDS gives a newcomer the reference can scale")


def new_item(synth):
    return _with(bc.new_item(synth), "new-item", (COS, JAC), {COS: 10})


def off_scale(synth):
    """ratings off the star scale and a fitted user with a negative mean; at k = U - 1 that user is entered like any other"""
    out = []
    for k, name, count in ((5, "off-scale", 8), (59, "off-scale-59", 60)):
        c = bc.off_scale(synth)
        c.k = k
        c.others = [v for v in c.others if v != bc.UNKNOWN_USER]
        out.append(_with(c, name, (COS,), {COS: count}))
    return out


def tiny_rows(synth, oracle):
    """trains with users of 1, 3 and 4 ratings: accepted under Jaccard, refused under the adjusted cosine"""
    want = {"tiny-1": 2, "tiny-4": 3, "tiny-5": 2}
    return [_with(c, c.name, (JAC,), {JAC: want[c.name]}) for c in bc.tiny_rows(synth, oracle)]


def all_cases(synth, oracle):
    return (near_clones(synth) + ties(synth, oracle) + short_lists(synth) + anti_clones(synth) + [tiny_newcomer(synth, oracle)]
            + [new_item(synth)] + off_scale(synth) + tiny_rows(synth, oracle))


NAMES = ["near-clone", "near-clone-k1", "tie-before", "tie-after", "short-59", "short-300", "anti-clone", "anti-clone-59",
         "tiny-newcomer", "new-item", "off-scale", "off-scale-59", "tiny-1", "tiny-4", "tiny-5"]


def expected_for(oracle, train, q, items, ratings, k, sim):
    """(users, sims, positions, displaced) of the oracle: per fitted user v in the fit's set order, getNeighbors(aug, k, sim)(v)
    on a fresh pipeline; where q is in it, its similarity and position there, and the id of getNeighbors(train, k, sim)(v) that
    is gone (-1: none)"""
    kind = sim_kind(oracle, sim)
    m0 = oracle.Model(*train)
    m1 = oracle.Model(*_aug(train, q, items, ratings))
    users, sims, pos, disp = [], [], [], []
    for v in m0.user_iteration_order().tolist():
        ids, ss = m1.pipeline(kind, k).neighbors(v)
        ids = ids.tolist()
        if q not in ids:
            continue
        gone = [x for x in m0.pipeline(kind, k).neighbors(v)[0].tolist() if x not in ids]
        assert len(gone) <= 1, (v, gone)
        users.append(v); sims.append(float(ss[ids.index(q)])); pos.append(ids.index(q)); disp.append(gone[0] if gone else -1)
    return (np.asarray(users, dtype=np.int32), np.asarray(sims, dtype=np.float64), np.asarray(pos, dtype=np.int32),
            np.asarray(disp, dtype=np.int32))


def expected(oracle, case, sim):
    return expected_for(oracle, case.train, case.q, case.items, case.ratings, case.k, sim)


def same_answer(got, want, what):
    assert got[0].tolist() == want[0].tolist(), what
    assert _bits(got[1]) == _bits(want[1]), what
    assert got[2].tolist() == want[2].tolist(), what
    assert got[3].tolist() == want[3].tolist(), what
