"""Inputs of the tests of knncf_update_bystander_* (a fitted user's kNN answers once ANOTHER user of the fit has added ratings),
shared by test_update_bystander_premises.py (CPU, oracle only: the inputs reach the cases) and test_gpu_update_bystander.py.

A case is a bystander_cases.Case whose `q` is the changer c — a user of the train set unless said otherwise — and whose rows are
c's ADDITIONAL rows: query_helpers._aug appends them to the file, which is aug.  The base fit is bystander_cases.base_train."""
import numpy as np

from tests import bystander_cases as bc
from tests.bystander_cases import NEW_ITEM, UNKNOWN_USER, Case, _rows, _users, base_train, trie_sorted
from tests.query_helpers import _aug, _bits

CHANGER = 5


def _others(train, c):
    return [u for u in _users(train) if u != c] + [UNKNOWN_USER]


def unrated(train, c, n, skip=0):
    """the first n train items, in ascending raw id after `skip` of them, that c has not rated"""
    mine = set(_rows(train, c)[0].tolist())
    free = [int(i) for i in np.unique(train[1]) if int(i) not in mine]
    return np.asarray(free[skip:skip + n], dtype=np.int32)


def adds_3(synth, k=5, name="adds-3"):
    """user 5 rates three more items, 5.0 each: its mean, every deviation and its norm move"""
    train = base_train(synth)
    return Case(name, train, CHANGER, unrated(train, CHANGER, 3), np.full(3, 5.0), k, _others(train, CHANGER))


def leaves_short(synth):
    """k >= the number of other users: no list is full, c can only move"""
    return [adds_3(synth, k=59, name="leaves-short-59"), adds_3(synth, k=300, name="leaves-short-300")]


def new_item(synth, k=5):
    """one additional row, on an item unknown to train: that item has exactly one rater in aug"""
    train = base_train(synth)
    return Case("new-item", train, CHANGER, np.asarray([NEW_ITEM], dtype=np.int32), np.asarray([5.0]), k, _others(train, CHANGER))


def negative_unknown(synth, k=5):
    """the off-scale fit of bystander_cases (one fitted user with a negative mean; UNKNOWN_USER among the bystanders); the
    changer adds three ratings"""
    base = bc.off_scale(synth)
    train = base.train
    c = Case("negative", train, CHANGER, unrated(train, CHANGER, 3), np.asarray([4.75, 0.57, 3.82]), k, _others(train, CHANGER))
    c.note["negative"] = base.note["negative"]
    assert c.note["negative"] != CHANGER
    return c


# ---- fold-place: the place, the deviation and the similarity of c's terms in a bystander's fold ------------------------------
def fold_rows(oracle, case, sim, v, item):
    """the terms of (v, item)'s fold on aug as the reference adds them: (rater, file row, deviation on aug, knn similarity of
    (v, rater)) of the item's rows in file order, on a fresh pipeline whose first evaluation is v's"""
    u, i, _ = case.aug
    m = oracle.Model(*case.aug)
    dev = m.normalized_deviations()
    p = m.pipeline(sim, case.k)
    return [(int(u[t]), int(t), float(dev[t]), p.knn_similarity(v, int(u[t]))) for t in np.flatnonzero(i == item)]


def fold_predict(oracle, avg, terms):
    """predictor :568-585 over (deviation, similarity) terms in the given order: both sums are left folds from 0.0"""
    a = d = 0.0
    for dv, s in terms:
        a = a + dv * s
        d = d + abs(s)
    w = a / d if d > 0 else 0.0
    return avg + w * oracle.scale(avg + w, avg)


SLIPS = ("train-term-last", "train-deviation", "train-similarity", "additional-first")


def slipped_terms(oracle, case, sim, v, item, slip, train_dev, train_sim):
    """the (deviation, similarity) terms of (v, item) on aug with one planted slip about the changer c = case.q; train_dev[t] =
    the deviation of file row t on train, train_sim = knn similarity of (v, c) on train"""
    rows = fold_rows(oracle, case, sim, v, item)
    n_train = len(case.train[0])
    terms = [(dv, s) for (_, _, dv, s) in rows]
    mine = [x for x, r in enumerate(rows) if r[0] == case.q]
    if not mine:
        return terms
    x = mine[0]
    is_train = rows[x][1] < n_train
    if slip == "train-term-last" and is_train:
        terms = terms[:x] + terms[x + 1:] + [terms[x]]
    elif slip == "train-deviation" and is_train:
        terms[x] = (float(train_dev[rows[x][1]]), terms[x][1])
    elif slip == "train-similarity":
        terms[x] = (terms[x][0], train_sim)
    elif slip == "additional-first" and not is_train:
        terms = [terms[x]] + terms[:x] + terms[x + 1:]
    return terms


def fold_place(synth, oracle):
    """The off-scale ratings (sums round) at k = 59, so that c is in every list.  The additional ratings are searched (seeds 0,
    1, ...) until every slip of SLIPS changes the bits of some (bystander, item) prediction; returns (case, witnesses) with
    witnesses[slip] = (bystander, item)."""
    train = bc.off_scale(synth).train
    sim = oracle.SIM_COSINE
    neg = bc.off_scale(synth).note["negative"]
    users = [u for u in _users(train) if u not in (CHANGER, neg)][:20]
    mt = oracle.Model(*train)
    train_dev = mt.normalized_deviations()
    own = _rows(train, CHANGER)[0]
    for seed in range(50):
        rng = np.random.default_rng(seed)
        items = unrated(train, CHANGER, 3, skip=seed % 7)
        case = Case("fold-place", train, CHANGER, items, np.round(rng.uniform(0.6, 4.8, 3), 2), 59, _others(train, CHANGER))
        m = oracle.Model(*case.aug)
        found = {}
        for v in users:
            avg = m.users_avg(v)
            train_sim = mt.pipeline(sim, 59).knn_similarity(v, CHANGER)
            for item in [int(x) for x in own[:8]] + [int(x) for x in items]:
                want = m.pipeline(sim, 59).predict(v, item)
                if _bits([fold_predict(oracle, avg, [(dv, s) for (_, _, dv, s) in fold_rows(oracle, case, sim, v, item)])]) != _bits([want]):
                    raise AssertionError(("the plain fold is not the oracle's", v, item))
                for slip in SLIPS:
                    if slip in found:
                        continue
                    got = fold_predict(oracle, avg, slipped_terms(oracle, case, sim, v, item, slip, train_dev, train_sim))
                    if _bits([got]) != _bits([want]):
                        found[slip] = (v, item)
            if len(found) == len(SLIPS):
                return case, found
    raise AssertionError("no seed gives a witness for every slip")


# ---- tiny: users of <= 4 ratings on either side ----------------------------------------------------------------------------
def tiny(synth, oracle):
    """On the train set of bystander_cases.tiny_rows (users trimmed to 1, 3 and 4 ratings whose file order is the reverse of
    their trie order): the 1-rating user as the changer with 2 additional rows (3 rows on aug), and a changer of more than 4
    rows that adds the tiny users' items, searched (seeds) until some S(v, c) differs bitwise from S(c, v) on aug."""
    base = bc.tiny_rows(synth, oracle)[0]
    train, tiny_users = base.train, base.note["tiny"]
    u1, u3, u4 = list(tiny_users)
    theirs = [int(i) for u in (u4, u3) for i in _rows(train, u)[0] if int(i) not in set(_rows(train, u1)[0].tolist())]
    small = Case("tiny-changer", train, u1, np.asarray(list(dict.fromkeys(theirs))[:2], dtype=np.int32), np.asarray([4.5, 1.5]), 5,
                 _others(train, u1), {"tiny": dict(tiny_users)})
    assert len(set(small.items.tolist())) == 2
    big_c = next(u for u in _users(train) if u not in tiny_users and len(_rows(train, u)[0]) > 4)
    mine = set(_rows(train, big_c)[0].tolist())
    share = [int(i) for u in (u1, u3, u4) for i in _rows(train, u)[0] if int(i) not in mine]
    share = np.asarray(list(dict.fromkeys(share))[::-1], dtype=np.int32)  # (not in ascending trie order)
    assert len(share) >= 3
    for seed in range(200):
        rng = np.random.default_rng(seed)
        big = Case("tiny-bystanders", train, big_c, share, np.round(rng.uniform(1.0, 5.0, len(share)), 2), 5, _others(train, big_c),
                   {"tiny": dict(tiny_users)})
        try:
            m = oracle.Model(*big.aug)
            differs = [v for v in (u3, u4) if _bits([m.fresh_similarity(oracle.SIM_COSINE, v, big_c)]) !=
                       _bits([m.fresh_similarity(oracle.SIM_COSINE, big_c, v)])]
        except oracle.OracleError:
            continue
        if differs:
            big.note["differs"] = differs
            return [small, big]
    raise AssertionError("no seed gives an order-dependent pair")


# ---- tie (Jaccard): S(v, c) on aug equals another candidate's similarity bitwise, the two on either side of the cut -----------
def _jaccard(a, b):
    both = len(a & b)
    return both / (len(a) + len(b) - both)


def tie(synth, oracle):
    """Jaccard similarities are ratios of counts, so additional rows can be chosen to make S(v, c) equal S(v, w) exactly.  The
    builder walks (changer, number of additional items, bystander) until it has one case in which c comes BEFORE the tied w in
    set order and one AFTER, with nobody else of that similarity: k is then the position of the second of the two."""
    train = base_train(synth)
    users = _users(train)
    order = {u: x for x, u in enumerate(trie_sorted(oracle, users))}
    sets = {u: set(_rows(train, u)[0].tolist()) for u in users}
    found = {}
    for c in users:
        for n in (1, 2, 3, 4):
            add = unrated(train, c, n)
            mine = sets[c] | set(add.tolist())
            for v in users:
                if v == c:
                    continue
                s = {x: _jaccard(sets[v], mine if x == c else sets[x]) for x in users if x != v}
                if s[c] == _jaccard(sets[v], sets[c]):
                    continue  # (the additional rows must have moved it)
                same = [x for x in s if x != c and s[x] == s[c]]
                if len(same) != 1:
                    continue
                w = same[0]
                side = "before" if order[c] < order[w] else "after"
                if side in found:
                    continue
                k = sum(1 for x in s if s[x] > s[c]) + 1  # the first of the two is in, the second is out
                if k < 2:
                    continue
                found[side] = Case(f"tie-{side}", train, c, add, np.full(n, 3.0), k, _others(train, c),
                                   {"bystander": v, "tied_with": w, "side": side})
            if len(found) == 2:
                return [found["before"], found["after"]]
    raise AssertionError(found.keys())


def all_cases(synth, oracle):
    return ([adds_3(synth)] + leaves_short(synth) + [new_item(synth), negative_unknown(synth), fold_place(synth, oracle)[0]]
            + tiny(synth, oracle) + tie(synth, oracle))


JACCARD_CASES = ["adds-3", "leaves-short-59", "leaves-short-300", "new-item", "tie-before", "tie-after", "tiny-changer", "tiny-bystanders"]


def expected(oracle, case, sim):
    return bc.expected(oracle, case, sim)


def list_changes(oracle, case, sim):
    """what the additional rows do to the lists that hold c = case.q: the bystanders whose list c leaves, enters, stays in, and of
    the last those where its position changes; lists as {bystander: (ids on train, ids on aug, sims on train, sims on aug)}"""
    mt, ma = oracle.Model(*case.train), oracle.Model(*case.aug)
    out = {"leaves": [], "enters": [], "stays": [], "moves": [], "lists": {}}
    for v in case.others:
        if v == UNKNOWN_USER:
            continue
        a, b = mt.pipeline(sim, case.k).neighbors(v), ma.pipeline(sim, case.k).neighbors(v)
        ia, ib = a[0].tolist(), b[0].tolist()
        out["lists"][v] = (ia, ib, a[1], b[1])
        if case.q in ia and case.q not in ib:
            out["leaves"].append(v)
        elif case.q not in ia and case.q in ib:
            out["enters"].append(v)
        elif case.q in ia:
            out["stays"].append(v)
            if ia.index(case.q) != ib.index(case.q):
                out["moves"].append(v)
    return out
