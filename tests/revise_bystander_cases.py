"""Inputs of the tests of knncf_revise_bystander_* (a fitted user's kNN answers once ANOTHER user of the fit has removed or
re-rated items), shared by test_revise_bystander_premises.py (CPU, oracle only: the inputs reach the cases) and
test_gpu_revise_bystander.py.

A case is an RCase: a bystander_cases.Case whose `q` is the changer c, with the train items c takes out (`removed`) beside its
ADDITIONAL rows; aug = revise_cases.aug_of.  The fits are those of bystander_cases: 60 users, and the off-scale variant with its
negative-mean user.  The changer is user 5 unless said otherwise; the bystanders are every other user and UNKNOWN_USER."""
from dataclasses import dataclass, field

import numpy as np

from tests import bystander_cases as bc
from tests.bystander_cases import NEW_ITEM, UNKNOWN_USER, Case, _rows, _users, base_train
from tests.query_helpers import UNKNOWN_ITEM, _bits
from tests.revise_cases import aug_of
from tests.update_bystander_cases import CHANGER, _others, fold_predict, unrated

LONE_ITEM = 4000


@dataclass
class RCase(Case):
    removed: np.ndarray = field(default_factory=lambda: np.empty(0, dtype=np.int32))

    @property
    def aug(self):
        return aug_of(self.train, self.q, self.removed, self.items, self.ratings)

    @property
    def pred_items(self):
        """every train item (the removed and the re-rated ones, the item that left and c's other train items among them), the
        additional items, an item nobody rates in train, one item unknown to aug"""
        return np.concatenate([np.unique(self.train[1]), self.items, [NEW_ITEM, UNKNOWN_ITEM]]).astype(np.int32)

    @property
    def query(self):
        return (self.q, self.removed, self.items, self.ratings)


def _case(name, train, c, removed, items, ratings, k, **note):
    return RCase(name, train, c, np.asarray(items, dtype=np.int32), np.asarray(ratings, dtype=np.float64), k, _others(train, c), dict(note),
                 np.asarray(removed, dtype=np.int32))


def is_dyadic(train):
    """the premise under which the fit sums exactly: every rating a small multiple of 1/16"""
    v = train[2] * 16.0
    return bool(np.all(v == np.rint(v)) and np.all(np.abs(v) <= 16777216.0))


def removes_3(synth, k=5, name=None):
    """user 5 takes out its first, its middle and its last train row in file order; nothing is added"""
    train = base_train(synth)
    mine = _rows(train, CHANGER)[0]
    return _case(name or f"removes-3-k{k}", train, CHANGER, mine[[0, len(mine) // 2, -1]], [], [], k)


def _other_value(r, dyadic):
    return float(r - 2 if r >= 3 else r + 2) if dyadic else float(np.round(5.9 - r, 2))


def re_rates_dyadic(synth, k=5):
    """on the base fit: two items removed and given again with another value, plus one plain addition between them"""
    train = base_train(synth)
    mine, vals = _rows(train, CHANGER)
    pick = [1, len(mine) - 2]
    items = [mine[pick[0]], unrated(train, CHANGER, 1)[0], mine[pick[1]]]
    ratings = [_other_value(vals[pick[0]], True), 4.5, _other_value(vals[pick[1]], True)]
    return _case("re-rates-dyadic", train, CHANGER, mine[pick], items, ratings, k)


# ---- re-rates: the place and the deviation of c's terms once rows have gone ---------------------------------------------------
SLIPS = ("rerated-at-train-row", "removed-still-a-term", "train-deviation", "rerated-first")


def fold_terms(oracle, case, sim, v, item):
    """the terms of (v, item)'s fold on aug as the reference adds them: (rater, deviation on aug, knn similarity of (v, rater)) of
    the item's rows in aug's file order, on a fresh pipeline whose first evaluation is v's"""
    u, i, _ = case.aug
    m = oracle.Model(*case.aug)
    dev = m.normalized_deviations()
    p = m.pipeline(sim, case.k)
    return [(int(u[t]), float(dev[t]), p.knn_similarity(v, int(u[t]))) for t in np.flatnonzero(i == item)]


def slipped_terms(case, rows, item, slip, train_dev):
    """the (deviation, similarity) terms of an item's fold with one planted slip about the changer c = case.q; rows =
    fold_terms(...), train_dev[t] = the deviation of train file row t on train"""
    tu, ti, _ = case.train
    terms = [(dv, s) for (_, dv, s) in rows]
    mine = [x for x, r in enumerate(rows) if r[0] == case.q]
    raters = [int(t) for t in np.flatnonzero(ti == item)]  # train file rows of the item
    c_row = next((t for t in raters if tu[t] == case.q), None)
    removed, given = item in case.removed.tolist(), item in case.items.tolist()
    if c_row is None:
        return terms
    place = sum(1 for t in raters if t < c_row)  # c's place among the item's train raters; the others keep their order on aug
    if removed and given:
        x = mine[0]  # (the last term: the additional row)
        rest = terms[:x] + terms[x + 1:]
        if slip == "rerated-at-train-row":
            return rest[:place] + [terms[x]] + rest[place:]
        if slip == "removed-still-a-term":
            return terms[:place] + [(float(train_dev[c_row]), terms[x][1])] + terms[place:]
        if slip == "rerated-first":
            return [terms[x]] + rest
    elif removed and slip == "removed-still-a-term":
        s = next((r[2] for r in rows if r[0] == case.q), None)
        return terms if s is None else terms[:place] + [(float(train_dev[c_row]), s)] + terms[place:]
    elif not removed and slip == "train-deviation":
        x = mine[0]
        terms[x] = (float(train_dev[c_row]), terms[x][1])
    return terms


def re_rates(synth, oracle):
    """The off-scale ratings (sums round) at k = 59, so that c is in every list.  c removes three train items and gives two of
    them again with another value, plus one plain addition.  The picks are searched (seeds 0, 1, ...) until every slip of SLIPS
    changes the bits of some (bystander, item) prediction; returns (case, witnesses), witnesses[slip] = (bystander, item)."""
    base = bc.off_scale(synth)
    train, neg = base.train, base.note["negative"]
    sim = oracle.SIM_COSINE
    users = [u for u in _users(train) if u not in (CHANGER, neg)][:12]
    train_dev = oracle.Model(*train).normalized_deviations()
    mine, vals = _rows(train, CHANGER)
    for seed in range(40):
        rng = np.random.default_rng(seed)
        pick = rng.choice(len(mine), 3, replace=False)
        items = [mine[pick[0]], unrated(train, CHANGER, 1, skip=seed % 5)[0], mine[pick[1]]]
        ratings = [_other_value(vals[pick[0]], False), float(np.round(rng.uniform(0.6, 4.8), 2)), _other_value(vals[pick[1]], False)]
        case = _case("re-rates", train, CHANGER, mine[pick], items, ratings, 59, negative=neg)
        m = oracle.Model(*case.aug)
        live = [int(x) for x in mine if int(x) not in case.removed.tolist()][:4]
        found = {}
        for v in users:
            avg = m.users_avg(v)
            for item in [int(x) for x in case.removed] + live:
                want = m.pipeline(sim, 59).predict(v, item)
                rows = fold_terms(oracle, case, sim, v, item)
                if _bits([fold_predict(oracle, avg, [(dv, s) for (_, dv, s) in rows])]) != _bits([want]):
                    raise AssertionError(("the plain fold is not the oracle's", v, item))
                for slip in SLIPS:
                    if slip not in found and _bits([fold_predict(oracle, avg, slipped_terms(case, rows, item, slip, train_dev))]) != _bits([want]):
                        found[slip] = (v, item)
            if len(found) == len(SLIPS):
                return case, found
    raise AssertionError("no seed gives a witness for every slip")


# ---- lone-item: an item that only c rates in train ----------------------------------------------------------------------------
def lone_train(synth):
    """the base file with one extra row of c on LONE_ITEM, which nobody else rates, in the middle of c's rows"""
    u, i, r = base_train(synth)
    at = int(np.flatnonzero(u == CHANGER)[3]) + 1
    return (np.insert(u, at, CHANGER).astype(np.int32), np.insert(i, at, LONE_ITEM).astype(np.int32), np.insert(r, at, 4.5))


def lone_item(synth, k=5):
    """removed: the item leaves aug; removed and re-rated: exactly one rater, the last of aug; kept: another row goes instead"""
    train = lone_train(synth)
    other = _rows(train, CHANGER)[0][0]
    return [_case("lone-item-removed", train, CHANGER, [LONE_ITEM], [], [], k),
            _case("lone-item-rerated", train, CHANGER, [LONE_ITEM], [LONE_ITEM], [1.5], k),
            _case("lone-item-kept", train, CHANGER, [other], [], [], k)]


# ---- membership: c leaves one full list and enters another ------------------------------------------------------------------
def list_changes(oracle, case, sim):
    """the bystanders whose list c = case.q leaves and enters between train and aug"""
    mt, ma = oracle.Model(*case.train), oracle.Model(*case.aug)
    leaves, enters = [], []
    for v in case.others:
        if v == UNKNOWN_USER:
            continue
        a = mt.pipeline(sim, case.k).neighbors(v)[0].tolist()
        b = ma.pipeline(sim, case.k).neighbors(v)[0].tolist()
        if case.q in a and case.q not in b:
            leaves.append(v)
        elif case.q not in a and case.q in b:
            enters.append(v)
    return leaves, enters


def membership(synth, oracle, k=5):
    """removals of user 5 (seeds 0, 1, ...: 2-8 of its train items, nothing added) after which it has left some bystander's full
    list and entered another's"""
    train = base_train(synth)
    mine = _rows(train, CHANGER)[0]
    for seed in range(60):
        rng = np.random.default_rng(seed)
        pick = rng.choice(len(mine), int(rng.integers(2, 9)), replace=False)
        case = _case("membership", train, CHANGER, mine[pick], [], [], k)
        leaves, enters = list_changes(oracle, case, oracle.SIM_COSINE)
        if leaves and enters:
            case.note.update(leaves=leaves, enters=enters)
            return case
    raise AssertionError("no seed moves the changer both ways")


# ---- tiny: <= 4 ratings on both sides ---------------------------------------------------------------------------------------
def tiny(synth, oracle, k=5):
    """On the train set of bystander_cases.tiny_rows (users of 1, 3 and 4 ratings whose file order is the reverse of their trie
    order): a changer of more than 4 rows keeps its first 3 and adds one on an item of the 4-rating user — 4 rows in aug"""
    base = bc.tiny_rows(synth, oracle)[0]
    train, tiny_users = base.train, base.note["tiny"]
    u4 = list(tiny_users)[2]
    c = next(u for u in _users(train) if u not in tiny_users and len(_rows(train, u)[0]) > 6)
    mine = _rows(train, c)[0]
    add = next(int(x) for x in _rows(train, u4)[0] if int(x) not in mine.tolist())
    return _case("tiny", train, c, mine[3:], [add], [1.75], k, tiny=dict(tiny_users))


# ---- off-scale: average(aug) is no continuation of the running total ------------------------------------------------------------
def shortcut_average(case):
    """what continuing the fit's running total would give: fold(train) - the removed ratings + the added ones, over the count"""
    u, i, r = case.train
    t = 0.0
    for x in r:
        t = t + float(x)
    gone = (u == case.q) & np.isin(i, case.removed)
    for x in r[gone]:
        t = t - float(x)
    for x in case.ratings:
        t = t + float(x)
    return t / float(len(r) - int(gone.sum()) + len(case.ratings))


def off_scale(synth, oracle, k=5):
    """the non-dyadic fit: c removes its first and its last train row in file order and adds two off-scale ratings.  Past 2048
    the running total moves on one grid, so whether the shortcut's bits differ from average(aug) is mostly a matter of WHERE the
    removed rows stand: the changer is searched from user 5 on (then the added ratings, seeds) until they do"""
    base = bc.off_scale(synth)
    train, neg = base.train, base.note["negative"]
    users = _users(train)
    for c in users[users.index(CHANGER):]:
        if c == neg:
            continue
        mine = _rows(train, c)[0]
        for seed in range(4):
            rng = np.random.default_rng(seed)
            case = _case("off-scale", train, c, mine[[0, -1]], unrated(train, c, 2), np.round(rng.uniform(0.3, 5.6, 2), 2), k, negative=neg)
            if _bits([shortcut_average(case)]) != _bits([oracle.Model(*case.aug).average()]):
                return case
    raise AssertionError("no changer separates the shortcut from the fold")


def all_cases(synth, oracle):
    return ([removes_3(synth, k) for k in (5, 59, 300)] + [re_rates(synth, oracle)[0], re_rates_dyadic(synth)] + lone_item(synth)
            + [membership(synth, oracle), tiny(synth, oracle), off_scale(synth, oracle)])


NAMES = ["removes-3-k5", "removes-3-k59", "removes-3-k300", "re-rates", "re-rates-dyadic", "lone-item-removed", "lone-item-rerated",
         "lone-item-kept", "membership", "tiny", "off-scale"]
JACCARD_NAMES = [n for n in NAMES if n != "membership"]  # (its removals are searched on the cosine lists)


def expected(oracle, case, sim):
    return bc.expected(oracle, case, sim)
