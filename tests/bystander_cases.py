"""Inputs of the bystander-query tests (knncf_query_bystander_*: a fitted user's kNN answers once a newcomer has joined),
shared by test_bystander_premises.py (CPU, oracle only: the inputs reach the cases) and test_gpu_bystander.py.

A case is a Case: the train set, the newcomer q with its rows, the handle's k, the bystanders and the items to ask for.  The
base fit is synth.syn_scaled(60, 80, 1500, 3).train: 60 users, 80 items, 1200 ratings, rows of 11-39."""
from dataclasses import dataclass, field

import numpy as np

from tests.query_helpers import UNKNOWN_ITEM, _aug, _bits

NEW_ITEM = 5000
UNKNOWN_USER = 7777


@dataclass
class Case:
    name: str
    train: tuple          # (users, items, ratings), file order
    q: int                # the newcomer's raw id
    items: np.ndarray     # its rows, in the given order
    ratings: np.ndarray
    k: int
    others: list          # the bystanders asked for
    note: dict = field(default_factory=dict)

    @property
    def aug(self):
        return _aug(self.train, self.q, self.items, self.ratings)

    @property
    def pred_items(self):
        """every train item, the newcomer's items, the item only a newcomer rates, one item unknown to aug"""
        return np.concatenate([np.unique(self.train[1]), self.items, [NEW_ITEM, UNKNOWN_ITEM]]).astype(np.int32)


def trie_sorted(oracle, ids):
    """ids in the iteration order of a hash set of MORE than 4 elements (a Set1..Set4 iterates in insertion order instead,
    which is all that oracle.int_set_order shows for so few ids)"""
    return sorted((int(x) for x in ids), key=lambda x: oracle.trie_key(oracle.improve(x)))


def base_train(synth):
    t = synth.syn_scaled(60, 80, 1500, 3).train
    return (t.users.copy(), t.items.copy(), t.ratings.copy())


def _users(train):
    return [int(u) for u in np.unique(train[0])]


def _rows(train, u):
    idx = np.flatnonzero(train[0] == u)
    return train[1][idx].copy(), train[2][idx].copy()


def near_clone(synth, k=5, q=1000, train=None, name="near-clone"):
    """q's rows are a fitted user c's rows with one rating changed"""
    train = base_train(synth) if train is None else train
    c = _users(train)[4]
    it, rt = _rows(train, c)
    rt[len(rt) // 2] = 1.0 if rt[len(rt) // 2] != 1.0 else 2.0
    return Case(name, train, q, it, rt, k, _users(train), {"clone_of": c})


def short_lists(synth):
    """k >= the number of other users: no list is full, q enters every one"""
    return [near_clone(synth, k=59, name="short-59"), near_clone(synth, k=300, name="short-300")]


def new_item(synth, k=5):
    """q also rates an item that is unknown to train"""
    c = near_clone(synth, k=k, name="new-item")
    at = len(c.items) // 3
    c.items = np.concatenate([c.items[:at], [NEW_ITEM], c.items[at:]]).astype(np.int32)
    c.ratings = np.concatenate([c.ratings[:at], [4.5], c.ratings[at:]])
    return c


def tie(synth, oracle):
    """q is an exact copy of a fitted user w (same items, ratings and order).  The norm folds in tuple_trie_key(q, item) order,
    so whether S(v, q) == S(v, w) bitwise depends on the id: the builder searches raw ids 1000, 1001, ... and returns two cases,
    one whose id sorts BEFORE w in set order and one AFTER, each with a (bystander, k) at which q and w tie bitwise and sit on
    both sides of the cut k."""
    train = base_train(synth)
    users = _users(train)
    w = users[10]
    it, rt = _rows(train, w)
    found = {}
    for q in range(1000, 1200):
        assert trie_sorted(oracle, users + [q]) == oracle.int_set_order(users + [q])
        side = "before" if trie_sorted(oracle, [q, w])[0] == q else "after"
        if side in found:
            continue
        m = oracle.Model(*_aug(train, q, it, rt))
        for v in users:
            if v == w or _bits([m.fresh_similarity(oracle.SIM_COSINE, v, q)]) != _bits([m.fresh_similarity(oracle.SIM_COSINE, v, w)]):
                continue
            ids = m.pipeline(oracle.SIM_COSINE, len(users)).neighbors(v)[0].tolist()
            a, b = sorted((ids.index(q), ids.index(w)))
            if b == a + 1:  # nobody else ties with them: the cut between the two
                found[side] = Case(f"tie-{side}", train, q, it, rt, b, users, {"copy_of": w, "bystander": v, "side": side})
                break
        if len(found) == 2:
            break
    assert len(found) == 2, found.keys()
    return [found["before"], found["after"]]


def tiny_rows(synth, oracle):
    """three users trimmed to 1, 3 and 4 ratings whose file order is the REVERSE of their trie order (the rows are moved to
    the end of the file), and newcomers of 1, 4 and 5 ratings in non-ascending item order that share the tiny users' items.
    The ratings are searched (seeds 0, 1, ...) until a tiny bystander's S(v, q) differs bitwise from S(q, v) for some pair."""
    base = base_train(synth)
    users = _users(base)
    tiny = {users[1]: 1, users[2]: 3, users[3]: 4}
    for seed in range(200):
        rng = np.random.default_rng(seed)
        keep = ~np.isin(base[0], list(tiny))
        tu, ti, tr_ = [base[0][keep]], [base[1][keep]], [base[2][keep]]
        rows = {}
        for u, n in tiny.items():
            it = _rows(base, u)[0][:n]
            it = np.asarray(trie_sorted(oracle, it)[::-1], dtype=np.int32)
            rt = np.round(rng.uniform(1.0, 5.0, n), 2)
            rows[u] = (it, rt)
            tu.append(np.full(n, u, dtype=np.int32)); ti.append(it); tr_.append(rt)
        train = (np.concatenate(tu).astype(np.int32), np.concatenate(ti).astype(np.int32), np.concatenate(tr_))
        u1, u3, u4 = list(tiny)
        free = [int(x) for x in np.unique(base[1]) if x not in set(rows[u3][0].tolist()) | set(rows[u4][0].tolist())]
        newcomers = [
            (2001, rows[u1][0].copy(), np.round(rng.uniform(1.0, 5.0, 1), 2)),
            (2002, np.concatenate([rows[u3][0][::-1][1:], [free[0]], rows[u3][0][::-1][:1]]).astype(np.int32), np.round(rng.uniform(1.0, 5.0, 4), 2)),
            (2003, np.concatenate([[free[1]], rows[u4][0][2:], rows[u4][0][:2]]).astype(np.int32), np.round(rng.uniform(1.0, 5.0, 5), 2)),
        ]
        cases = [Case(f"tiny-{len(it)}", train, q, it, rt, 5, _users(train), {"tiny": dict(tiny)}) for q, it, rt in newcomers]
        try:
            differs = False
            for c in cases:
                m = oracle.Model(*c.aug)
                for v in tiny:
                    differs |= _bits([m.fresh_similarity(oracle.SIM_COSINE, v, c.q)]) != _bits([m.fresh_similarity(oracle.SIM_COSINE, c.q, v)])
        except oracle.OracleError:
            continue  # (a scale() == 0 input: the next seed replaces it)
        if differs:
            return cases
    raise AssertionError("no seed gives an order-dependent tiny pair")


def off_scale(synth):
    """ratings round(r * 0.93 + 0.1, 2), so that sums round; one fitted user with a negative mean; one bystander id unknown
    to aug"""
    u, i, r = base_train(synth)
    r = np.round(r * 0.93 + 0.1, 2)
    users = _users((u, i, r))
    neg = users[7]
    r[u == neg] = np.round(r[u == neg] - 6.0, 2)
    c = near_clone(synth, k=5, train=(u, i, r), name="off-scale")
    c.others = users + [UNKNOWN_USER]
    c.note["negative"] = neg
    return c


def all_cases(synth, oracle):
    return [near_clone(synth)] + tie(synth, oracle) + short_lists(synth) + tiny_rows(synth, oracle) + [new_item(synth), off_scale(synth)]


def expected(oracle, case, sim):
    """(neighbours per bystander, predictions [bystander][item]) of the oracle on aug, a fresh pipeline per row"""
    m = oracle.Model(*case.aug)
    nbrs = [m.pipeline(sim, case.k).neighbors(v) for v in case.others]
    preds = [[m.pipeline(sim, case.k).predict(v, int(i)) for i in case.pred_items] for v in case.others]
    return nbrs, preds
