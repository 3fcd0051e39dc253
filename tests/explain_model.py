"""The terms behind a kNN prediction, from the CPU oracle alone (helper of test_explain_model.py and test_gpu_explain.py).

weightedSumDeviation shared/predictions.scala:504-548 walks the item's training rows in file order, pairs each rater's
normalized deviation with getSimilarity(u, rater) :513-517 and folds (num + dev * sim, den + |sim|) from (0.0, 0.0) :520-524.
TermModel rebuilds that from three oracle answers — Pipeline.neighbors(u) (getSimilarity is the list's value for a listed
user and 0.0 for everybody else, :634-648), Model.normalized_deviations() and a walk of the training file for the item's rows —
keeps the raters whose similarity is non-zero (the terms), and combines with oracle.scale :578.  Nothing here asks the oracle
for a wsd or a prediction: those are what test_explain_model.py compares the fold against.

rows() calls the pipeline in the batch's row order, and only for a row whose user is known and whose item has raters — where
the reference's lazy closure would build the user's neighbourhood — so the memo history matches the engine's."""
from dataclasses import dataclass

import numpy as np

SUM_ORDER, BY_WEIGHT = 0, 1


@dataclass
class Row:
    raters: np.ndarray      # int32 raw ids of the terms, summation order (training file order of the item's raters)
    sims: np.ndarray        # float64
    devs: np.ndarray        # float64
    by_weight: np.ndarray   # the permutation of the terms under (|sim| descending, summation order ascending)
    num: float
    den: float
    prediction: float

    @property
    def count(self):
        return len(self.raters)

    def terms(self, order):
        """(raters, sims, devs) in the requested order"""
        if order == SUM_ORDER:
            return self.raters, self.sims, self.devs
        return self.raters[self.by_weight], self.sims[self.by_weight], self.devs[self.by_weight]


def fold(sims, devs):
    """the left fold :520-524 of the terms as given"""
    num, den = 0.0, 0.0
    for s, d in zip(np.asarray(sims, dtype=np.float64).tolist(), np.asarray(devs, dtype=np.float64).tolist()):
        num = num + d * s
        den = den + abs(s)
    return num, den


def combine(oracle, ua, num, den):
    """predictor :578 from the user's mean and the fold's sums"""
    wsd = num / den if den > 0 else 0.0
    return ua + wsd * oracle.scale(ua + wsd, ua)


class TermModel:
    def __init__(self, oracle, model, sim_kind, k, pipeline=None):
        """pipeline: an existing Pipeline(model, sim_kind, k) whose memo the terms share (tests/call_sequences.py); a fresh one
        by default"""
        self.oracle, self.model = oracle, model
        self.pipeline = pipeline if pipeline is not None else model.pipeline(sim_kind, k)
        self.dev = model.normalized_deviations()
        order = np.argsort(model.items, kind="stable")  # (stable: the rows of an item stay in file order)
        items, first = np.unique(model.items[order], return_index=True)
        ends = np.append(first[1:], len(order))
        self.item_rows = {int(i): order[a:b] for i, a, b in zip(items, first, ends)}
        self.known_users = set(np.unique(model.users).tolist())
        self._lists = {}

    def _neighbors(self, u):
        if u not in self._lists:
            ids, sims = self.pipeline.neighbors(u)
            self._lists[u] = dict(zip(ids.tolist(), sims.tolist()))
        return self._lists[u]

    def row(self, u, i):
        u, i = int(u), int(i)
        empty = (np.empty(0, np.int32), np.empty(0), np.empty(0), np.empty(0, np.int64), 0.0, 0.0)
        if u not in self.known_users:
            return Row(*empty, self.model.average())
        ua = self.model.users_avg(u)
        rows = self.item_rows.get(i)
        if rows is None:
            return Row(*empty, combine(self.oracle, ua, 0.0, 0.0))
        near = self._neighbors(u)
        raters, sims, devs = [], [], []
        for t in rows.tolist():
            x = int(self.model.users[t])
            s = near.get(x, 0.0)
            if s != 0.0:
                raters.append(x)
                sims.append(s)
                devs.append(float(self.dev[t]))
        num, den = fold(sims, devs)
        by_weight = sorted(range(len(sims)), key=lambda c: (-abs(sims[c]), c))
        return Row(np.asarray(raters, np.int32), np.asarray(sims, np.float64), np.asarray(devs, np.float64),
                   np.asarray(by_weight, np.int64), num, den, combine(self.oracle, ua, num, den))

    def rows(self, users, items):
        return [self.row(u, i) for u, i in zip(np.asarray(users).tolist(), np.asarray(items).tolist())]


# ---- the small structured inputs of both test files (tests/degenerate.py generators at a size the oracle walks in seconds) ----
def disjoint_case():
    """144 ordinary users + 16 whose training items nobody else rates: similarity exactly 0.0 with everybody"""
    from tests import degenerate

    return degenerate.cold(160, 16, n_items=120, per_user=25, seed=171)


def clone_case():
    """two mirrored prototype rows held by 16 users each: exact ties of |similarity| under both signs"""
    from tests import degenerate

    return degenerate.clones(160, 2, 16, n_items=120, per_user=25, seed=272)


# ---- a small dense train for the match-count and kernel-class edges: k >= U - 1 makes kcap = U - 1 ----------------------------
def dense_train(n_users, seed):
    """every user rates item 1 and six of the items 2..40 (more than 4 ratings each), rows shuffled: U - 1 matches on item 1"""
    rng = np.random.default_rng(seed)
    others = np.argsort(rng.random((n_users, 39)), axis=1)[:, :6] + 2
    items = np.concatenate([np.ones((n_users, 1), dtype=np.int64), others], axis=1)
    # item 1 gets a 5 and the user's other items one lower value: the mean lies between, every deviation on item 1 is positive
    # and every other one negative, so the products over any two users' common items are all positive — no similarity is 0.0
    ratings = np.repeat(rng.integers(1, 5, (n_users, 1)), 7, axis=1).astype(np.float64)
    ratings[:, 0] = 5.0
    users = np.repeat(rng.permutation(n_users) + 1, 7)
    rows = rng.permutation(len(users))
    return users[rows].astype(np.int32), items.reshape(-1)[rows].astype(np.int32), ratings.reshape(-1)[rows]


def dense_rows(tr):
    users = np.unique(tr[0])
    u = np.array([users[0], users[len(users) // 2], users[-1], users[1], users[2]], dtype=np.int32)
    return u, np.array([1, 1, 1, 7, 876_543], dtype=np.int32)
