"""Deterministic STRUCTURED rating sets for the degenerate-row tests (numpy only; the product's synth.py draws i.i.d. rows,
whose similarity distributions are all smooth).

Every generator lays one planted sub-population over a background of ordinary users (Zipf item popularity, log-normal
activity, whole-star ratings from user and item biases — the density of synth.syn_scaled) and returns a Case: train and
test column triples (users int32, items int32, ratings float64) in a seeded shuffled row order, and the raw ids of every
population.  Ratings are whole stars 1..5 (scale() is never 0), every user keeps at least 5 training ratings (the <= 4-rating
memo-order rule, SURVEY N6, stays out of it), raw user ids are a seeded permutation of 1..U (planted users are scattered
over the dense index range).

  cold      users whose 6 training ratings lie in a private item range: similarity exactly 0.0 with (nearly) everybody
  clones    prototype rows copied under many ids: similarities to a third user equal up to an ulp of the copies' norms (the
            reference folds a row's squares in an order that depends on the user id), ~1.0 to each other: ties hundreds wide
  camps     two camps rating one shared item set with opposite 1/5 patterns: strongly negative rows for the small camp
  constant  users whose ratings are all equal: zero deviations, zero norm, cosine similarity 0 with everybody
            (n_const of cold / clones mixes them in)

CASES names the exact parameter sets that tests/test_gpu_degenerate_rows.py runs and tests/test_degenerate_premises.py
checks against the oracle; case(name) builds each once per process."""
import functools
from dataclasses import dataclass, field

import numpy as np


@dataclass
class Case:
    train: tuple
    test: tuple
    groups: dict = field(default_factory=dict)  # population name -> sorted raw user ids (int32)

    @property
    def num_users(self):
        return len(np.unique(self.train[0]))


class _Rows:
    """(local user, raw item, rating, is_test) pieces, concatenated and shuffled at the end"""

    def __init__(self):
        self.u, self.i, self.r, self.t = [], [], [], []

    def add(self, u, i, r, is_test):
        u = np.asarray(u, dtype=np.int64)
        self.u.append(u)
        self.i.append(np.asarray(i, dtype=np.int64))
        self.r.append(np.asarray(r, dtype=np.float64))
        self.t.append(np.broadcast_to(np.asarray(is_test, dtype=bool), u.shape).copy())

    def finish(self, rng, n_users, groups):
        u, i, r, t = (np.concatenate(x) for x in (self.u, self.i, self.r, self.t))
        raw = (rng.permutation(n_users) + 1).astype(np.int32)  # local user -> raw id
        keys = u * (1 << 32) + i
        assert len(np.unique(keys)) == len(keys), "a (user, item) pair twice"
        assert r.min() >= 1.0 and r.max() <= 5.0 and np.array_equal(r, np.round(r))
        assert np.bincount(u[~t], minlength=n_users).min() >= 5, "a user with fewer than 5 training ratings"
        out = []
        for part in (~t, t):
            ix = rng.permutation(np.flatnonzero(part))
            out.append((raw[u[ix]], i[ix].astype(np.int32), r[ix].copy()))
        return Case(out[0], out[1], {name: np.sort(raw[np.asarray(loc, dtype=np.int64)]) for name, loc in groups.items()})


def _popularity(rng, n_items):
    """(cdf over popularity ranks, raw item id of every rank): shifted Zipf over a random permutation of 1..n_items"""
    w = 1.0 / (np.arange(n_items, dtype=np.float64) + 10.0)
    cdf = np.cumsum(w / w.sum())
    cdf[-1] = 1.0
    return cdf, rng.permutation(n_items).astype(np.int64) + 1


def _draw_items(rng, cdf, item_of_rank, users, n_draws):
    """distinct (user, item) pairs from n_draws popularity draws per user, sorted by (user, item)"""
    u = np.repeat(np.asarray(users, dtype=np.int64), n_draws)
    it = item_of_rank[np.minimum(np.searchsorted(cdf, rng.random(len(u))), len(cdf) - 1)]
    key = np.unique(u * (1 << 32) + it)
    return key >> 32, key & 0xFFFFFFFF


def _background(rows, rng, users, cdf, item_of_rank, per_user):
    """ordinary users: about per_user ratings each (log-normal), ratings from user + item biases; the first 5 ratings of a
    user always train, the others test with probability 0.2"""
    n_items = len(cdf)
    counts = np.clip(rng.lognormal(np.log(per_user) - 0.28, 0.75, len(users)), 12, n_items // 3).astype(np.int64)
    u, it = _draw_items(rng, cdf, item_of_rank, users, counts + counts // 4 + 4)
    ub = np.zeros(int(np.max(users)) + 1)
    ub[users] = rng.normal(0.0, 0.45, len(users))
    ib = rng.normal(0.0, 0.45, n_items + 1)
    r = np.clip(np.round(3.35 + ub[u] + ib[it] + rng.normal(0.0, 0.95, len(u))), 1.0, 5.0)
    prio = rng.random(len(u))
    order = np.lexsort((prio, u))
    start = np.flatnonzero(np.concatenate([[True], u[order][1:] != u[order][:-1]]))
    rank = np.arange(len(u)) - np.repeat(start, np.diff(np.concatenate([start, [len(u)]])))
    is_test = np.zeros(len(u), dtype=bool)
    is_test[order] = (rank >= 5) & (rng.random(len(u)) < 0.2)
    rows.add(u, it, r, is_test)


def _constant(rows, rng, users, cdf, item_of_rank):
    """14 background items per user, every rating (2 test rows included) the same whole star"""
    if len(users) == 0:
        return
    u, it = _draw_items(rng, cdf, item_of_rank, users, np.full(len(users), 40))
    star = np.zeros(int(np.max(users)) + 1)
    star[users] = rng.integers(2, 5, len(users))
    for x in users:
        m = np.flatnonzero(u == x)[:14]
        assert len(m) == 14
        rows.add(u[m], it[m], star[u[m]], np.arange(14) >= 12)


def cold(U, n_cold, n_const=0, n_items=3000, per_user=75, seed=101):
    """U users: n_cold cold ones (6 training ratings in a private item range above n_items, 2 test rows on popular
    background items), n_const constant ones, the rest background"""
    rng = np.random.Generator(np.random.PCG64(seed))
    cdf, item_of_rank = _popularity(rng, n_items)
    n_bg = U - n_cold - n_const
    bg, cd, cs = np.arange(n_bg), np.arange(n_bg, n_bg + n_cold), np.arange(n_bg + n_cold, U)
    rows = _Rows()
    _background(rows, rng, bg, cdf, item_of_rank, per_user)
    _constant(rows, rng, cs, cdf, item_of_rank)
    private = n_items + 1 + rng.integers(0, 1_000_000, size=(n_cold, 6))  # (two cold users rarely share an item)
    for j, x in enumerate(cd):
        its = np.unique(private[j])
        while len(its) < 6:
            its = np.unique(np.concatenate([its, n_items + 1 + rng.integers(0, 1_000_000, size=6 - len(its))]))
        r = rng.integers(1, 6, 6).astype(np.float64)
        r[0], r[1] = 1.0, 5.0  # never constant
        rows.add(np.full(6, x), its, r, False)
        rows.add(np.full(2, x), item_of_rank[[2 * (j % 8), 2 * (j % 8) + 1]], rng.integers(1, 6, 2), True)
    return rows.finish(rng, U, {"background": bg, "cold": cd, "constant": cs})


def clones(U, group, copies, n_const=0, n_items=600, per_user=60, seed=202):
    """group prototype rows of 40 background items, each held by `copies` users (training rows identical; one test row each on
    an item outside the prototype), n_const constant users, the rest background"""
    rng = np.random.Generator(np.random.PCG64(seed))
    cdf, item_of_rank = _popularity(rng, n_items)
    n_cl = group * copies
    n_bg = U - n_cl - n_const
    assert n_bg > 0
    bg, cl, cs = np.arange(n_bg), np.arange(n_bg, n_bg + n_cl), np.arange(n_bg + n_cl, U)
    rows = _Rows()
    _background(rows, rng, bg, cdf, item_of_rank, per_user)
    _constant(rows, rng, cs, cdf, item_of_rank)
    # Prototypes come in mirrored pairs (g, g + group / 2): the same 40 items — every (group / 2)-th of the most popular ones,
    # so that nearly every background user shares some — with ratings r and 6 - r.  Mirroring negates every normalized
    # deviation exactly, so a third user's similarities to the two are s and -s: one of the two groups of `copies` users is on
    # the positive side of (nearly) every background row, which keeps those rows ordinary at k < copies.
    assert group % 2 == 0
    half = group // 2
    protos = []
    for g in range(half):
        r = rng.integers(1, 6, 40).astype(np.float64)
        r[0], r[1] = 1.0, 5.0
        protos.append((item_of_rank[g + half * np.arange(40)], r))
    protos += [(its, 6.0 - r) for its, r in protos]
    for g, (its, r) in enumerate(protos):
        members = cl[g * copies:(g + 1) * copies]
        rows.add(np.repeat(members, 40), np.tile(its, copies), np.tile(r, copies), False)
        others = np.setdiff1d(np.arange(1, n_items + 1), its)
        rows.add(members, rng.choice(others, copies), rng.integers(1, 6, copies), True)
    groups = {"background": bg, "clones": cl, "constant": cs}
    groups.update({f"clones{g}": cl[g * copies:(g + 1) * copies] for g in range(group)})
    return rows.finish(rng, U, groups)


def camps(U, n_a, n_shared=24, seed=303):
    """n_a users of camp A rate the shared items 1..n_shared with one fixed 1/5 pattern, the U - n_a users of camp B with the
    opposite one; every user flips one or two entries, leaves two shared items out of the training rows (one of them is its
    test row) and rates three filler items of a wide range that hardly anybody shares"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pattern = np.where(rng.permutation(n_shared) < n_shared // 2, 1.0, 5.0)
    a, b = np.arange(n_a), np.arange(n_a, U)
    r = np.tile(pattern, (U, 1))
    r[n_a:] = 6.0 - r[n_a:]
    order = np.argsort(rng.random((U, n_shared)), axis=1)  # per user: columns 0..1 flipped, columns 2..3 left out
    n_flip = rng.integers(1, 3, U)
    for c in range(2):
        m = np.flatnonzero(n_flip > c)
        r[m, order[m, c]] = 6.0 - r[m, order[m, c]]
    keep = np.ones((U, n_shared), dtype=bool)
    keep[np.arange(U), order[:, 2]] = False
    keep[np.arange(U), order[:, 3]] = False
    uu = np.repeat(np.arange(U), n_shared).reshape(U, n_shared)
    ii = np.tile(np.arange(1, n_shared + 1), (U, 1))
    rows = _Rows()
    rows.add(uu[keep], ii[keep], r[keep], False)
    rows.add(np.arange(U), ii[np.arange(U), order[:, 2]], r[np.arange(U), order[:, 2]], True)
    filler = n_shared + 1 + rng.integers(0, 2_000_000, size=(U, 3))
    filler[:, 1] += 2_000_000  # (the three of a user are distinct)
    filler[:, 2] += 4_000_000
    rows.add(np.repeat(np.arange(U), 3), filler.reshape(-1), rng.integers(1, 6, 3 * U), False)
    return rows.finish(rng, U, {"camp_a": a, "camp_b": b})


K = 300  # the neighbourhood size of every case but the clones' second one
CASES = {
    "cold40": lambda: cold(20_480, 40, n_const=50),
    "cold160": lambda: cold(20_480, 160),
    "cold_wide": lambda: cold(70_000, 24, n_items=4000, per_user=30, seed=111),
    "camps12k": lambda: camps(12_000, 100),
    "camps20k": lambda: camps(20_480, 100, seed=313),
    "clones": lambda: clones(3_200, 4, 700, n_const=50),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def every(ids, step):
    """every step-th id of a population (the background may be sampled; planted rows never are)"""
    return np.asarray(ids)[::step]


# the background (camps: camp B) users that stand for the ordinary rows of each case, in both test files
SAMPLE_STEP = {"cold40": 29, "cold160": 29, "cold_wide": 5800, "camps12k": 97, "camps20k": 97, "clones": 7}


def ordinary_sample(name):
    c = case(name)
    return every(c.groups["camp_b" if name.startswith("camps") else "background"], SAMPLE_STEP[name])
