"""Seeded rating sets OFF the MovieLens star scale (numpy only, nothing on disk): non-dyadic ratings, ratings outside
[1, 5], fitted users with a negative mean, and fits that sit on the two limits of prep.hip's dyadic rule (multiples of 1/16,
|r| <= 2^20) and on the FOLD_CHUNK = 2048 edges of its sequential average.  tests/test_rating_scale_premises.py proves from
the data, the oracle and the literal model that every case is what it claims to be; tests/test_gpu_rating_scales.py pins each
of them to the oracle.  scripts/fuzz_parity.py --rating-domain draws its ratings from rating_values() too."""
import functools
import importlib

import numpy as np

DOMAINS = ("tenths", "sixteenths", "thirtyseconds", "wide", "neg_users")
FOLD_CHUNK = 2048          # prep.hip: elements per LDS chunk of k_sequential_sum / k_ordered_fold (a literal here on purpose)
AVG_EDGE_N = (1, 5, 2047, 2048, 2049, 4096, 4097)
DYADIC_LIMIT = 1048576.0   # 2^20: k_check_dyadic accepts |r| * 16 <= 2^24
# wide100k: r' = A[u % 3] * r + B[u % 3] on the raw user id
WIDE_A = (1.7, 0.9, 1.7)
WIDE_B = (-5.3, 0.35, -0.5)
UNKNOWN_USER, UNKNOWN_ITEM = 999_999, 888_888


def rating_values(rng, domain, size):
    """`size` ratings of a domain (neg_users: the tenths; small_case shifts three users afterwards)"""
    if domain in ("tenths", "neg_users"):
        return rng.integers(5, 51, size=size) / 10.0            # 0.5 .. 5.0
    if domain == "sixteenths":
        return rng.integers(8, 81, size=size) / 16.0            # 0.5 .. 5.0, every one dyadic by the 1/16 rule
    if domain == "thirtyseconds":
        return rng.integers(16, 161, size=size) / 32.0          # 0.5 .. 5.0, half of them off the 1/16 grid
    if domain == "wide":
        return rng.integers(-60, 121, size=size) / 10.0         # -6.0 .. 12.0
    raise ValueError(f"unknown rating domain {domain!r}")


def small_case(rng, domain, n_users=14, n_items=15, n_ratings=90, tiny_rows=0):
    """rows (user, item, rating) with sparse raw ids in a shuffled file order, like test_oracle_semantics._random_case;
    tiny_rows adds users of 1..4 ratings (Set1..Set4: their summation order follows the insertion order).  neg_users: the
    three smallest user ids have every rating shifted by -7 (means below zero)."""
    pairs, rows = set(), []
    while len(rows) < n_ratings:
        u, i = int(rng.integers(1, n_users + 1)), int(rng.integers(1, n_items + 1))
        if (u, i) in pairs:
            continue
        pairs.add((u, i))
        rows.append((u * 7 + 3, i * 13 + 1, float(rating_values(rng, domain, 1)[0])))
    for t in range(tiny_rows):
        u = 10_000 + t
        for i in rng.choice(n_items, size=int(rng.integers(1, 5)), replace=False):
            rows.append((u, int(i + 1) * 13 + 1, float(rating_values(rng, domain, 1)[0])))
    if domain == "neg_users":
        low = set(sorted(set(u for u, _, _ in rows))[:3])
        rows = [(u, i, r - 7.0 if u in low else r) for u, i, r in rows]
    rng.shuffle(rows)
    return rows


def split_small(rows):
    """(train rows, test rows + one unknown user and one unknown item), the 4/5 cut of the existing small-case tests"""
    cut = len(rows) * 4 // 5
    train, test = rows[:cut], rows[cut:]
    return train, test + [(UNKNOWN_USER, train[0][1], 3.0), (train[0][0], UNKNOWN_ITEM, 4.0)]


def history_case():
    """(train rows, test rows): a neg_users case with four users of 1..4 ratings in which the memo history shows: the
    predictor answers a negative-mean user's test rows at :573 WITHOUT evaluating weightedSumDeviation, so that user's
    neighbourhood is not built there; building it at its first test row (as for every other fitted user) leaves other pairs
    with a <= 4-rating user summed from the other side, and two neighbour lists differ in their bits"""
    return split_small(small_case(np.random.default_rng([4321, 5]), "neg_users", tiny_rows=4))


def cols(rows):
    u, i, r = zip(*rows)
    return np.asarray(u, np.int32), np.asarray(i, np.int32), np.asarray(r, np.float64)


# ---- the average's fold at the FOLD_CHUNK edges ---------------------------------------------------------------------------
# The lone non-dyadic rating of variant (b) is x + 1/3, not x.1: beside exact (half-star) addends a sum can depend on its
# order only through double rounding, and the repeating 1001 / 0011 mantissas of the tenths never produce one (no seed of
# 300 did for any tenth; tests/test_rating_scale_premises.py keeps that observation as an assertion), so a fold in the wrong
# order or a missed flag would leave the bits alone.  The 0101 mantissa of a third ties at every dropped bit.
LONE_FRACTION = 1.0 / 3.0
# (n, where) -> seed: the first seed whose left fold differs in its bits from the k_exact_sum order (256-wide trees, then the
# block sums in ascending order); where == n - 1 (the lone rating is added last: one rounding in both orders) from the
# reversed or numpy's pairwise order instead.  n == 1 has one order only.
AVG_EDGE_SEEDS = {
    (1, None): 0, (1, 0): 0, (5, None): 3, (5, 0): 3, (5, 4): 4,
    (2047, None): 0, (2047, 0): 5, (2047, 255): 0, (2047, 256): 0, (2047, 2046): 0,
    (2048, None): 0, (2048, 0): 6, (2048, 255): 0, (2048, 256): 7, (2048, 2047): 0,
    (2049, None): 0, (2049, 0): 10, (2049, 255): 0, (2049, 256): 0, (2049, 2048): 0,
    (4096, None): 0, (4096, 0): 1, (4096, 255): 1, (4096, 256): 3, (4096, 4095): 0,
    (4097, None): 0, (4097, 0): 1, (4097, 255): 4, (4097, 256): 1, (4097, 4096): 0,
}


def avg_edge_wheres(n):
    """file rows of the lone non-dyadic rating: first thread, the two sides of a workgroup edge, last thread of k_check_dyadic"""
    return tuple(sorted({w for w in (0, 255, 256, n - 1) if 0 <= w < n}))


def avg_edge_cases():
    """every (n, where): where is None for variant (a)"""
    return [(n, w) for n in AVG_EDGE_N for w in (None,) + avg_edge_wheres(n)]


def avg_edge(n, where=None, seed=None, lone=LONE_FRACTION):
    """n rows over min(40, n // 5) users (at least 5 ratings each where n allows), one item per round, file order shuffled.
    where is None (variant a): every rating is a tenth 0.5 .. 5.0.  Otherwise (variant b) every rating is a half star but
    the one at file row `where`, which is x + lone: the only rating that sets ST_NOT_DYADIC."""
    if seed is None:
        seed = AVG_EDGE_SEEDS[n, where]
    rng = np.random.default_rng([seed, n, 0 if where is None else where + 1])
    n_users = max(1, min(40, n // 5))
    j = rng.permutation(n)
    users = (j % n_users + 1).astype(np.int32)
    items = (j // n_users + 1).astype(np.int32)
    if where is None:
        ratings = rng.integers(5, 51, size=n) / 10.0
    else:
        ratings = rng.integers(1, 11, size=n) / 2.0
        ratings[where] = float(rng.integers(0, 5)) + lone
    return users, items, ratings


# ---- the two limits of the dyadic rule ------------------------------------------------------------------------------------
DYADIC_LIMIT_CASES = ("sixteenths", "thirtyseconds", "at_2_20", "past_2_20")
BIG_USER = 7


def _limit_fit(kind):
    rng = np.random.default_rng(20_260 + DYADIC_LIMIT_CASES.index(kind))
    n_users, n_items, n = 60, 40, 1500
    cells = rng.permutation(n_users * n_items)[:n + 200]
    users = (cells // n_items + 1).astype(np.int32)
    items = (cells % n_items + 1).astype(np.int32)
    if kind == "sixteenths":
        ratings = rng.integers(8, 81, size=len(cells)) / 16.0
    elif kind == "thirtyseconds":
        ratings = rng.integers(16, 161, size=len(cells)) / 32.0
        ratings[0] = 67 / 32.0  # (an odd multiple for certain)
    else:
        # stars 1..4, user BIG_USER's rows times 2^18: its 4-star ratings are 2^20 exactly, the largest magnitude the rule
        # accepts; past_2_20 moves the first of them (a training row) one sixteenth beyond
        ratings = rng.integers(1, 5, size=len(cells)).astype(np.float64)
        big = np.flatnonzero(users[:n] == BIG_USER)
        ratings[big[0]] = 4.0
        ratings[users == BIG_USER] *= 262144.0
        if kind == "past_2_20":
            ratings[big[0]] += 0.0625
    return (users[:n], items[:n], ratings[:n]), (users[n:], items[n:], ratings[n:])


@functools.lru_cache(maxsize=None)
def dyadic_limits():
    """name -> (train, test): four fits of 60 users x 40 items, 1 500 training rows and a 200-row test part, shuffled.
    sixteenths and at_2_20 satisfy k_check_dyadic's rule; thirtyseconds and past_2_20 are one step beyond each limit.  At this
    size the sums of the latter two are still exact in any order (a 1/32 grid below 2^13, a 1/16 grid below 2^26), so they
    check that the ordered paths agree with the oracle like the order-free ones, not that the two differ."""
    return {kind: _limit_fit(kind) for kind in DYADIC_LIMIT_CASES}


def is_dyadic(ratings):
    """k_check_dyadic's rule restated: every rating a multiple of 1/16 with |r| <= 2^20"""
    v = np.asarray(ratings, dtype=np.float64) * 16.0
    return bool(np.all((np.abs(v) <= 16777216.0) & (v == np.rint(v))))


# ---- the ml-100k shape on a wide scale ------------------------------------------------------------------------------------
WIDE_RECO_K = 10
_wide_sets = {}


def wide_user_sets(oracle, per_set=3):
    """user sets of wide100k, searched over the oracle's answers (k = WIDE_RECO_K): `negative` — every fitted user whose mean
    is below zero; `mixed_sign` — the first per_set users (ascending id, non-negative mean) whose FULL kNN recommendation
    list holds predictions of both signs; `tied` — the first per_set such users whose list holds two equal predictions"""
    if not _wide_sets:
        tr, _ = wide100k()
        m = oracle.Model(*tr)
        p = m.pipeline(oracle.SIM_COSINE, WIDE_RECO_K)
        users = np.unique(tr[0])
        n_items = len(np.unique(tr[1]))
        negative = [int(u) for u in users if m.users_avg(int(u)) < 0.0]
        mixed, tied = [], []
        for u in users.tolist():
            if len(mixed) >= per_set and len(tied) >= per_set:
                break
            if u in negative:
                continue
            _, preds = p.recommend(u, n_items)
            if len(mixed) < per_set and (preds < 0.0).any() and (preds > 0.0).any():
                mixed.append(u)
            if len(tied) < per_set and len(np.unique(preds)) < len(preds):
                tied.append(u)
        _wide_sets.update(negative=negative, mixed_sign=mixed, tied=tied)
    return _wide_sets


FOLD_CLONE, FOLD_HEAVY = 7001, 7002
_wide_queries = {}


def wide_query_cases(oracle):
    """queries against the wide100k fit (k = WIDE_RECO_K), built from the data and the oracle's answers:
    fold_clone   (user, items, ratings): a user outside the fit with the rows of the second mixed-sign user (mean > 5);
    fold_heavy   the same user having also rated, at its rounded mean, every item the clone is predicted above zero but 20:
                 its 33 best recommendations then hold predictions below zero;
    lift         (user, items, ratings): the negative-mean fitted user with the fewest rows and three more ratings of 6.3
                 on items it has not rated — the mean over all its rows is above zero;
    stay_negative the same user with one more rating of -2.0;
    revise_keep  (user, removed, items, ratings): the first user (ascending id) with a positive mean over at least five
                 negative and some positive ratings, removing two of its positive ratings — still a positive mean;
    revise_negative the same user removing every positive rating."""
    if not _wide_queries:
        tr, _ = wide100k()
        all_items = np.unique(tr[1])
        sets = wide_user_sets(oracle)
        src = sets["mixed_sign"][1]
        it, rt = tr[1][tr[0] == src], tr[2][tr[0] == src]
        aug = (np.concatenate([tr[0], np.full(len(it), FOLD_CLONE)]).astype(np.int32), np.concatenate([tr[1], it]),
               np.concatenate([tr[2], rt]))
        p = oracle.Model(*aug).pipeline(oracle.SIM_COSINE, WIDE_RECO_K)
        ids, preds = p.recommend(FOLD_CLONE, len(all_items))
        extra = ids[preds > 0.0][20:]
        heavy = (FOLD_HEAVY, np.concatenate([it, extra]).astype(np.int32),
                 np.concatenate([rt, np.full(len(extra), np.round(rt.mean(), 1))]))
        counts = {u: int((tr[0] == u).sum()) for u in sets["negative"]}
        low = min(sets["negative"], key=lambda u: (counts[u], u))
        free = np.setdiff1d(all_items, tr[1][tr[0] == low])[:4].astype(np.int32)
        for q in np.unique(tr[0]).tolist():
            r = tr[2][tr[0] == q]
            if r.mean() > 0.05 and (r < 0.0).sum() >= 5 and (r > 0.0).any() and (r != 0.0).all():
                break
        mine = tr[1][tr[0] == q]
        none_i, none_r = np.empty(0, dtype=np.int32), np.empty(0)
        _wide_queries.update(
            fold_clone=(FOLD_CLONE, it.astype(np.int32), rt.copy()), fold_heavy=heavy,
            lift=(low, free[:3], np.full(3, 6.3)), stay_negative=(low, free[3:], np.array([-2.0])),
            revise_keep=(q, mine[r > 0.0][:2].astype(np.int32), none_i, none_r),
            revise_negative=(q, mine[r > 0.0].astype(np.int32), none_i, none_r))
    return _wide_queries


def _remap(rs):
    a, b = np.asarray(WIDE_A)[rs.users % 3], np.asarray(WIDE_B)[rs.users % 3]
    return rs.users, rs.items, a * rs.ratings + b


@functools.lru_cache(maxsize=None)
def wide100k():
    """(train, test): synth.syn_100k() with every rating remapped per user class (u % 3); the test part ends with one row
    of an unknown user and one of an unknown item, like test_gpu_k_sweep._with_unknowns"""
    synth = importlib.import_module("movie-recommender-system_amd.synth")
    d = synth.syn_100k()
    tr, te = _remap(d.train), _remap(d.test)
    te = (np.concatenate([te[0], [UNKNOWN_USER, tr[0][0]]]).astype(np.int32),
          np.concatenate([te[1], [tr[1][0], UNKNOWN_ITEM]]).astype(np.int32),
          np.concatenate([te[2], [3.0, 4.0]]))
    for a in tr + te:
        a.setflags(write=False)
    return tr, te
