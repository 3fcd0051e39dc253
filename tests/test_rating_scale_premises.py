"""The cases of tests/rating_scales.py sit where they claim (CPU: the oracle, the literal model and numpy alone), and the
oracle that tests/test_gpu_rating_scales.py compares with is itself right off the star scale: it equals the literal Scala
model (tests/scala_model.py) bit for bit on every rating domain."""
import numpy as np
import pytest

from tests import rating_scales as rs
from tests import scala_model as sm

SEEDS = range(4)
SMALL = [(d, s) for d in rs.DOMAINS for s in SEEDS]


def _small(domain, seed):
    rng = np.random.default_rng([1234, rs.DOMAINS.index(domain), seed])
    rows = rs.small_case(rng, domain, tiny_rows=seed % 3)
    return rs.split_small(rows)


def _zero_scale(train):
    m = sm.users_avg(train)
    return any(sm.scale(r, m[u]) == 0 for (u, _, r) in train)


def _lists(rows):
    return tuple(a.tolist() for a in rs.cols(rows))


def _fold(x):
    acc = 0.0
    for v in np.asarray(x, dtype=np.float64).tolist():
        acc = acc + v
    return acc


def _exact_sum_order(x):
    """k_exact_sum's order for n <= 262 144: a 256-wide tree per block, the block sums added in ascending order (one of the
    orders its atomics may take)"""
    x = np.asarray(x, dtype=np.float64)
    out = 0.0
    for b in range(0, len(x), 256):
        red = np.zeros(256)
        red[:min(256, len(x) - b)] = x[b:b + 256]
        o = 128
        while o > 0:
            red[:o] = red[:o] + red[o:2 * o]
            o >>= 1
        out = out + float(red[0])
    return out


def _bits(v):
    return np.float64(v).view(np.int64)


# ---- the oracle against the literal model -----------------------------------------------------------------------------------
def test_at_most_two_small_cases_hit_a_zero_scale():
    assert sum(_zero_scale(_small(d, s)[0]) for d, s in SMALL) <= 2


@pytest.mark.parametrize("domain,seed", SMALL)
def test_oracle_equals_literal_model_off_the_star_scale(oracle, domain, seed):
    """the quantity list of test_oracle_semantics.test_oracle_equals_literal_model_bitwise plus recommendations, with a fresh
    adjusted-cosine memo for the neighbour queries (a memo that a MAE run filled holds pairs summed from the other side)"""
    train, test = _small(domain, seed)
    if _zero_scale(train):
        pytest.skip("scale() == 0 corner")
    m = oracle.Model(*_lists(train))
    tu, ti, tr = _lists(test)

    assert m.average() == sm.average(train)
    ua, ia = sm.users_avg(train), sm.items_avg(train)
    assert all(m.users_avg(u) == v for u, v in ua.items())
    assert all(m.items_avg(i) == v for i, v in ia.items())
    negative = sorted(u for u, v in ua.items() if v < 0.0)
    assert (len(negative) >= 3) if domain == "neg_users" else True
    nd = sm.compute_normalize_deviation(train)
    assert m.normalized_deviations().tolist() == [nd.d[(u, i)] for (u, i, _) in train]
    pre = sm.preprocessed_rating(train)
    assert m.preprocessed().tolist() == [pre[(u, i)] for (u, i, _) in train]
    dev = sm.items_avg_dev(train)
    assert all(m.items_avg_dev(i) == v for i, v in dev.items())

    g = sm.average(train)
    base = sm.compute_prediction(train)
    assert m.mae(oracle.KIND_BASELINE, tu, ti, tr) == sm.mae(base, test)
    assert m.mae(oracle.KIND_GLOBAL, tu, ti, tr) == sm.mae(lambda u, i: g, test)
    assert m.mae(oracle.KIND_USER, tu, ti, tr) == sm.mae(lambda u, i: ua.get(u, g), test)
    assert m.mae(oracle.KIND_ITEM, tu, ti, tr) == sm.mae(lambda u, i: ia.get(i, g), test)

    users = sorted(ua)
    for k in (1, 3, 40):
        cos = sm.adjusted_cosine_similarity_function(train)
        want = sm.mae(sm.predictor(train, sm.weighted_sum_deviation(train, sm.get_similarity(train, k, cos))), test)
        got, preds = m.pipeline(oracle.SIM_COSINE, k).mae(tu, ti, tr, True)
        assert got == want
        if negative:  # a fitted user with a negative mean is answered with the global average :572-573
            rows = [j for j, u in enumerate(tu) if u in negative]
            assert all(preds[j] == g for j in rows)
        nn = sm.get_neighbors(train, k, sm.adjusted_cosine_similarity_function(train))  # fresh memo
        p2 = m.pipeline(oracle.SIM_COSINE, k)
        for u in users[::2] + users[1::2]:
            ids, sims = p2.neighbors(u)
            ref = nn(u)
            assert ids.tolist() == [x for x, _ in ref]
            assert sims.tolist() == [s for _, s in ref]

    want = sm.mae(sm.predictor(train, sm.weighted_sum_deviation(train, sm.jaccard_coefficient(train))), test)
    assert m.pipeline(oracle.SIM_JACCARD, -1).mae(tu, ti, tr) == want

    # recommendations :651-674, kNN and baseline: a negative-mean user where the domain has one, and an ordinary user
    ordinary = next(u for u in users if ua[u] >= 0.0)
    k = 3
    cos = sm.adjusted_cosine_similarity_function(train)
    knn = sm.recommendations(train, sm.predictor(train, sm.weighted_sum_deviation(train, sm.get_similarity(train, k, cos))))
    basr = sm.recommendations(train, base)
    p = m.pipeline(oracle.SIM_COSINE, k)
    for u in negative[:1] + [ordinary]:
        for n in (3, 100):
            ids, preds = p.recommend(u, n)
            assert (ids.tolist(), preds.tolist()) == ([x for x, _ in knn(u, n)], [v for _, v in knn(u, n)])
            ids, preds = m.recommend(oracle.KIND_BASELINE, u, n)
            assert (ids.tolist(), preds.tolist()) == ([x for x, _ in basr(u, n)], [v for _, v in basr(u, n)])
            if u in negative:
                assert set(preds.tolist()) == {g} and ids.tolist() == sorted(ids.tolist())


def test_history_case_tells_the_two_build_histories_apart(oracle):
    """the reference's history (no neighbourhood for a negative-mean user's test rows) against the one that builds every
    fitted user's list at its first test row whose item has raters: the same predictions, different neighbour lists"""
    train, test = rs.history_case()
    tr, te = rs.cols(train), rs.cols(test)
    m = oracle.Model(*tr)
    users = np.unique(tr[0]).tolist()
    negative = [u for u in users if m.users_avg(u) < 0.0]
    assert negative and set(negative) & set(te[0].tolist())
    assert np.bincount(np.unique(tr[0], return_inverse=True)[1]).min() <= 4
    known_items = set(tr[1].tolist())
    differing = 0
    for k in (1, 4, len(users) + 3):
        right, wrong = m.pipeline(oracle.SIM_COSINE, k), m.pipeline(oracle.SIM_COSINE, k)
        _, preds = right.mae(*te, True)
        other = []
        for u, i in zip(te[0].tolist(), te[1].tolist()):
            if u in users and i in known_items:
                wrong.neighbors(u)
            other.append(wrong.predict(u, i))
        assert np.array_equal(preds.view(np.int64), np.asarray(other).view(np.int64))
        # the literal model agrees with the oracle's history
        cos = sm.adjusted_cosine_similarity_function(train)
        nn = sm.get_neighbors(train, k, cos)
        lit = sm.predictor(train, sm.weighted_sum_deviation(train, lambda a, b: sm.ssum([s if x == b else 0.0 for x, s in nn(a)])))
        assert sm.mae(lit, test) == right.mae(*te)
        for u in users:
            a, b, ref = right.neighbors(u), wrong.neighbors(u), nn(u)
            assert a[0].tolist() == [x for x, _ in ref] and a[1].tolist() == [s for _, s in ref]
            differing += a[0].tolist() != b[0].tolist() or a[1].view(np.int64).tolist() != b[1].view(np.int64).tolist()
    assert differing >= 2


def test_history_case_tells_a_recommendation_from_a_neighbour_query(oracle):
    """recommend(u, n) for a negative-mean user is answered at :573 and builds no neighbourhood; neighbors(u) builds one, and
    the lists queried afterwards then differ in their bits.  tests/test_gpu_recommend_batch.py's history test relies on user
    17 showing this at k = 5"""
    train, _ = rs.history_case()
    tr = rs.cols(train)
    m = oracle.Model(*tr)
    users = np.unique(tr[0]).tolist()
    assert len(users) == 18 and len(np.unique(tr[1])) == 15
    assert [u for u in users if m.users_avg(u) < 0.0] == [10, 17, 24]

    def lists(first):
        p = m.pipeline(oracle.SIM_COSINE, 5)
        first(p)
        return [(ids.tolist(), sims.view(np.int64).tolist()) for ids, sims in (p.neighbors(u) for u in users)]

    untouched = lists(lambda p: None)
    assert lists(lambda p: p.recommend(17, 3)) == untouched
    built = lists(lambda p: p.neighbors(17))
    assert sum(a != b for a, b in zip(built, untouched)) >= 1


# ---- wide100k ---------------------------------------------------------------------------------------------------------------
def test_wide100k_is_off_the_scale_where_it_claims(oracle):
    tr, te = rs.wide100k()
    m = oracle.Model(*tr)
    users, counts = np.unique(tr[0], return_counts=True)
    means = np.array([m.users_avg(int(u)) for u in users])
    assert len(users) == 943 and counts.min() == 17 > 4
    assert int((means < 0.0).sum()) == 68 and int((means > 5.0).sum()) == 213
    assert int(((means >= 0.0) & (means < 1.0)).sum()) == 153
    dev = m.normalized_deviations()  # (orc_fit refuses a zero scale(); every deviation is finite and many leave [-1, 1])
    assert np.isfinite(dev).all() and (np.abs(dev) > 1.0).mean() > 0.2 and np.abs(dev).max() > 1000.0
    # the average is an order-sensitive left fold here
    n = len(tr[2])
    assert m.average() == _fold(tr[2]) / n
    assert m.average() != float(np.sum(tr[2])) / n and m.average() != _fold(tr[2][::-1]) / n
    order_dependent = 0
    for u in users:
        rows = np.flatnonzero(tr[0] == u)
        by_item_desc = rows[np.argsort(-tr[1][rows], kind="stable")]
        assert m.users_avg(int(u)) == _fold(tr[2][rows]) / len(rows)
        order_dependent += _fold(tr[2][rows]) != _fold(tr[2][by_item_desc])
    assert order_dependent >= 500
    # predictions of both signs, far outside [1, 5]
    for k, negative_rows in ((10, 1627), (300, 4743)):
        _, preds = m.pipeline(oracle.SIM_COSINE, k).mae(*te, True)
        assert np.isfinite(preds).all() and int((preds < 0.0).sum()) == negative_rows
    sets = rs.wide_user_sets(oracle)
    assert len(sets["negative"]) == 68
    assert len(sets["mixed_sign"]) >= 1 and len(sets["tied"]) >= 1
    assert not set(sets["negative"]) & (set(sets["mixed_sign"]) | set(sets["tied"]))
    neg_rows = np.isin(te[0], sets["negative"])
    assert int(neg_rows.sum()) >= 100


def test_wide100k_queries_cross_the_zero_mean_where_they_claim(oracle):
    from tests import revise_cases as rc
    from tests.query_helpers import _aug

    tr, _ = rs.wide100k()
    q = rs.wide_query_cases(oracle)
    m = oracle.Model(*tr)
    fitted = set(np.unique(tr[0]).tolist())
    n_items = len(np.unique(tr[1]))
    for name in ("fold_clone", "fold_heavy"):
        user, items, ratings = q[name]
        assert user not in fitted and len(items) <= 65536 and len(set(items.tolist())) == len(items)
        p = oracle.Model(*_aug(tr, user, items, ratings)).pipeline(oracle.SIM_COSINE, rs.WIDE_RECO_K)
        assert p.model.users_avg(user) > 0.0
        _, full = p.recommend(user, n_items)
        _, best = p.recommend(user, 33)
        assert (full < 0.0).any() and (full > 0.0).any()
        assert len(best) == 33 and (bool((best < 0.0).any()) == (name == "fold_heavy"))
    user, items, ratings = q["lift"]
    assert m.users_avg(user) < 0.0 and oracle.Model(*_aug(tr, user, items, ratings)).users_avg(user) > 0.0
    user2, items, ratings = q["stay_negative"]
    assert user2 == user and oracle.Model(*_aug(tr, user, items, ratings)).users_avg(user) < 0.0
    user, removed, items, ratings = q["revise_keep"]
    assert m.users_avg(user) > 0.0 and len(removed) == 2
    assert oracle.Model(*rc.aug_of(tr, user, removed, items, ratings)).users_avg(user) > 0.0
    user2, removed, items, ratings = q["revise_negative"]
    aug = rc.aug_of(tr, user2, removed, items, ratings)
    assert user2 == user and (aug[0] == user).sum() >= 5 and oracle.Model(*aug).users_avg(user) < 0.0


# ---- avg_edge ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,where", rs.avg_edge_cases())
def test_avg_edge_left_fold_differs_from_another_order(n, where):
    users, items, r = rs.avg_edge(n, where)
    assert len(r) == n and len(set(zip(users.tolist(), items.tolist()))) == n
    assert not rs.is_dyadic(r) or (n == 1 and where is None)
    if where is not None:  # the lone flag-setter
        off = np.flatnonzero(r * 2.0 != np.rint(r * 2.0))
        assert off.tolist() == [where]
        assert rs.is_dyadic(np.delete(r, where))
    if n >= 5:
        assert np.bincount(users)[1:].min() >= 5
    left = _bits(_fold(r))
    if n == 1:
        return  # one addend has one order: the case is the <= 4-row class of prep_fit alone
    if where == n - 1:  # the lone rating is added last: one rounding in the left fold and in k_exact_sum's order alike
        assert left != _bits(_fold(r[::-1])) or left != _bits(float(np.sum(r)))
    else:
        assert left != _bits(_exact_sum_order(r))
        if where is not None:  # a tenth in the lone rating's place would leave nothing to see
            _, _, tenth = rs.avg_edge(n, where, lone=0.1)
            assert _bits(_fold(tenth)) == _bits(_exact_sum_order(tenth))


# ---- dyadic_limits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", rs.DYADIC_LIMIT_CASES)
def test_dyadic_limit_cases_sit_on_the_rule(kind):
    """sixteenths and at_2_20 are dyadic by k_check_dyadic's rule, and their sums are exact in any order: the order-free
    k_exact_sum and the canonical-order fold are legitimate.  thirtyseconds and past_2_20 are one step beyond each limit and
    take the sequential paths; at 1 500 rows their sums are still exact in any order (a 1/32 grid below 2^13, a 1/16 grid
    below 2^26), so these two cases check that both paths agree with the oracle, not that they differ from each other."""
    tr, te = rs.dyadic_limits()[kind]
    assert len(tr[2]) == 1500 and len(te[2]) == 200
    assert len(set(zip(tr[0].tolist(), tr[1].tolist()))) == 1500
    assert np.bincount(tr[0])[1:].min() > 4
    assert rs.is_dyadic(tr[2]) == (kind in ("sixteenths", "at_2_20"))
    if kind == "at_2_20":
        assert np.abs(tr[2]).max() == rs.DYADIC_LIMIT
    if kind == "past_2_20":
        assert np.abs(tr[2]).max() == rs.DYADIC_LIMIT + 0.0625
        assert rs.is_dyadic(np.delete(tr[2], np.argmax(tr[2])))
    if kind == "thirtyseconds":
        assert (tr[2] * 16.0 != np.rint(tr[2] * 16.0)).any() and np.abs(tr[2]).max() <= 5.0
    shuffled = np.random.default_rng(5).permutation(1500)
    assert _bits(_fold(tr[2])) == _bits(_fold(tr[2][shuffled])) == _bits(_exact_sum_order(tr[2]))
    for u in np.unique(tr[0]):
        rows = np.flatnonzero(tr[0] == u)
        assert _bits(_fold(tr[2][rows])) == _bits(_fold(tr[2][rows[::-1]])), int(u)
