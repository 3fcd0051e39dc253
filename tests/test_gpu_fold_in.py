"""Fold-in kNN queries (knncf_query_neighbors / _predict / _recommend, csrc/foldin.hip): the neighbourhood, predictions and
recommendations of a user that is NOT in the fit, given its ratings, without a refit.  Every answer is compared bit for
bit with the oracle on aug = train ++ the query rows (data.union(personal), recommend/Recommender.scala:68), on a fresh
pipeline whose first call is the query user's neighbourhood.  A single call is a chunk of one of the batched path
(tests/test_gpu_fold_in_batch.py has the larger chunks), on the scratch that the batch calls and recommend_batch use too."""
import importlib
import os

import numpy as np
import pytest

from tests.query_helpers import UNKNOWN_ITEM, _aug, _bits

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "personal.csv")


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _check(kn, oracle, eng, train, q, items, ratings, sim, k, pred_items, ns=(3, None)):
    """the three calls against the oracle on aug; returns the oracle's neighbour list"""
    p = oracle.Model(*_aug(train, q, items, ratings)).pipeline(sim, k)
    oids, osims = p.neighbors(q)  # first evaluation: the query user's
    ids, sims = eng.neighbors_for(q, items, ratings)
    assert len(oids) == min(k, len(np.unique(train[0]))), q
    assert ids.tolist() == oids.tolist(), q
    assert _bits(sims) == _bits(osims), q
    pred_items = np.asarray(pred_items, dtype=np.int32)
    want = [p.predict(q, int(i)) for i in pred_items]
    got = eng.predict_for(q, items, ratings, pred_items)
    assert _bits(got) == _bits(want), q
    n_items = len(np.unique(np.concatenate([train[1], np.asarray(items, dtype=np.int32)])))
    for n in ns:
        n = n_items if n is None else n
        wi, wp = p.recommend(q, n)
        gi, gp = eng.recommend_for(q, items, ratings, n)
        assert gi.tolist() == wi.tolist(), (q, n)
        assert _bits(gp) == _bits(wp), (q, n)
    return oids, osims


def _holdout_users(train):
    u, c = np.unique(train[0], return_counts=True)
    order = np.argsort(c, kind="stable")
    picks = [int(u[order[0]]), int(u[order[-1]])]
    for target in (20, 60, 200):
        picks.append(int(u[np.argmin(np.abs(c - target))]))
    rng = np.random.default_rng(7)
    picks += [int(x) for x in rng.choice(u, 12, replace=False)]
    return list(dict.fromkeys(picks))


def _split(train, q):
    m = train[0] == q
    rest = tuple(a[~m] for a in train)
    return rest, train[1][m], train[2][m]


@pytest.mark.parametrize("k", [300, 10])
def test_holdout_syn100k_cosine(kn, oracle, syn100k, k):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    all_items = np.unique(train[1])
    cases = []
    users = _holdout_users(train)
    for q in users:
        rest, it, rt = _split(train, q)
        cases.append((q, rest, it, rt))
    # short rows (1, 3, 4 and 5 ratings): a prefix of a held-out row
    q0 = users[2]
    rest0, it0, rt0 = _split(train, q0)
    for m in (1, 3, 4, 5):
        cases.append((q0, rest0, it0[:m], rt0[:m]))
    # a held-out user who is the only rater of some items: the query holds items unknown to train
    q1 = users[3]
    rest1, it1, rt1 = _split(train, q1)
    own = set(it1[:3].tolist())
    keep = ~np.isin(rest1[1], list(own))
    cases.append((q1, tuple(a[keep] for a in rest1), it1, rt1))
    e = kn.Engine(k=k)
    for q, rest, it, rt in cases:
        e.fit(*rest)
        preds = np.concatenate([all_items, it, [UNKNOWN_ITEM]])
        _check(kn, oracle, e, rest, q, it, rt, oracle.SIM_COSINE, k, preds)
    e.close()


def test_holdout_syn100k_jaccard(kn, oracle, syn100k):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    all_items = np.unique(train[1])
    e = kn.Engine(k=50, similarity=kn.SIM_JACCARD)
    for q in _holdout_users(train)[:5]:
        rest, it, rt = _split(train, q)
        e.fit(*rest)
        _check(kn, oracle, e, rest, q, it, rt, oracle.SIM_JACCARD, 50, np.concatenate([all_items, it, [UNKNOWN_ITEM]]))
    # a 3-rating Jaccard query with an unknown item
    rest, it, rt = _split(train, _holdout_users(train)[5])
    e.fit(*rest)
    qi = np.array([it[0], UNKNOWN_ITEM, it[1]], dtype=np.int32)
    _check(kn, oracle, e, rest, 5000, qi, rt[:3], oracle.SIM_JACCARD, 50, np.concatenate([all_items, qi]))
    e.close()


def test_personal_csv_against_syn100k(kn, oracle, syn100k):
    """the Recommender's own case: personal.csv's ratings of user 944 as the query"""
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    assert 944 not in set(train[0].tolist())
    _, (pu, pi, pr) = kn.load_personal(GOLDEN, 944)
    e = kn.Engine(k=300)
    e.fit(*train)
    _check(kn, oracle, e, train, 944, pi, pr, oracle.SIM_COSINE, 300, np.concatenate([np.unique(train[1]), pi]))
    e.close()


def test_order_and_value_edge_cases(kn, oracle, syn100k):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    all_items = np.unique(train[1])
    e = kn.Engine(k=30)
    e.fit(*train)
    u, c = np.unique(train[0], return_counts=True)
    long_user = int(u[np.argmax(c)])
    its = train[1][train[0] == long_user][:3]
    rts = np.array([5.0, 1.0, 3.0])
    preds = np.concatenate([all_items, [UNKNOWN_ITEM]])
    # a 3-rating query in two row orders: the <= 4-item set iterates in insertion order
    a = _check(kn, oracle, e, train, 5001, its, rts, oracle.SIM_COSINE, 30, preds)
    b = _check(kn, oracle, e, train, 5001, its[[2, 0, 1]], rts[[2, 0, 1]], oracle.SIM_COSINE, 30, preds)
    assert a[0].tolist() == b[0].tolist()  # (the same users; the sums may round differently)
    # non-dyadic ratings
    its = train[1][train[0] == long_user][:40]
    rts = np.round(np.linspace(0.7, 4.9, len(its)), 1)
    rts[::3] = 3.7
    _check(kn, oracle, e, train, 5002, its, rts, oracle.SIM_COSINE, 30, np.concatenate([preds, its]))
    # every item unknown to train: similarities 0.0, the first k users in order, every prediction the query's mean
    its = np.arange(100_000, 100_007, dtype=np.int32)
    rts = np.array([1.0, 2.0, 3.5, 4.0, 5.0, 2.5, 3.0])
    ids, sims = _check(kn, oracle, e, train, 5003, its, rts, oracle.SIM_COSINE, 30, np.concatenate([preds, its]))
    assert _bits(sims) == _bits(np.zeros(30))
    assert ids.tolist() == list(oracle.Model(*train).user_iteration_order())[:30]
    mean = sum(rts.tolist(), 0.0) / len(rts)
    assert set(e.predict_for(5003, its, rts, all_items).tolist()) == {mean}
    e.close()


def test_ids_outside_the_direct_tables(kn, oracle, synth):
    d = synth.syn_scaled(300, 120, 9_000, seed=5, half_stars=True)
    big = lambda a, off: (a.astype(np.int64) * 7919 + off).astype(np.int32)
    train = (big(d.train.users, -40_000), big(d.train.items, 1 << 25), d.train.ratings)
    q = 1 << 26
    its = np.unique(train[1])[::9][:25]
    rts = np.linspace(1.0, 5.0, len(its))
    e = kn.Engine(k=20)
    e.fit(*train)
    _check(kn, oracle, e, train, q, its, rts, oracle.SIM_COSINE, 20,
           np.concatenate([np.unique(train[1]), [UNKNOWN_ITEM, -5]]))
    _check(kn, oracle, e, train, q, its[:4], rts[:4], oracle.SIM_COSINE, 20, np.unique(train[1]))
    e.close()


def test_status_codes(kn, syn100k):
    import ctypes as C

    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    lib = kn.load_library()
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    its = np.array([1, 2, 3, 50], dtype=np.int32)
    rts = np.array([4.0, 3.0, 5.0, 1.0])
    e = kn.Engine(k=10)
    with pytest.raises(kn.KnncfError) as ex:
        e.neighbors_for(5000, its, rts)
    assert ex.value.status == kn.E_STATE
    e.fit(*train)
    cases = [
        (lambda: e.neighbors_for(int(train[0][0]), its, rts), kn.E_INVALID),  # user in train
        (lambda: e.recommend_for(5000, [1, 2, 1], [4.0, 3.0, 2.0], 3), kn.E_DUPLICATE),
        (lambda: e.predict_for(5000, [1, 2], [6.0, 4.0], [1]), kn.E_NONFINITE),  # mean 5, 6 > 5: scale 0
        (lambda: e.neighbors_for(5000, np.arange(1, 65_539, dtype=np.int32), np.full(65_538, 3.0)), kn.E_UNSUPPORTED),
    ]
    for call, status in cases:
        with pytest.raises(kn.KnncfError) as ex:
            call()
        assert ex.value.status == status
        # the single call's own text, not the batch's "query batch: query 0: ..."
        text = lib.knncf_last_error(e._h).decode()
        assert text.startswith("query:") and "query batch" not in text, text
    out = np.empty(4, dtype=np.float64)
    c = C.c_int32()
    ptr = lambda a, t: a.ctypes.data_as(t)
    # null pointers and n_ratings <= 0 at the C boundary
    assert lib.knncf_query_predict(e._h, kn.PRED_KNN, 5000, None, ptr(rts, f64p), 4, ptr(its, i32p), 4, ptr(out, f64p)) == kn.E_INVALID
    assert lib.knncf_query_predict(e._h, kn.PRED_KNN, 5000, ptr(its, i32p), ptr(rts, f64p), 0, ptr(its, i32p), 4, ptr(out, f64p)) == kn.E_INVALID
    assert lib.knncf_query_neighbors(e._h, 5000, ptr(its, i32p), ptr(rts, f64p), 4, 4, None, None, C.byref(c)) == kn.E_INVALID
    # another predictor
    ids = np.empty(4, dtype=np.int32)
    assert lib.knncf_query_recommend(e._h, kn.PRED_BASELINE, 5000, ptr(its, i32p), ptr(rts, f64p), 4, 4, ptr(ids, i32p),
                                     ptr(out, f64p), C.byref(c)) == kn.E_UNSUPPORTED
    # several refusals at once: the predictor is checked before the user, the null pointer before the predictor
    assert lib.knncf_query_recommend(e._h, kn.PRED_BASELINE, int(train[0][0]), ptr(its, i32p), ptr(rts, f64p), 4, 4, ptr(ids, i32p),
                                     ptr(out, f64p), C.byref(c)) == kn.E_UNSUPPORTED
    assert lib.knncf_query_recommend(e._h, kn.PRED_BASELINE, 5000, None, ptr(rts, f64p), 4, 4, ptr(ids, i32p),
                                     ptr(out, f64p), C.byref(c)) == kn.E_INVALID
    e.close()
    # similarityOne, sharded handles are refused; fewer than 5 train users
    e1 = kn.Engine(k=10, similarity=kn.SIM_ONE)
    e1.fit(*train)
    with pytest.raises(kn.KnncfError) as ex:
        e1.neighbors_for(5000, its, rts)
    assert ex.value.status == kn.E_UNSUPPORTED
    e1.close()
    m = np.isin(train[0], np.unique(train[0])[:4])
    e4 = kn.Engine(k=10)
    e4.fit(*(a[m] for a in train))
    with pytest.raises(kn.KnncfError) as ex:
        e4.recommend_for(5000, its, rts, 3)
    assert ex.value.status == kn.E_UNSUPPORTED
    e4.close()


def test_counts_at_the_edges(kn, syn100k):
    """n = 0 and an empty pred_items still run the query's prep and report its status; *count of the neighbours is
    min(k, U) whatever cap is"""
    import ctypes as C

    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    lib = kn.load_library()
    e = kn.Engine(k=40)
    e.fit(*train)
    its = np.array([1, 2, 3, 50], dtype=np.int32)
    rts = np.array([4.0, 3.0, 5.0, 1.0])
    gi, gp = e.recommend_for(5000, its, rts, 0)
    assert len(gi) == 0 and len(gp) == 0
    assert len(e.predict_for(5000, its, rts, np.empty(0, dtype=np.int32))) == 0
    for call in (lambda: e.recommend_for(5000, [1, 2, 1], [4.0, 3.0, 2.0], 0),
                 lambda: e.predict_for(5000, [1, 2, 1], [4.0, 3.0, 2.0], np.empty(0, dtype=np.int32))):
        with pytest.raises(kn.KnncfError) as ex:
            call()
        assert ex.value.status == kn.E_DUPLICATE
    # recommend's *count at the C boundary: 0 for n = 0 (set from a sentinel)
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ptr = lambda a, t: a.ctypes.data_as(t)
    c = C.c_int32(-7)
    assert lib.knncf_query_recommend(e._h, kn.PRED_KNN, 5000, ptr(its, i32p), ptr(rts, f64p), 4, 0, None, None, C.byref(c)) == kn.OK
    assert c.value == 0
    c = C.c_int32(-7)
    assert lib.knncf_query_neighbors(e._h, 5000, ptr(its, i32p), ptr(rts, f64p), 4, 0, None, None, C.byref(c)) == kn.OK
    assert c.value == min(40, e.num_users) == 40
    e.close()


def test_single_calls_on_the_shared_scratch(kn, oracle, syn100k):
    """The single calls, the batch calls and recommend_batch (n > 32: the segmented full order on lent buffers) use one
    scratch set of the handle.  After a 40-query chunk (k_query_sim_dual) and a recommend_batch have sized and filled it,
    the single calls still answer as the oracle does, and they leave nothing behind that changes recommend_batch."""
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    all_items = np.unique(train[1])
    rng = np.random.default_rng(29)
    queries = []
    for j in range(40):
        m = int(rng.integers(1, 120))
        its = rng.choice(np.arange(1, 1700, dtype=np.int32), m, replace=False)
        queries.append((10_000 + j, its, rng.integers(1, 6, m).astype(np.float64)))
    fitted = np.unique(train[0])[[3, 77, 400, 650, 900]]
    long_row = train[0] == int(fitted[2])
    singles = [(5001, train[1][long_row][:3], np.array([5.0, 1.0, 3.0])),
               (5002, all_items[::20][:70], np.round(np.linspace(0.7, 4.9, 70), 1))]
    assert len(singles[1][1]) >= 60

    def same(a, b):
        return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))

    e = kn.Engine(k=40)
    e.fit(*train)
    _, st = e.recommend_for_batch(queries, 3)
    assert st.tolist() == [kn.OK] * len(queries)
    before = e.recommend_batch(kn.PRED_KNN, fitted, 40)
    for q, it, rt in singles:
        _check(kn, oracle, e, train, q, it, rt, oracle.SIM_COSINE, 40, np.concatenate([all_items, it, [UNKNOWN_ITEM]]))
    after = e.recommend_batch(kn.PRED_KNN, fitted, 40)
    e.close()
    fresh = kn.Engine(k=40)
    fresh.fit(*train)
    alone = fresh.recommend_batch(kn.PRED_KNN, fitted, 40)
    fresh.close()
    assert same(before, after) and same(before, alone)


def test_queries_leave_the_handle_untouched(kn, syn100k, tmp_path):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    test = (d.test.users, d.test.items, d.test.ratings)
    users = np.unique(train[0])
    rng = np.random.default_rng(3)
    queries = []
    for j in range(50):
        m = int(rng.integers(1, 120))
        its = rng.choice(np.arange(1, 1700, dtype=np.int32), m, replace=False)
        queries.append((10_000 + j, its, rng.integers(1, 6, m).astype(np.float64)))

    def session(path, with_queries):
        e = kn.Engine(k=40)
        e.fit(*train)
        first = (e.mae(kn.PRED_KNN, *test), [e.neighbors(int(u)) for u in users[[4, 80, 500]]])
        answers = []
        if with_queries:
            for rep in range(2):
                got = []
                for j, (q, its, rts) in enumerate(queries):
                    call = (e.neighbors_for, e.predict_for, e.recommend_for)[j % 3]
                    arg = {0: (), 1: (np.arange(1, 1700),), 2: (10,)}[j % 3]
                    got.append(call(q, its, rts, *arg))
                answers.append(got)
        e.neighbors_save(str(path))
        second = (e.mae(kn.PRED_KNN, *test), [e.neighbors(int(u)) for u in users[[4, 80, 500, 900]]])
        e.close()
        return first, second, answers

    fa, sa, answers = session(tmp_path / "a.bin", True)
    fb, sb, _ = session(tmp_path / "b.bin", False)
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes()
    for x, y in ((fa, fb), (sa, sb)):
        assert _bits([x[0]]) == _bits([y[0]])
        for (i1, s1), (i2, s2) in zip(x[1], y[1]):
            assert i1.tolist() == i2.tolist() and _bits(s1) == _bits(s2)
    # the repeated queries answer the same
    for g1, g2 in zip(*answers):
        if isinstance(g1, tuple):
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(g1, g2))
        else:
            assert _bits(g1) == _bits(g2)


def test_ml25m_shape_holdouts(kn, oracle, synth):
    """syn-25m: one fit of train minus three held-out users (short, median and longest row), then the three queries,
    each against its own oracle fit of aug"""
    d = synth.syn_25m()
    train = (d.train.users, d.train.items, d.train.ratings)
    u, c = np.unique(train[0], return_counts=True)
    order = np.argsort(c, kind="stable")
    qs = [int(u[order[0]]), int(u[order[len(order) // 2]]), int(u[order[-1]])]
    held = np.isin(train[0], qs)
    rest = tuple(a[~held] for a in train)
    e = kn.Engine(k=300)
    e.fit(*rest)
    some_items = np.unique(rest[1])[::50]
    for q in qs:
        m = train[0] == q
        it, rt = train[1][m], train[2][m]
        _check(kn, oracle, e, rest, q, it, rt, oracle.SIM_COSINE, 300, np.concatenate([some_items, it[:50], [UNKNOWN_ITEM]]),
               ns=(3, 500))
    e.close()
