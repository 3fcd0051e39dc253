"""Update queries (knncf_update_neighbors / _predict / _recommend and their batched forms, csrc/foldin.hip): the answers for
a user that may be IN the fit and has rated a few more items since, without a refit.  Every answer is compared bit for bit
with the oracle on aug = train ++ the additional rows (data.union(personal), recommend/Recommender.scala:68), on a fresh
pipeline whose first call is the user's neighbourhood.  To hold rows of a fitted user out, the user's last m file rows are
moved out of train and given back as the additional rows: aug is then a permutation of the data."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from tests.query_helpers import MAX_CHUNK, UNKNOWN_ITEM, _aug, _bits, _chunk, _same_pair, _workspace_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _hold_out(full, users, m):
    """train = full minus the last m file rows of every user of `users` (m: one number or one per user); rows[u] = (items,
    ratings) of those rows in file order"""
    ms = dict(zip(users, m)) if not isinstance(m, int) else {u: m for u in users}
    out = np.zeros(len(full[0]), dtype=bool)
    rows = {}
    for u in users:
        idx = np.flatnonzero(full[0] == u)[-ms[u]:] if ms[u] else np.empty(0, dtype=np.int64)
        out[idx] = True
        rows[u] = (full[1][idx], full[2][idx])
    return tuple(a[~out] for a in full), rows


def _pred_items(train, q, items):
    """every train item, the additional items, the user's train items, one unknown item"""
    return np.concatenate([np.unique(train[1]), items, train[1][train[0] == q], [UNKNOWN_ITEM]]).astype(np.int32)


def _oracle_answers(oracle, train, q, items, ratings, sim, k, pred_items, ns):
    p = oracle.Model(*_aug(train, q, items, ratings)).pipeline(sim, k)
    nb = p.neighbors(q)  # first evaluation: the user's
    known = int(q in set(train[0].tolist()))
    assert len(nb[0]) == min(k, len(np.unique(train[0])) - known), q  # (allUsers - u) :608
    pr = [p.predict(q, int(i)) for i in pred_items]
    return nb, pr, [p.recommend(q, n) for n in ns]


def _check(kn, oracle, eng, train, q, items, ratings, sim, k, ns=(3, None)):
    """the three single calls against the oracle on aug; returns the neighbour list"""
    pred_items = _pred_items(train, q, items)
    n_items = len(np.unique(np.concatenate([train[1], np.asarray(items, dtype=np.int32)])))
    ns = [n_items if n is None else n for n in ns]
    (oids, osims), want, recos = _oracle_answers(oracle, train, q, items, ratings, sim, k, pred_items, ns)
    ids, sims = eng.neighbors_with(q, items, ratings)
    assert q not in ids.tolist(), q  # s(u, u) would head the list
    assert ids.tolist() == oids.tolist(), q
    assert _bits(sims) == _bits(osims), q
    assert _bits(eng.predict_with(q, items, ratings, pred_items)) == _bits(want), q
    for n, (wi, wp) in zip(ns, recos):
        gi, gp = eng.recommend_with(q, items, ratings, n)
        assert gi.tolist() == wi.tolist(), (q, n)
        assert _bits(gp) == _bits(wp), (q, n)
    return ids, sims


def _pick_users(train):
    """the shortest and the longest row, rows near 20 / 60 / 200 ratings, random ones: about a dozen"""
    u, c = np.unique(train[0], return_counts=True)
    order = np.argsort(c, kind="stable")
    picks = [int(u[order[0]]), int(u[order[-1]])]
    for target in (20, 60, 200):
        picks.append(int(u[np.argmin(np.abs(c - target))]))
    rng = np.random.default_rng(7)
    picks += [int(x) for x in rng.choice(u, 8, replace=False)]
    return list(dict.fromkeys(picks))


def _syn100k(d, shuffled=False):
    full = (d.train.users, d.train.items, d.train.ratings)
    if shuffled:  # file order is no longer the users' item order: the seeded rows must come in FILE order
        order = np.random.default_rng(41).permutation(len(full[0]))
        full = tuple(a[order] for a in full)
    return full


@pytest.mark.parametrize("m", [1, 3, 10])
@pytest.mark.parametrize("k", [300, 10])
def test_fitted_users_syn100k_cosine(kn, oracle, syn100k, k, m):
    full = _syn100k(syn100k)
    users = _pick_users(full)
    train, rows = _hold_out(full, users, m)
    e = kn.Engine(k=k)
    e.fit(*train)
    for q in users:
        _check(kn, oracle, e, train, q, *rows[q], oracle.SIM_COSINE, k)
    e.close()


def test_file_order_and_non_dyadic_ratings(kn, oracle, syn100k):
    """shuffled file rows and ratings whose sums round: the mean folds the train rows in file order, then the additional ones"""
    u, i, r = _syn100k(syn100k, shuffled=True)
    r = np.round(r * 0.93 + 0.1, 2)
    full = (u, i, r)
    users = _pick_users(full)[:6]
    train, rows = _hold_out(full, users, 3)
    e = kn.Engine(k=40)
    e.fit(*train)
    for q in users:
        _check(kn, oracle, e, train, q, *rows[q], oracle.SIM_COSINE, 40)
    e.close()


def test_fitted_users_syn100k_jaccard(kn, oracle, syn100k):
    full = _syn100k(syn100k)
    users = _pick_users(full)[:5]
    train, rows = _hold_out(full, users, 3)
    e = kn.Engine(k=50, similarity=kn.SIM_JACCARD)
    e.fit(*train)
    for q in users:
        _check(kn, oracle, e, train, q, *rows[q], oracle.SIM_JACCARD, 50)
    # additional rows with an item unknown to train
    q = users[2]
    it, rt = rows[q]
    _check(kn, oracle, e, train, q, np.array([it[0], UNKNOWN_ITEM, it[1]], dtype=np.int32), rt, oracle.SIM_JACCARD, 50)
    e.close()


def _small_set(seed=3):
    """40 users x 30 items in shuffled file order, non-dyadic ratings; users 1..6 have 1..4 ratings, user 7 has 3, user 8
    has 5, user 9 has 4, the others 5..20"""
    rng = np.random.default_rng(seed)
    sizes = {1: 1, 2: 2, 3: 3, 4: 4, 5: 4, 6: 2, 7: 3, 8: 5, 9: 4}
    us, its = [], []
    for u in range(1, 41):
        n = sizes.get(u, int(rng.integers(5, 21)))
        its.append(rng.choice(np.arange(1, 31, dtype=np.int32), n, replace=False))
        us.append(np.full(n, u, dtype=np.int32))
    us, its = np.concatenate(us), np.concatenate(its)
    rts = np.round(rng.uniform(0.5, 5.0, len(us)), 1)
    order = rng.permutation(len(us))
    return us[order], its[order].astype(np.int32), rts[order]


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_row_size_classes(kn, oracle, sim_name):
    """the <= 4 regime (given-order folding) is decided by the COMBINED row count"""
    osim, esim = {"cosine": (oracle.SIM_COSINE, kn.SIM_COSINE), "jaccard": (oracle.SIM_JACCARD, kn.SIM_JACCARD)}[sim_name]
    full = _small_set()
    # user 7: 2 train + 1 additional; user 8: 2 train + 3 additional (crosses to > 4); user 9: 4 train + 0 additional;
    # user 3: 1 train + 2 additional; user 20: a long row + 2; the neighbours include users of <= 4 ratings
    users, ms = [7, 8, 9, 3, 20], [1, 3, 0, 2, 2]
    train, rows = _hold_out(full, users, ms)
    for q, m in zip(users, ms):
        assert len(rows[q][0]) == m
    assert [int((train[0] == q).sum()) for q in users[:4]] == [2, 2, 4, 1]
    for k in (10, 64):  # k >= U: every other user is a neighbour
        e = kn.Engine(k=k, similarity=esim)
        e.fit(*train)
        for q in users:
            ids, _ = _check(kn, oracle, e, train, q, *rows[q], osim, k)
            if k == 10:
                continue
            assert len(ids) == 39
        if k == 10:
            # an extra row for user 7 in two given orders, beside its 2 train rows: <= 4 combined, file order decides
            free = np.setdiff1d(np.arange(1, 31), full[1][full[0] == 7])[:2].astype(np.int32)
            rt = np.array([4.3, 1.7])
            tr7, _ = _hold_out(full, [7], 1)
            e.fit(*tr7)
            _check(kn, oracle, e, tr7, 7, free, rt, osim, k)
            _check(kn, oracle, e, tr7, 7, free[::-1], rt[::-1], osim, k)
        e.close()


def test_empty_additional_rows(kn, oracle, syn100k, tmp_path):
    """neighbors_with(u, [], []) is the fresh-closure answer on train itself, and it leaves the handle as it was"""
    train = _syn100k(syn100k)
    users = _pick_users(train)[:4]
    e = kn.Engine(k=40)
    e.fit(*train)
    e.neighbors(int(train[0][-1]))  # something in the table
    e.neighbors_save(str(tmp_path / "before.bin"))
    none_i, none_r = np.empty(0, dtype=np.int32), np.empty(0)
    for q in users:
        ids, sims = _check(kn, oracle, e, train, q, none_i, none_r, oracle.SIM_COSINE, 40)
        fresh = kn.Engine(k=40)
        fresh.fit(*train)
        _same_pair((ids, sims), fresh.neighbors(q), q)  # the first evaluation of a freshly fitted engine
        fresh.close()
    # null pointers with n_ratings == 0 at the C boundary
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    got = np.full(40, -77, dtype=np.int32)
    vals = np.full(40, -77.5)
    c = C.c_int32(-7)
    assert e._lib.knncf_update_neighbors(e._h, users[0], None, None, 0, 40, got.ctypes.data_as(i32p), vals.ctypes.data_as(f64p),
                                         C.byref(c)) == kn.OK
    assert c.value == 40
    _same_pair((got, vals), e.neighbors_with(users[0], [], []), "null rows")
    e.neighbors_save(str(tmp_path / "after.bin"))
    assert (tmp_path / "before.bin").read_bytes() == (tmp_path / "after.bin").read_bytes()
    # the user's own stored list is neither read nor replaced
    stored = e.neighbors(users[1])
    it = np.array([UNKNOWN_ITEM, UNKNOWN_ITEM + 1], dtype=np.int32)
    e.recommend_with(users[1], it, [1.0, 5.0], 5)
    _same_pair(stored, e.neighbors(users[1]), "stored list")
    e.close()


def test_k_beyond_the_user_count(kn, oracle):
    """k >= U: U - 1 neighbours for a user of the fit, U for another in the same batch; cells beyond the count untouched"""
    full = _small_set(seed=5)
    train, rows = _hold_out(full, [12], 2)
    U = 40
    e = kn.Engine(k=64)
    e.fit(*train)
    queries = [(12,) + rows[12], (500, np.array([3, 9, 17], dtype=np.int32), np.array([4.5, 2.0, 3.1])),
               (13, np.empty(0, dtype=np.int32), np.empty(0))]
    us, off, it, rt = e._query_batch(queries)
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    ids = np.full((3, 64), -77, dtype=np.int32)
    vals = np.full((3, 64), -77.5)
    cnt = np.full(3, -1, dtype=np.int32)
    st = np.full(3, 99, dtype=np.int32)
    assert e._lib.knncf_update_neighbors_batch(e._h, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), 3, 64,
                                               p(ids.reshape(-1), i32p), p(vals.reshape(-1), f64p), p(cnt, i32p), p(st, i32p)) == kn.OK
    assert st.tolist() == [kn.OK] * 3 and cnt.tolist() == [U - 1, U, U - 1]
    for b, (q, qi, qr) in enumerate(queries):
        n = cnt[b]
        assert ids[b, n:].tolist() == [-77] * (64 - n) and vals[b, n:].tolist() == [-77.5] * (64 - n)
        got = _check(kn, oracle, e, train, q, qi, qr, oracle.SIM_COSINE, 64)
        _same_pair((ids[b, :n], vals[b, :n]), got, b)
    # predictions and recommendations of the batch at k >= U
    pred_items = np.arange(0, 32, dtype=np.int32)
    pr, st = e.predict_with_batch(queries, [pred_items] * 3)
    rc, st2 = e.recommend_with_batch(queries, 30)
    assert st.tolist() == [kn.OK] * 3 and st2.tolist() == [kn.OK] * 3
    for b, (q, qi, qr) in enumerate(queries):
        assert _bits(pr[b]) == _bits(e.predict_with(q, qi, qr, pred_items)), b
        _same_pair(rc[b], e.recommend_with(q, qi, qr, 30), b)
    e.close()


def test_per_query_statuses(kn, syn100k):
    full = _syn100k(syn100k)
    users = _pick_users(full)
    train, rows = _hold_out(full, users, 2)
    e = kn.Engine(k=20)
    e.fit(*train)
    good = [(q,) + rows[q] for q in users[:5]]
    known = users[5]
    mine = train[1][train[0] == known]
    free = np.setdiff1d(np.unique(train[1]), mine)[:3].astype(np.int32)
    bad = [
        ((known, np.array([free[0], mine[1]], dtype=np.int32), [4.0, 3.0]), kn.E_DUPLICATE),  # against a train item
        ((known, np.array([free[0], free[1], free[0]], dtype=np.int32), [4.0, 3.0, 2.0]), kn.E_DUPLICATE),  # inside the rows
        ((known, free[:1], [np.inf]), kn.E_NONFINITE),
        ((known, free[:2], [-1.0e6, 2.0]), kn.E_UNSUPPORTED),  # negative combined mean
        ((7004, np.empty(0, dtype=np.int32), np.empty(0)), kn.E_INVALID),  # empty rows for an unknown user
    ]
    for (q, it, rt), status in bad:
        with pytest.raises(kn.KnncfError) as ex:
            e.recommend_with(q, it, rt, 3)
        assert ex.value.status == status
    # more than 65536 combined rows: the train rows count
    n_over = 65_537 - len(mine)
    with pytest.raises(kn.KnncfError) as ex:
        e.neighbors_with(known, np.arange(200_000, 200_000 + n_over, dtype=np.int32), np.full(n_over, 3.0))
    assert ex.value.status == kn.E_UNSUPPORTED
    mixed, want = [], []
    for j in range(5):
        mixed += [good[j], bad[j][0]]
        want += [kn.OK, bad[j][1]]
    pred_items = np.arange(1, 400, dtype=np.int32)
    nb, st = e.neighbors_with_batch(mixed)
    assert st.tolist() == want
    assert "query 1:" in e._lib.knncf_last_error(e._h).decode()
    pr, st = e.predict_with_batch(mixed, [pred_items] * 10)
    assert st.tolist() == want
    rc, st = e.recommend_with_batch(mixed, 5)
    assert st.tolist() == want
    for j, (q, it, rt) in enumerate(good):
        _same_pair(nb[2 * j], e.neighbors_with(q, it, rt), j)
        assert _bits(pr[2 * j]) == _bits(e.predict_with(q, it, rt, pred_items)), j
        _same_pair(rc[2 * j], e.recommend_with(q, it, rt, 5), j)
        assert len(nb[2 * j + 1][0]) == 0 and len(rc[2 * j + 1][0]) == 0 and np.isnan(pr[2 * j + 1]).all()
    # failed rows: count 0 and untouched outputs (sentinels at the C boundary)
    us, off, it, rt = e._query_batch(mixed)
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    ids = np.full((10, 5), -77, dtype=np.int32)
    vals = np.full((10, 5), -77.5)
    cnt = np.full(10, -1, dtype=np.int32)
    st = np.full(10, 99, dtype=np.int32)
    lib = e._lib
    assert lib.knncf_update_recommend_batch(e._h, kn.PRED_KNN, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), 10, 5,
                                            p(ids.reshape(-1), i32p), p(vals.reshape(-1), f64p), p(cnt, i32p), p(st, i32p)) == kn.OK
    assert st.tolist() == want
    for j in range(5):
        assert cnt[2 * j] == 5 and cnt[2 * j + 1] == 0
        assert ids[2 * j].tolist() == rc[2 * j][0].tolist()
        assert ids[2 * j + 1].tolist() == [-77] * 5 and vals[2 * j + 1].tolist() == [-77.5] * 5
    ids[:], vals[:] = -77, -77.5
    assert lib.knncf_update_neighbors_batch(e._h, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), 10, 5,
                                            p(ids.reshape(-1), i32p), p(vals.reshape(-1), f64p), p(cnt, i32p), p(st, i32p)) == kn.OK
    for j in range(5):
        assert cnt[2 * j] == 20 and cnt[2 * j + 1] == 0
        assert ids[2 * j].tolist() == nb[2 * j][0][:5].tolist()
        assert ids[2 * j + 1].tolist() == [-77] * 5 and vals[2 * j + 1].tolist() == [-77.5] * 5
    e.close()


def test_handle_level_refusals(kn, syn100k):
    train = _syn100k(syn100k)
    q = int(train[0][0])
    it, rt = np.array([UNKNOWN_ITEM], dtype=np.int32), np.array([3.0])
    good = [(q, it, rt), (5001, [4, 5], [2.0, 3.0])]

    def status_of(call):
        with pytest.raises(kn.KnncfError) as ex:
            call()
        return ex.value.status

    e = kn.Engine(k=10)
    assert status_of(lambda: e.neighbors_with(q, it, rt)) == kn.E_STATE  # before a fit
    assert status_of(lambda: e.recommend_with_batch(good, 3)) == kn.E_STATE
    e.fit(*train)
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    ids, out, c = np.empty(4, dtype=np.int32), np.empty(4), C.c_int32()
    reco = lambda pred, items, n_ratings: e._lib.knncf_update_recommend(e._h, pred, q, items, p(rt, f64p), n_ratings, 4, p(ids, i32p),
                                                                        p(out, f64p), C.byref(c))
    assert reco(kn.PRED_BASELINE, p(it, i32p), 1) == kn.E_UNSUPPORTED  # a predictor other than the kNN one
    assert reco(kn.PRED_KNN, None, 1) == kn.E_INVALID                   # null rows with n_ratings > 0
    assert reco(kn.PRED_KNN, p(it, i32p), -1) == kn.E_INVALID
    assert reco(kn.PRED_KNN, p(it, i32p), 1) == kn.OK
    e.close()
    e1 = kn.Engine(k=10, similarity=kn.SIM_ONE)
    e1.fit(*train)
    assert status_of(lambda: e1.recommend_with(q, it, rt, 3)) == kn.E_UNSUPPORTED
    assert status_of(lambda: e1.recommend_with_batch(good, 3)) == kn.E_UNSUPPORTED
    e1.close()
    es = kn.Engine(k=10, shard_rank=0, shard_count=2)  # a shard handle
    es.fit(*train)
    assert status_of(lambda: es.predict_with(q, it, rt, [1])) == kn.E_UNSUPPORTED
    assert status_of(lambda: es.predict_with_batch(good, [[1], [2]])) == kn.E_UNSUPPORTED
    es.close()
    m = np.isin(train[0], np.unique(train[0])[:4])
    e4 = kn.Engine(k=10)
    e4.fit(*(a[m] for a in train))
    assert status_of(lambda: e4.neighbors_with(q, it, rt)) == kn.E_UNSUPPORTED  # fewer than 5 train users
    assert status_of(lambda: e4.neighbors_with_batch(good)) == kn.E_UNSUPPORTED
    e4.close()


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_mixed_batch_in_large_and_small_chunks(kn, oracle, syn100k, sim_name):
    """40 answerable queries — users of the fit, others, one user of the fit twice with different rows — as one chunk (the
    whole-chunk similarity kernel) and in chunks of 5 (the per-slot kernel): every row is the single call's and the oracle's"""
    osim, esim = {"cosine": (oracle.SIM_COSINE, kn.SIM_COSINE), "jaccard": (oracle.SIM_JACCARD, kn.SIM_JACCARD)}[sim_name]
    full = _syn100k(syn100k)
    rng = np.random.default_rng(17)
    u, c = np.unique(full[0], return_counts=True)
    fitted = [int(x) for x in rng.choice(u[c > 12], 26, replace=False)]
    ms = [int(x) for x in rng.integers(1, 6, len(fitted))]
    ms[0] = 6
    train, rows = _hold_out(full, fitted, ms)
    twice = fitted[0]
    queries = [(twice, rows[twice][0][:3], rows[twice][1][:3]), (twice, rows[twice][0][3:], rows[twice][1][3:])]
    queries += [(q,) + rows[q] for q in fitted[1:]]
    queries.insert(5, (fitted[3], np.empty(0, dtype=np.int32), np.empty(0)))  # no additional rows
    outside = []
    for j in range(12):
        n = (2, 4, 5, 40)[j % 4]
        outside.append((20_000 + j, rng.choice(np.arange(1, 1700, dtype=np.int32), n, replace=False),
                        rng.integers(1, 6, n).astype(np.float64)))
    for j, x in enumerate(outside):  # interleaved
        queries.insert(3 * j + 1, x)
    assert len(queries) == 40
    pred_items = np.concatenate([np.unique(train[1])[::7], [UNKNOWN_ITEM]]).astype(np.int32)
    n_users, n_items = len(np.unique(train[0])), len(np.unique(train[1]))
    ws = _workspace_for(5, n_users, n_items)
    k = 30
    answers = []
    for workspace in (0, ws):
        e = kn.Engine(k=k, similarity=esim, workspace_bytes=workspace)
        e.fit(*train)
        if workspace:
            assert _chunk(e, ws) == 5
        nb, st = e.neighbors_with_batch(queries)
        assert st.tolist() == [kn.OK] * 40
        pr, st = e.predict_with_batch(queries, [pred_items] * 40)
        assert st.tolist() == [kn.OK] * 40
        rc, st = e.recommend_with_batch(queries, 3)
        assert st.tolist() == [kn.OK] * 40
        answers.append((nb, pr, rc))
        for b, (q, it, rt) in enumerate(queries):
            _same_pair(nb[b], e.neighbors_with(q, it, rt), (workspace, b))
            assert _bits(pr[b]) == _bits(e.predict_with(q, it, rt, pred_items)), (workspace, b)
            _same_pair(rc[b], e.recommend_with(q, it, rt, 3), (workspace, b))
        if not workspace:
            # the rows of users outside the fit are the fold-in answers
            where = [b for b, x in enumerate(queries) if x[0] >= 20_000]
            fold = [queries[b] for b in where]
            fnb, _ = e.neighbors_for_batch(fold)
            fpr, _ = e.predict_for_batch(fold, [pred_items] * len(fold))
            frc, _ = e.recommend_for_batch(fold, 3)
            for j, b in enumerate(where):
                _same_pair(nb[b], fnb[j], b)
                assert _bits(pr[b]) == _bits(fpr[j]), b
                _same_pair(rc[b], frc[j], b)
            # a permuted batch returns the same rows, permuted
            perm = rng.permutation(40)
            back = [queries[b] for b in perm]
            nb2, _ = e.neighbors_with_batch(back)
            pr2, _ = e.predict_with_batch(back, [pred_items] * 40)
            rc2, _ = e.recommend_with_batch(back, 3)
            for j, b in enumerate(perm):
                _same_pair(nb2[j], nb[b], b)
                assert _bits(pr2[j]) == _bits(pr[b]), b
                _same_pair(rc2[j], rc[b], b)
        e.close()
    # ... and the oracle's
    nb, pr, rc = answers[0]
    for b, (q, it, rt) in enumerate(queries):
        onb, opr, (orc,) = _oracle_answers(oracle, train, q, it, rt, osim, k, pred_items, [3])
        assert q not in nb[b][0].tolist()
        _same_pair(nb[b], onb, b)
        assert _bits(pr[b]) == _bits(opr), b
        _same_pair(rc[b], orc, b)


def test_fold_in_calls_still_refuse_a_train_user(kn, syn100k):
    train = _syn100k(syn100k)
    e = kn.Engine(k=10)
    e.fit(*train)
    with pytest.raises(kn.KnncfError) as ex:
        e.neighbors_for(int(train[0][0]), [UNKNOWN_ITEM], [3.0])
    assert ex.value.status == kn.E_INVALID
    assert "the user occurs in the training set" in e._lib.knncf_last_error(e._h).decode()
    _, st = e.neighbors_for_batch([(int(train[0][0]), [UNKNOWN_ITEM], [3.0]), (5000, [1, 2], [3.0, 4.0])])
    assert st.tolist() == [kn.E_INVALID, kn.OK]
    e.close()
