"""Revise queries (knncf_revise_neighbors / _predict / _recommend and their batched forms, csrc/foldin.hip): the answers for a
user of the fit who removed or re-rated items, without a refit.  Every answer is compared bit for bit with the oracle on
aug = train without the user's rows on the removed items ++ the additional rows, on a fresh pipeline whose first call is the
user's neighbourhood.  tests/test_revise_premises.py proves from the oracle alone that each removal changes the answer."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import revise_cases as rc
from tests.query_helpers import MAX_CHUNK, UNKNOWN_ITEM, _bits, _chunk, _same_pair, _workspace_for

pytestmark = pytest.mark.gpu

NONE_I, NONE_R = np.empty(0, dtype=np.int32), np.empty(0)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _oracle_answers(oracle, train, q, removed, items, ratings, sim, k, pred_items, ns):
    aug = rc.aug_of(train, q, removed, items, ratings)
    p = oracle.Model(*aug).pipeline(sim, k)
    nb = p.neighbors(q)  # first evaluation: the user's
    assert len(nb[0]) == min(k, len(np.unique(aug[0])) - 1), q  # (allUsers - u) :608
    pr = [p.predict(q, int(i)) for i in pred_items]
    n_items = len(np.unique(aug[1]))
    return nb, pr, [p.recommend(q, n_items if n is None else n) for n in ns], n_items


def _check(kn, oracle, eng, train, q, removed, items, ratings, sim, k, ns=(3, None)):
    """the three single calls against the oracle on aug; returns the neighbour list"""
    pred_items = rc.pred_items(train, q, removed, items)
    (oids, osims), want, recos, n_items = _oracle_answers(oracle, train, q, removed, items, ratings, sim, k, pred_items, ns)
    ids, sims = eng.neighbors_revised(q, removed, items, ratings)
    assert q not in ids.tolist(), q
    assert ids.tolist() == oids.tolist(), q
    assert _bits(sims) == _bits(osims), q
    assert _bits(eng.predict_revised(q, removed, items, ratings, pred_items)) == _bits(want), q
    for n, (wi, wp) in zip(ns, recos):
        n = n_items + 1 if n is None else n  # more than every item of aug: the count is what aug leaves
        gi, gp = eng.recommend_revised(q, removed, items, ratings, n)
        assert gi.tolist() == wi.tolist(), (q, n)
        assert _bits(gp) == _bits(wp), (q, n)
    return ids, sims


# ---- 1: syn-100k, cosine ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("case", rc.CASES)
@pytest.mark.parametrize("k", [300, 10])
def test_fitted_users_syn100k_cosine(kn, oracle, syn100k, k, case, shuffled):
    train = rc.syn100k(syn100k, shuffled)
    e = kn.Engine(k=k)
    e.fit(*train)
    for q in rc.pick_users(train):
        removed, items, ratings = rc.case_query(train, q, case, dyadic=not shuffled)
        _check(kn, oracle, e, train, q, removed, items, ratings, oracle.SIM_COSINE, k)
    e.close()


# ---- 2: Jaccard -------------------------------------------------------------------------------------------------------------
def test_fitted_users_syn100k_jaccard(kn, oracle, syn100k):
    train = rc.syn100k(syn100k)
    e = kn.Engine(k=50, similarity=kn.SIM_JACCARD)
    e.fit(*train)
    for n, q in enumerate(rc.pick_users(train)[:5]):
        removed, items, ratings = rc.case_query(train, q, "mixed", unknown=n == 2)  # one with an item unknown to train
        _check(kn, oracle, e, train, q, removed, items, ratings, oracle.SIM_JACCARD, 50)
    e.close()


# ---- 3: row-size classes and items that leave aug, on the hand set ------------------------------------------------------------
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_row_size_classes_and_lone_items(kn, oracle, sim_name):
    osim, esim = {"cosine": (oracle.SIM_COSINE, kn.SIM_COSINE), "jaccard": (oracle.SIM_JACCARD, kn.SIM_JACCARD)}[sim_name]
    train = rc.small_set()
    qs = rc.small_queries(train)
    n_train_items = len(np.unique(train[1]))
    assert n_train_items == 31
    for k in (10, 64):  # k >= U: every other user is a neighbour
        e = kn.Engine(k=k, similarity=esim)
        e.fit(*train)
        for name, (q, removed, items, ratings) in qs.items():
            ids, _ = _check(kn, oracle, e, train, q, removed, items, ratings, osim, k)
            if k == 64:
                assert len(ids) == 39, name  # U - 1, also for the user whose train rows are all removed
        # the item only the query user rated, removed: no candidate, whatever n; counts is one smaller; the user's mean
        q, removed, items, ratings = qs["lone_item_removed"]
        rated = int((train[0] == q).sum())
        gi, gp = e.recommend_revised(q, removed, items, ratings, 100)
        assert rc.LONE_ITEM not in gi.tolist()
        assert len(gi) == (n_train_items - 1) - (rated - 1)
        with_it, _ = e.recommend_with(q, NONE_I, NONE_R, 100)
        assert len(with_it) == n_train_items - rated and len(gi) == len(with_it)  # one item and one rated item fewer
        u, i, r = rc.aug_of(train, q, removed, items, ratings)
        mine = r[u == q]
        mean = 0.0
        for x in mine:
            mean = mean + x
        mean = mean / len(mine)
        got = e.predict_revised(q, removed, items, ratings, [rc.LONE_ITEM, UNKNOWN_ITEM])
        assert _bits(got) == _bits([mean, mean])
        # the same item removed and re-rated: it is rated, so it is not a candidate, and nothing left aug
        q, removed, items, ratings = qs["lone_item_rerated"]
        gi, _ = e.recommend_revised(q, removed, items, ratings, 100)
        assert rc.LONE_ITEM not in gi.tolist() and len(gi) == n_train_items - rated
        e.close()


# ---- 4: batches in large and small chunks -----------------------------------------------------------------------------------------
def _mixed_batch(train):
    """40 answerable queries: users of the fit with removals (one of them twice, with different removals), users of the fit
    without removals, users outside the fit; interleaved"""
    rng = np.random.default_rng(17)
    u, c = np.unique(train[0], return_counts=True)
    fitted = [int(x) for x in rng.choice(u[c > 12], 26, replace=False)]
    queries = []
    for n, q in enumerate(fitted[:18]):
        queries.append((q,) + rc.case_query(train, q, rc.CASES[n % 4]))
    queries.append((fitted[0],) + rc.case_query(train, fitted[0], "mixed"))  # the same user again, other removals
    free = lambda q: np.setdiff1d(np.unique(train[1]), train[1][train[0] == q])
    for n, q in enumerate(fitted[18:]):  # no removals: the update answer
        m = n % 3
        queries.append((q, NONE_I, free(q)[:m].astype(np.int32), np.array([4.0, 2.0])[:m]))
    outside = []
    for j in range(40 - len(queries)):
        n = (2, 4, 5, 40)[j % 4]
        outside.append((20_000 + j, NONE_I, rng.choice(np.arange(1, 1700, dtype=np.int32), n, replace=False),
                        rng.integers(1, 6, n).astype(np.float64)))
    for j, x in enumerate(outside):
        queries.insert(3 * j + 1, x)
    assert len(queries) == 40
    return queries, fitted


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_mixed_batch_in_large_and_small_chunks(kn, oracle, syn100k, sim_name):
    osim, esim = {"cosine": (oracle.SIM_COSINE, kn.SIM_COSINE), "jaccard": (oracle.SIM_JACCARD, kn.SIM_JACCARD)}[sim_name]
    train = rc.syn100k(syn100k)
    queries, fitted = _mixed_batch(train)
    known = set(train[0].tolist())
    assert sum(1 for x in queries if len(x[1])) == 19 and sum(1 for x in queries if x[0] not in known) == 13
    assert [x[0] for x in queries].count(fitted[0]) == 2
    pred_items = np.concatenate([np.unique(train[1])[::7], [UNKNOWN_ITEM]]).astype(np.int32)
    n_users, n_items = len(np.unique(train[0])), len(np.unique(train[1]))
    ws = _workspace_for(5, n_users, n_items)
    k = 30
    rng = np.random.default_rng(23)
    answers = []
    for workspace in (0, ws):
        e = kn.Engine(k=k, similarity=esim, workspace_bytes=workspace)
        e.fit(*train)
        if workspace:
            assert _chunk(e, ws) == 5
        nb, st = e.neighbors_revised_batch(queries)
        assert st.tolist() == [kn.OK] * 40
        pr, st = e.predict_revised_batch(queries, [pred_items] * 40)
        assert st.tolist() == [kn.OK] * 40
        rcm, st = e.recommend_revised_batch(queries, 3)
        assert st.tolist() == [kn.OK] * 40
        answers.append((nb, pr, rcm))
        for b, (q, rm, it, rt) in enumerate(queries):
            _same_pair(nb[b], e.neighbors_revised(q, rm, it, rt), (workspace, b))
            assert _bits(pr[b]) == _bits(e.predict_revised(q, rm, it, rt, pred_items)), (workspace, b)
            _same_pair(rcm[b], e.recommend_revised(q, rm, it, rt, 3), (workspace, b))
        if not workspace:
            # rows without removals are the update answers; those of users outside the fit the fold-in answers
            plain = [b for b, x in enumerate(queries) if len(x[1]) == 0]
            upd = [(queries[b][0],) + queries[b][2:] for b in plain]
            unb, _ = e.neighbors_with_batch(upd)
            upr, _ = e.predict_with_batch(upd, [pred_items] * len(upd))
            urc, _ = e.recommend_with_batch(upd, 3)
            for j, b in enumerate(plain):
                _same_pair(nb[b], unb[j], b)
                assert _bits(pr[b]) == _bits(upr[j]), b
                _same_pair(rcm[b], urc[j], b)
            where = [b for b in plain if queries[b][0] not in known]
            fold = [(queries[b][0],) + queries[b][2:] for b in where]
            fnb, _ = e.neighbors_for_batch(fold)
            fpr, _ = e.predict_for_batch(fold, [pred_items] * len(fold))
            frc, _ = e.recommend_for_batch(fold, 3)
            for j, b in enumerate(where):
                _same_pair(nb[b], fnb[j], b)
                assert _bits(pr[b]) == _bits(fpr[j]), b
                _same_pair(rcm[b], frc[j], b)
            # a permuted batch returns the same rows, permuted
            perm = rng.permutation(40)
            back = [queries[b] for b in perm]
            nb2, _ = e.neighbors_revised_batch(back)
            pr2, _ = e.predict_revised_batch(back, [pred_items] * 40)
            rc2, _ = e.recommend_revised_batch(back, 3)
            for j, b in enumerate(perm):
                _same_pair(nb2[j], nb[b], b)
                assert _bits(pr2[j]) == _bits(pr[b]), b
                _same_pair(rc2[j], rcm[b], b)
        e.close()
    # ... and the oracle's
    nb, pr, rcm = answers[0]
    for b, (q, rm, it, rt) in enumerate(queries):
        onb, opr, (orc,), _ = _oracle_answers(oracle, train, q, rm, it, rt, osim, k, pred_items, [3])
        _same_pair(nb[b], onb, b)
        assert _bits(pr[b]) == _bits(opr), b
        _same_pair(rcm[b], orc, b)
    for other in answers[1:]:  # the results do not depend on C
        for b in range(40):
            _same_pair(other[0][b], nb[b], b)
            assert _bits(other[1][b]) == _bits(pr[b]), b
            _same_pair(other[2][b], rcm[b], b)


# ---- 5: statuses ----------------------------------------------------------------------------------------------------------------
def test_per_query_statuses(kn, syn100k):
    train = rc.syn100k(syn100k)
    users = rc.pick_users(train)
    e = kn.Engine(k=20)
    e.fit(*train)
    good = [(q,) + rc.case_query(train, q, rc.CASES[n % 4]) for n, q in enumerate(users[:6])]
    known = users[6]
    mine = train[1][train[0] == known].astype(np.int32)
    free = np.setdiff1d(np.unique(train[1]), mine)[:3].astype(np.int32)
    bad = [
        ((known, free[:1], NONE_I, NONE_R), kn.E_INVALID, "did not rate"),                        # an item the user did not rate
        ((known, np.array([mine[0], UNKNOWN_ITEM], dtype=np.int32), NONE_I, NONE_R), kn.E_INVALID, "did not rate"),  # an unknown id
        ((known, np.array([mine[0], mine[1], mine[0]], dtype=np.int32), NONE_I, NONE_R), kn.E_INVALID, "twice"),  # an item twice
        ((7004, mine[:1], free[:2], [3.0, 4.0]), kn.E_INVALID, "not in the training set"),         # anything for a user outside the fit
        ((known, mine, NONE_I, NONE_R), kn.E_INVALID, "without a row"),                            # every row, no additional one
        ((known, mine[:1], np.array([free[0], mine[1]], dtype=np.int32), [4.0, 3.0]), kn.E_DUPLICATE, "repeat"),  # on a kept train item
    ]
    for (q, rm, it, rt), status, text in bad:
        with pytest.raises(kn.KnncfError) as ex:
            e.recommend_revised(q, rm, it, rt, 3)
        assert ex.value.status == status, text
        assert text in str(ex.value), (text, str(ex.value))
    # more removed items than train rows (cannot all be valid), and the cap: the removed train rows count
    with pytest.raises(kn.KnncfError) as ex:
        e.neighbors_revised(known, np.concatenate([mine, free[:1]]), free[1:2], [3.0])
    assert ex.value.status == kn.E_INVALID
    n_over = 65_537 - len(mine)
    with pytest.raises(kn.KnncfError) as ex:
        e.neighbors_revised(known, mine[:5], np.arange(200_000, 200_000 + n_over, dtype=np.int32), np.full(n_over, 3.0))
    assert ex.value.status == kn.E_UNSUPPORTED
    # mixed into a batch: a failed-removal slot stands between two good slots of one chunk
    mixed, want = [], []
    for j in range(6):
        mixed += [good[j], bad[j][0]]
        want += [kn.OK, bad[j][1]]
    pred_items = np.arange(1, 400, dtype=np.int32)
    nb, st = e.neighbors_revised_batch(mixed)
    assert st.tolist() == want
    err = e._lib.knncf_last_error(e._h).decode()
    assert "query 1:" in err and "did not rate" in err
    pr, st = e.predict_revised_batch(mixed, [pred_items] * 12)
    assert st.tolist() == want
    rcm, st = e.recommend_revised_batch(mixed, 5)
    assert st.tolist() == want
    for j, (q, rm, it, rt) in enumerate(good):
        _same_pair(nb[2 * j], e.neighbors_revised(q, rm, it, rt), j)
        assert _bits(pr[2 * j]) == _bits(e.predict_revised(q, rm, it, rt, pred_items)), j
        _same_pair(rcm[2 * j], e.recommend_revised(q, rm, it, rt, 5), j)
        assert len(nb[2 * j + 1][0]) == 0 and len(rcm[2 * j + 1][0]) == 0 and np.isnan(pr[2 * j + 1]).all()
    # failed rows: count 0 and untouched outputs (sentinels at the C boundary)
    args, keep = e._batch_args("revise", mixed)
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    ids = np.full((12, 5), -77, dtype=np.int32)
    vals = np.full((12, 5), -77.5)
    cnt = np.full(12, -1, dtype=np.int32)
    st = np.full(12, 99, dtype=np.int32)
    lib = e._lib
    assert lib.knncf_revise_recommend_batch(e._h, kn.PRED_KNN, *args, 5, p(ids.reshape(-1), i32p), p(vals.reshape(-1), f64p),
                                            p(cnt, i32p), p(st, i32p)) == kn.OK
    assert st.tolist() == want
    for j in range(6):
        assert cnt[2 * j] == 5 and cnt[2 * j + 1] == 0
        assert ids[2 * j].tolist() == rcm[2 * j][0].tolist()
        assert ids[2 * j + 1].tolist() == [-77] * 5 and vals[2 * j + 1].tolist() == [-77.5] * 5
    ids[:], vals[:] = -77, -77.5
    assert lib.knncf_revise_neighbors_batch(e._h, *args, 5, p(ids.reshape(-1), i32p), p(vals.reshape(-1), f64p), p(cnt, i32p),
                                            p(st, i32p)) == kn.OK
    for j in range(6):
        assert cnt[2 * j] == 20 and cnt[2 * j + 1] == 0
        assert ids[2 * j].tolist() == nb[2 * j][0][:5].tolist()
        assert ids[2 * j + 1].tolist() == [-77] * 5 and vals[2 * j + 1].tolist() == [-77.5] * 5
    # null removals with n_removed == 0 at the C boundary: the update answer
    q, _, it, rt = good[3]
    it, rt = np.ascontiguousarray(it, dtype=np.int32), np.ascontiguousarray(rt, dtype=np.float64)
    free_q = np.setdiff1d(np.unique(train[1]), train[1][train[0] == q])[:2].astype(np.int32)
    two = np.array([2.0, 5.0])
    got, gv, c = np.full(20, -77, dtype=np.int32), np.full(20, -77.5), C.c_int32(-7)
    assert lib.knncf_revise_neighbors(e._h, q, None, 0, p(free_q, i32p), p(two, f64p), 2, 20, p(got, i32p), p(gv, f64p),
                                      C.byref(c)) == kn.OK
    assert c.value == 20
    _same_pair((got, gv), e.neighbors_with(q, free_q, two), "no removals")
    assert lib.knncf_revise_neighbors(e._h, q, None, 1, p(free_q, i32p), p(two, f64p), 2, 20, p(got, i32p), p(gv, f64p),
                                      C.byref(c)) == kn.E_INVALID  # null removals with n_removed > 0
    e.close()


def test_handle_level_refusals(kn, syn100k):
    train = rc.syn100k(syn100k)
    q = int(train[0][0])
    rm = train[1][train[0] == q][:1].astype(np.int32)
    it, rt = np.array([UNKNOWN_ITEM], dtype=np.int32), np.array([3.0])
    good = [(q, rm, it, rt), (5001, NONE_I, [4, 5], [2.0, 3.0])]

    def status_of(call):
        with pytest.raises(kn.KnncfError) as ex:
            call()
        return ex.value.status

    e = kn.Engine(k=10)
    assert status_of(lambda: e.neighbors_revised(q, rm, it, rt)) == kn.E_STATE  # before a fit
    assert status_of(lambda: e.recommend_revised_batch(good, 3)) == kn.E_STATE
    e.fit(*train)
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    ids, out, c = np.empty(4, dtype=np.int32), np.empty(4), C.c_int32()
    reco = lambda pred, n_removed: e._lib.knncf_revise_recommend(e._h, pred, q, p(rm, i32p), n_removed, p(it, i32p), p(rt, f64p), 1, 4,
                                                                 p(ids, i32p), p(out, f64p), C.byref(c))
    assert reco(kn.PRED_BASELINE, 1) == kn.E_UNSUPPORTED  # a predictor other than the kNN one
    assert reco(kn.PRED_KNN, -1) == kn.E_INVALID
    assert reco(kn.PRED_KNN, 1) == kn.OK
    # the CSR of the removals is checked like offsets
    us, off = np.array([q], dtype=np.int32), np.array([0, 1], dtype=np.int64)
    cnt, st = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    batch = lambda roff: e._lib.knncf_revise_recommend_batch(e._h, kn.PRED_KNN, p(us, i32p), roff, p(rm, i32p), p(off, i64p), p(it, i32p),
                                                             p(rt, f64p), 1, 4, p(ids, i32p), p(out, f64p), p(cnt, i32p), p(st, i32p))
    assert batch(None) == kn.E_INVALID
    assert batch(p(np.array([1, 1], dtype=np.int64), i64p)) == kn.E_INVALID
    assert batch(p(np.array([0, -1], dtype=np.int64), i64p)) == kn.E_INVALID
    assert batch(p(np.array([0, 1], dtype=np.int64), i64p)) == kn.OK and st[0] == kn.OK
    e.close()
    e1 = kn.Engine(k=10, similarity=kn.SIM_ONE)
    e1.fit(*train)
    assert status_of(lambda: e1.recommend_revised(q, rm, it, rt, 3)) == kn.E_UNSUPPORTED
    assert status_of(lambda: e1.recommend_revised_batch(good, 3)) == kn.E_UNSUPPORTED
    e1.close()
    es = kn.Engine(k=10, shard_rank=0, shard_count=2)  # a shard handle
    es.fit(*train)
    assert status_of(lambda: es.predict_revised(q, rm, it, rt, [1])) == kn.E_UNSUPPORTED
    assert status_of(lambda: es.predict_revised_batch(good, [[1], [2]])) == kn.E_UNSUPPORTED
    es.close()
    m = np.isin(train[0], np.unique(train[0])[:4])
    e4 = kn.Engine(k=10)
    e4.fit(*(a[m] for a in train))
    assert status_of(lambda: e4.neighbors_revised(q, rm, it, rt)) == kn.E_UNSUPPORTED  # fewer than 5 train users
    assert status_of(lambda: e4.neighbors_revised_batch(good)) == kn.E_UNSUPPORTED
    e4.close()


# ---- 6: read-only ---------------------------------------------------------------------------------------------------------------
def test_read_only_on_the_handle(kn, syn100k, tmp_path):
    train = rc.syn100k(syn100k)
    users = rc.pick_users(train)[:4]
    e = kn.Engine(k=40)
    e.fit(*train)
    e.neighbors(int(train[0][-1]))  # something in the table
    stored = e.neighbors(users[1])
    e.neighbors_save(str(tmp_path / "before.bin"))
    queries = [(q,) + rc.case_query(train, q, rc.CASES[n % 4]) for n, q in enumerate(users)]
    for q, rm, it, rt in queries:
        e.neighbors_revised(q, rm, it, rt)
        e.predict_revised(q, rm, it, rt, [1, 2, 3])
        e.recommend_revised(q, rm, it, rt, 5)
    e.neighbors_revised_batch(queries)
    e.recommend_revised_batch(queries, 5)
    e.neighbors_save(str(tmp_path / "after.bin"))
    assert (tmp_path / "before.bin").read_bytes() == (tmp_path / "after.bin").read_bytes()
    _same_pair(stored, e.neighbors(users[1]), "stored list")  # the queried user's own list is neither read nor replaced
    e.close()
