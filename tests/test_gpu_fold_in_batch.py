"""Batched fold-in queries (knncf_query_neighbors_batch / _predict_batch / _recommend_batch, csrc/foldin.hip): B
independent queries per call, answered chunk by chunk.  Row b is compared bit for bit with the oracle on
aug_b = train ++ the rows of query b (fresh pipeline, the query user's neighbourhood first), and with the single calls
neighbors_for / predict_for / recommend_for on the same handle.  The single calls run the same code as a chunk of one, so
that second comparison is a chunk of C against chunks of one: it checks the slot indexing, the segmented sorts and
k_query_sim_dual against k_query_sim, not one implementation against another.  It runs across chunk boundaries and on both
sides of every size-dependent switch of the path:
  * chunk size C from the rule of include/knncf.h (64 at most; a small workspace_bytes makes it smaller),
  * C < 32 answerable queries: k_query_sim once per query (itself switching at 262 144 items), C >= 32: k_query_sim_dual,
  * fewer than 64 and exactly 64 live lanes in k_query_sim_dual.
(The rule's third bound, (2^31 - 1) / max(U, I), starts to bind at 33.5 M users or items: not reachable in a test.)"""
import ctypes as C
import importlib
import importlib.util
import os

import numpy as np
import pytest

from tests.query_edges import wide_train as _wide_train
from tests.query_helpers import MAX_CHUNK, UNKNOWN_ITEM, _aug, _bits, _chunk, _same_pair, _workspace_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "personal.csv")


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def latency_script():
    spec = importlib.util.spec_from_file_location("fold_in_latency", os.path.join(ROOT, "scripts", "fold_in_latency.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _batch_vs_singles(kn, e, queries, pred_items, ns=(3,)):
    """the three batch calls against the single calls (chunks of one) of the same handle; returns the batch answers"""
    nb, st = e.neighbors_for_batch(queries)
    assert st.tolist() == [kn.OK] * len(queries)
    pr, st = e.predict_for_batch(queries, [pred_items] * len(queries))
    assert st.tolist() == [kn.OK] * len(queries)
    recos = {}
    for n in ns:
        recos[n], st = e.recommend_for_batch(queries, n)
        assert st.tolist() == [kn.OK] * len(queries)
    for b, (q, it, rt) in enumerate(queries):
        _same_pair(nb[b], e.neighbors_for(q, it, rt), ("neighbours", b))
        assert _bits(pr[b]) == _bits(e.predict_for(q, it, rt, pred_items)), ("predictions", b)
        for n in ns:
            _same_pair(recos[n][b], e.recommend_for(q, it, rt, n), ("recommendations", n, b))
    return nb, pr, recos


def _holdout_users(train):
    u, c = np.unique(train[0], return_counts=True)
    order = np.argsort(c, kind="stable")
    picks = [int(u[order[0]]), int(u[order[-1]])]
    for target in (20, 60, 200):
        picks.append(int(u[np.argmin(np.abs(c - target))]))
    rng = np.random.default_rng(7)
    picks += [int(x) for x in rng.choice(u, 12, replace=False)]
    return list(dict.fromkeys(picks))


def _oracle_batch(kn, syn100k):
    """(train = syn100k minus the held-out set H, the batch of the issue's first check)"""
    d = syn100k
    full = (d.train.users, d.train.items, d.train.ratings)
    held = _holdout_users(full)
    m = np.isin(full[0], held)
    train = tuple(a[~m] for a in full)
    rows = lambda q: (full[1][full[0] == q], full[2][full[0] == q])
    queries = [(q,) + rows(q) for q in held]
    it0, rt0 = rows(held[2])
    for n in (1, 3, 4, 5):  # prefixes of a held-out row
        queries.append((held[2], it0[:n], rt0[:n]))
    it1 = rows(held[1])[0][:3]  # a 3-rating query in two row orders
    rt1 = np.array([5.0, 1.0, 3.0])
    queries.append((5001, it1, rt1))
    queries.append((5001, it1[[2, 0, 1]], rt1[[2, 0, 1]]))
    it2, rt2 = rows(held[3])  # items unknown to train among the query's
    it2 = it2.copy()
    it2[::4] = np.arange(100_000, 100_000 + len(it2[::4]), dtype=np.int32)
    queries.append((held[3], it2, rt2))
    assert 944 not in set(train[0].tolist())
    _, (pu, pi, pr) = kn.load_personal(GOLDEN, 944)
    queries.append((944, pi, pr))
    it3 = rows(held[1])[0][:40]  # non-dyadic ratings
    rt3 = np.round(np.linspace(0.7, 4.9, len(it3)), 1)
    rt3[::3] = 3.7
    queries.append((5002, it3, rt3))
    return train, queries


@pytest.mark.parametrize("sim_name,k", [("cosine", 300), ("cosine", 10), ("jaccard", 50)])
def test_batch_against_the_oracle(kn, oracle, syn100k, sim_name, k):
    train, queries = _oracle_batch(kn, syn100k)
    osim, esim = {"cosine": (oracle.SIM_COSINE, kn.SIM_COSINE), "jaccard": (oracle.SIM_JACCARD, kn.SIM_JACCARD)}[sim_name]
    all_items = np.unique(train[1])
    n_users = len(np.unique(train[0]))
    e = kn.Engine(k=k, similarity=esim)
    e.fit(*train)
    pred_items = [np.concatenate([all_items, it, [UNKNOWN_ITEM]]).astype(np.int32) for _, it, _ in queries]
    nb, st = e.neighbors_for_batch(queries)
    assert st.tolist() == [kn.OK] * len(queries)
    pr, st = e.predict_for_batch(queries, pred_items)
    assert st.tolist() == [kn.OK] * len(queries)
    r3, st = e.recommend_for_batch(queries, 3)
    assert st.tolist() == [kn.OK] * len(queries)
    n_all = len(all_items) + 200  # more than the train items: every unrated one
    rall, st = e.recommend_for_batch(queries, n_all)
    assert st.tolist() == [kn.OK] * len(queries)
    e.close()
    for b, (q, it, rt) in enumerate(queries):
        p = oracle.Model(*_aug(train, q, it, rt)).pipeline(osim, k)
        oids, osims = p.neighbors(q)  # first evaluation: the query user's
        assert len(oids) == min(k, n_users), b
        assert nb[b][0].tolist() == oids.tolist(), b
        assert _bits(nb[b][1]) == _bits(osims), b
        assert _bits(pr[b]) == _bits([p.predict(q, int(i)) for i in pred_items[b]]), b
        n_items = len(np.unique(np.concatenate([train[1], np.asarray(it, dtype=np.int32)])))
        for got, n in ((r3[b], 3), (rall[b], n_items)):
            wi, wp = p.recommend(q, n)
            assert got[0].tolist() == wi.tolist(), (b, n)
            assert _bits(got[1]) == _bits(wp), (b, n)


def test_chunks_against_the_single_calls(kn, syn100k, latency_script):
    """13 queries at 5 per chunk: chunks of 5, 5 and 3 against 13 chunks of one; the reversed batch gives the reversed rows"""
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    n_users, n_items = len(np.unique(train[0])), len(np.unique(train[1]))
    ws = _workspace_for(5, n_users, n_items)
    e = kn.Engine(k=40, workspace_bytes=ws)
    e.fit(*train)
    assert _chunk(e, ws) == 5
    queries = latency_script._queries(d, 13, seed=11)
    pred_items = np.concatenate([np.unique(train[1])[::7], [UNKNOWN_ITEM]]).astype(np.int32)
    nb, pr, recos = _batch_vs_singles(kn, e, queries, pred_items, ns=(3, 25))
    back = queries[::-1]
    nb2, _ = e.neighbors_for_batch(back)
    pr2, _ = e.predict_for_batch(back, [pred_items] * len(back))
    r2, _ = e.recommend_for_batch(back, 3)
    for b in range(len(queries)):
        _same_pair(nb2[len(queries) - 1 - b], nb[b], b)
        assert _bits(pr2[len(queries) - 1 - b]) == _bits(pr[b]), b
        _same_pair(r2[len(queries) - 1 - b], recos[3][b], b)
    e.close()


@pytest.mark.parametrize("chunk,count", [(1, 2), (31, 31), (32, 32), (64, 70)])
def test_switches_of_the_similarity_pass(kn, syn100k, latency_script, chunk, count):
    """chunks of 1 and 31 (k_query_sim per query), of 32 (the smallest k_query_sim_dual), of 64 + 6 (every lane live, then 6
    through k_query_sim), each against the single calls' chunks of one (k_query_sim)"""
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    n_users, n_items = len(np.unique(train[0])), len(np.unique(train[1]))
    ws = _workspace_for(chunk, n_users, n_items)
    for esim in (kn.SIM_COSINE, kn.SIM_JACCARD):
        e = kn.Engine(k=30, similarity=esim, workspace_bytes=ws)
        e.fit(*train)
        assert _chunk(e, ws) == chunk
        queries = latency_script._queries(d, count, seed=11)
        queries[1] = (queries[1][0], queries[1][1][:3], queries[1][2][:3])  # a <= 4-rating slot beside long ones
        _batch_vs_singles(kn, e, queries, np.unique(train[1])[::11].astype(np.int32))
        e.close()


@pytest.mark.parametrize("n_items", [262_144, 262_145 + 64])
@pytest.mark.parametrize("chunk", [2, 33])
def test_both_sides_of_the_item_bitmap_switch(kn, n_items, chunk):
    """foldin.hip holds a query's bitmap in LDS up to 262 144 items (4096 words) and probes global memory beyond; the
    per-query kernel (chunk 2) and the chunk kernel (chunk 33, then a chunk of 1) on both sides"""
    train = _wide_train(n_items)
    ws = _workspace_for(chunk, 400, n_items)
    e = kn.Engine(k=25, workspace_bytes=ws)
    e.fit(*train)
    assert e.num_items == n_items and _chunk(e, ws) == chunk
    rng = np.random.default_rng(23)
    queries = []
    for j in range(chunk + 1):
        m = (3, 30, 200)[j % 3]
        its = rng.choice(n_items - 100, m, replace=False).astype(np.int32)
        its[-1] = n_items - 1 - j  # the last bitmap word
        queries.append((1000 + j, its, rng.integers(1, 11, m).astype(np.float64) / 2))
    pred_items = np.concatenate([rng.choice(n_items, 500, replace=False), [n_items + 5]]).astype(np.int32)
    _batch_vs_singles(kn, e, queries, pred_items)
    e.close()


def test_per_query_statuses(kn, syn100k, latency_script):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    e = kn.Engine(k=20)
    e.fit(*train)
    good = latency_script._queries(d, 6, seed=11)
    bad = [
        ((7000, [1, 2, 1], [4.0, 3.0, 2.0]), kn.E_DUPLICATE),
        ((7001, [1, 2], [6.0, 4.0]), kn.E_NONFINITE),  # mean 5, 6 > 5: scale() == 0
        ((7002, [1, 2, 3], [-4.0, -3.0, 1.0]), kn.E_UNSUPPORTED),  # negative mean
        ((int(train[0][0]), [1, 2, 3], [4.0, 3.0, 5.0]), kn.E_INVALID),  # the user occurs in train
        ((7003, np.arange(1, 65_539, dtype=np.int32), np.full(65_538, 3.0)), kn.E_UNSUPPORTED),
        ((7004, np.empty(0, dtype=np.int32), np.empty(0)), kn.E_INVALID),
    ]
    # the single calls return the query's status as their own (the empty query is refused by the wrapper: asked at the C boundary)
    for (q, it, rt), status in bad[:-1]:
        with pytest.raises(kn.KnncfError) as ex:
            e.recommend_for(q, it, rt, 3)
        assert ex.value.status == status
    mixed, want = [], []
    for j in range(6):
        mixed += [good[j], bad[j][0]]
        want += [kn.OK, bad[j][1]]
    pred_items = np.arange(1, 400, dtype=np.int32)
    nb_good, _ = e.neighbors_for_batch(good)
    pr_good, _ = e.predict_for_batch(good, [pred_items] * 6)
    re_good, _ = e.recommend_for_batch(good, 5)
    nb, st = e.neighbors_for_batch(mixed)
    assert st.tolist() == want
    pr, st = e.predict_for_batch(mixed, [pred_items] * 12)
    assert st.tolist() == want
    rc, st = e.recommend_for_batch(mixed, 5)
    assert st.tolist() == want
    assert "query 1:" in e._lib.knncf_last_error(e._h).decode()
    for j in range(6):
        _same_pair(nb[2 * j], nb_good[j], j)
        assert _bits(pr[2 * j]) == _bits(pr_good[j]), j
        _same_pair(rc[2 * j], re_good[j], j)
        assert len(nb[2 * j + 1][0]) == 0 and len(rc[2 * j + 1][0]) == 0
    # output rows of failed queries are left untouched: sentinels at the C boundary
    lib = kn.load_library()
    us, off, it, rt = e._query_batch(mixed)
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    ids = np.full((12, 5), -77, dtype=np.int32)
    vals = np.full((12, 5), -77.5)
    cnt = np.full(12, -1, dtype=np.int32)
    st = np.full(12, 99, dtype=np.int32)
    assert lib.knncf_query_recommend_batch(e._h, kn.PRED_KNN, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), 12, 5,
                                           p(ids.reshape(-1), i32p), p(vals.reshape(-1), f64p), p(cnt, i32p), p(st, i32p)) == kn.OK
    assert st.tolist() == want
    for j in range(6):
        assert cnt[2 * j] == 5 and cnt[2 * j + 1] == 0
        assert ids[2 * j].tolist() == re_good[j][0].tolist()
        assert ids[2 * j + 1].tolist() == [-77] * 5 and vals[2 * j + 1].tolist() == [-77.5] * 5
    ids[:], vals[:] = -77, -77.5
    assert lib.knncf_query_neighbors_batch(e._h, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), 12, 5,
                                           p(ids.reshape(-1), i32p), p(vals.reshape(-1), f64p), p(cnt, i32p), p(st, i32p)) == kn.OK
    for j in range(6):
        assert cnt[2 * j] == 20 and cnt[2 * j + 1] == 0
        assert ids[2 * j].tolist() == nb_good[j][0][:5].tolist()
        assert ids[2 * j + 1].tolist() == [-77] * 5 and vals[2 * j + 1].tolist() == [-77.5] * 5
    poff = np.arange(13, dtype=np.int64) * len(pred_items)
    pit = np.tile(pred_items, 12)
    out = np.full(len(pit), -77.5)
    assert lib.knncf_query_predict_batch(e._h, kn.PRED_KNN, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), 12, p(poff, i64p),
                                         p(pit, i32p), p(out, f64p), p(st, i32p)) == kn.OK
    out = out.reshape(12, -1)
    for j in range(6):
        assert _bits(out[2 * j]) == _bits(pr_good[j])
        assert set(out[2 * j + 1].tolist()) == {-77.5}
    e.close()


def test_the_same_user_in_two_queries(kn, syn100k, latency_script):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    e = kn.Engine(k=30)
    e.fit(*train)
    a, b, c, f, g = latency_script._queries(d, 5, seed=11)
    queries = [(9000, a[1], a[2]), (9000, b[1], b[2]), c, (9000, a[1][:4], a[2][:4]), f, g]
    _batch_vs_singles(kn, e, queries, np.unique(train[1])[::5].astype(np.int32))
    e.close()


def test_batches_leave_the_handle_untouched(kn, syn100k, latency_script, tmp_path):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    test = (d.test.users, d.test.items, d.test.ratings)
    users = np.unique(train[0])
    queries = latency_script._queries(d, 20, seed=11)

    def session(path, with_batches):
        e = kn.Engine(k=40)
        e.fit(*train)
        first = (e.mae(kn.PRED_KNN, *test), e.neighbors_batch(users[[4, 80, 500]]))
        if with_batches:
            e.neighbors_for_batch(queries)
            e.predict_for_batch(queries, [np.arange(1, 1700, dtype=np.int32)] * len(queries))
            e.recommend_for_batch(queries, 10)
        e.neighbors_save(str(path))
        second = (e.mae(kn.PRED_KNN, *test), e.neighbors_batch(users[[4, 80, 500, 900]]))
        e.close()
        return first, second

    fa, sa = session(tmp_path / "a.bin", True)
    fb, sb = session(tmp_path / "b.bin", False)
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes()
    for x, y in ((fa, fb), (sa, sb)):
        assert _bits([x[0]]) == _bits([y[0]])
        for p, q in zip(x[1], y[1]):
            assert np.array_equal(np.asarray(p).view(np.uint8), np.asarray(q).view(np.uint8))


def test_call_level_errors(kn, syn100k):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    good = [(5000, [1, 2, 3, 50], [4.0, 3.0, 5.0, 1.0]), (5001, [4, 5], [2.0, 3.0])]

    def status_of(call):
        with pytest.raises(kn.KnncfError) as ex:
            call()
        return ex.value.status

    e = kn.Engine(k=10)
    assert status_of(lambda: e.neighbors_for_batch(good)) == kn.E_STATE  # before a fit
    e.fit(*train)
    lib = kn.load_library()
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    us, off, it, rt = e._query_batch(good)
    ids = np.full(6, -77, dtype=np.int32)
    vals = np.full(6, -77.5)
    cnt = np.full(2, -1, dtype=np.int32)
    st = np.full(2, 99, dtype=np.int32)
    outs = (p(ids, i32p), p(vals, f64p), p(cnt, i32p), p(st, i32p))
    reco = lambda pred, o, nq=2, n=3: lib.knncf_query_recommend_batch(e._h, pred, p(us, i32p), p(o, i64p), p(it, i32p), p(rt, f64p),
                                                                      nq, n, *outs)
    assert reco(kn.PRED_BASELINE, off) == kn.E_UNSUPPORTED  # another predictor
    assert reco(kn.PRED_KNN, np.array([1, 4, 6], dtype=np.int64)) == kn.E_INVALID  # offsets not starting at 0
    assert reco(kn.PRED_KNN, np.array([0, 4, 3], dtype=np.int64)) == kn.E_INVALID  # offsets decreasing
    assert reco(kn.PRED_KNN, off, nq=-1) == kn.E_INVALID
    assert reco(kn.PRED_KNN, off, n=-1) == kn.E_INVALID
    assert lib.knncf_query_recommend_batch(e._h, kn.PRED_KNN, p(us, i32p), None, p(it, i32p), p(rt, f64p), 2, 3, *outs) == kn.E_INVALID
    assert ids.tolist() == [-77] * 6 and st.tolist() == [99, 99]
    assert reco(kn.PRED_KNN, off, nq=0) == kn.OK  # an empty batch touches nothing
    assert ids.tolist() == [-77] * 6 and st.tolist() == [99, 99] and cnt.tolist() == [-1, -1]
    assert reco(kn.PRED_KNN, off) == kn.OK
    assert st.tolist() == [kn.OK, kn.OK] and cnt.tolist() == [3, 3]
    e.close()
    e1 = kn.Engine(k=10, similarity=kn.SIM_ONE)
    e1.fit(*train)
    assert status_of(lambda: e1.recommend_for_batch(good, 3)) == kn.E_UNSUPPORTED
    e1.close()
    es = kn.Engine(k=10, shard_rank=0, shard_count=2)  # a shard handle
    es.fit(*train)
    assert status_of(lambda: es.predict_for_batch(good, [[1], [2]])) == kn.E_UNSUPPORTED
    es.close()
    m = np.isin(train[0], np.unique(train[0])[:4])
    e4 = kn.Engine(k=10)
    e4.fit(*(a[m] for a in train))
    assert status_of(lambda: e4.neighbors_for_batch(good)) == kn.E_UNSUPPORTED  # fewer than 5 train users
    e4.close()
