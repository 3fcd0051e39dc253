"""KNNCF_PRED_PERSONALIZED on the query families (knncf_query_* / knncf_update_* / knncf_revise_* predict and recommend, single
and batched; csrc/foldin.hip: k_qb_self_sim, k_qb_sim_transpose, k_qb_fold_all).  Every answer is compared bit for bit with
oracle.Model(*aug).pipeline(sim, -1): predictor(aug, weightedSumDeviation(aug, S)) on fresh closures on which only the query user
is evaluated.  tests/test_personalized_query_premises.py shows on the CPU that these inputs exercise the own term's weight
S(u, u) != 1, its place in the item's file order, and the difference to the kNN predictor with k = U."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import personalized_query_cases as pc
from tests.query_helpers import _chunk, _same_pair, _workspace_for

pytestmark = pytest.mark.gpu

TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _sims(kn, oracle, name):
    return {"cosine": (oracle.SIM_COSINE, kn.SIM_COSINE), "jaccard": (oracle.SIM_JACCARD, kn.SIM_JACCARD)}[name]


def _n_items(train, items):
    return len(np.unique(np.concatenate([train[1], np.asarray(items, dtype=np.int32)])))


def _single(kn, e, family, q, removed, items, ratings, want_items, ns):
    """(predictions, [recommendations]) of one query through the single calls of `family`"""
    P = kn.PRED_PERSONALIZED
    if family == "query":
        return (e.predict_for(q, items, ratings, want_items, predictor=P), [e.recommend_for(q, items, ratings, n, predictor=P) for n in ns])
    if family == "update":
        return (e.predict_with(q, items, ratings, want_items, predictor=P), [e.recommend_with(q, items, ratings, n, predictor=P) for n in ns])
    return (e.predict_revised(q, removed, items, ratings, want_items, predictor=P),
            [e.recommend_revised(q, removed, items, ratings, n, predictor=P) for n in ns])


def _batched(kn, e, family, queries, want_items, ns):
    """the same through the batched calls: queries = [(q, removed, items, ratings)], want_items one array per query"""
    P = kn.PRED_PERSONALIZED
    name = {"query": "for", "update": "with", "revise": "revised"}[family]
    rows = [x if family == "revise" else (x[0], x[2], x[3]) for x in queries]
    pr, st = getattr(e, f"predict_{name}_batch")(rows, want_items, predictor=P)
    assert st.tolist() == [kn.OK] * len(queries)
    recos = []
    for n in ns:
        rc, st = getattr(e, f"recommend_{name}_batch")(rows, n, predictor=P)
        assert st.tolist() == [kn.OK] * len(queries)
        recos.append(rc)
    return pr, recos


def _check(kn, oracle, e, train, family, queries, osim, ns=(3, None)):
    """every query through the single and the batched calls of `family` against the oracle on its aug"""
    want_items = [pc.pred_items(train, q, rm, it) for q, rm, it, rt in queries]
    widest = max(_n_items(train, it) for q, rm, it, rt in queries)
    ns = [widest if n is None else n for n in ns]
    bpr, brc = _batched(kn, e, family, queries, want_items, ns)
    for b, (q, rm, it, rt) in enumerate(queries):
        want, recos = pc.oracle_answers(oracle, pc.aug_of(train, q, rm, it, rt), q, osim, want_items[b], ns)
        got, got_recos = _single(kn, e, family, q, rm, it, rt, want_items[b], ns)
        assert pc.bits(got) == pc.bits(want), (family, q)
        assert pc.bits(bpr[b]) == pc.bits(want), (family, q)
        for j, n in enumerate(ns):
            _same_pair(got_recos[j], recos[j], (family, q, n))
            _same_pair(brc[j][b], recos[j], (family, q, n))


# ---- syn-100k ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_fold_in_users_syn100k(kn, oracle, syn100k, sim_name):
    """the user's rows taken out of train entirely and given as the query"""
    osim, esim = _sims(kn, oracle, sim_name)
    full = pc.syn100k(syn100k)
    users = pc.pick_users(full)[:6]
    mask = np.isin(full[0], users)
    train = tuple(a[~mask] for a in full)
    queries = []
    for n, q in enumerate(users):
        at = full[0] == q
        items, ratings = full[1][at].astype(np.int32), full[2][at]
        if n == 1:  # an additional item unknown to train: one term, the user's own
            items, ratings = np.append(items, pc.NEW_ITEM).astype(np.int32), np.append(ratings, 2.0)
        queries.append((q, pc.NONE_I, items, ratings))
    e = kn.Engine(k=10, similarity=esim)
    e.fit(*train)
    _check(kn, oracle, e, train, "query", queries, osim)
    e.close()


@pytest.mark.parametrize("m", [1, 3, 10])
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_update_users_syn100k(kn, oracle, syn100k, sim_name, m):
    """the last m file rows held out and given back as additional rows"""
    osim, esim = _sims(kn, oracle, sim_name)
    full = pc.syn100k(syn100k)
    users = pc.pick_users(full)[:7 if sim_name == "cosine" else 4]
    train, rows = pc.hold_out(full, users, m)
    queries = [(q, pc.NONE_I) + rows[q] for q in users]
    it, rt = queries[2][2], queries[2][3]
    queries[2] = (users[2], pc.NONE_I, np.append(it, pc.NEW_ITEM).astype(np.int32), np.append(rt, 4.0))
    e = kn.Engine(k=40, similarity=esim)
    e.fit(*train)
    _check(kn, oracle, e, train, "update", queries, osim)
    e.close()


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_revise_users_syn100k(kn, oracle, syn100k, sim_name):
    """a removed item others rate, a re-rated item, both with a new item; and a removed item whose only rater was the user"""
    osim, esim = _sims(kn, oracle, sim_name)
    u, i, r = pc.syn100k(syn100k)
    users = pc.pick_users((u, i, r))[:4]
    lone = 555_555  # an item that users[0] alone rates in train
    train = (np.append(u, users[0]).astype(np.int32), np.append(i, lone).astype(np.int32), np.append(r, 4.0))
    queries = []
    for q in users:
        queries += [(q,) + x for x in pc.revise_queries(train, q).values()]
    queries.append((users[0], np.array([lone], dtype=np.int32), pc.NONE_I, pc.NONE_R))
    e = kn.Engine(k=40, similarity=esim)
    e.fit(*train)
    _check(kn, oracle, e, train, "revise", queries, osim)
    # the item that left aug answers the mean and is no candidate
    q, rm, it, rt = queries[-1]
    got = e.predict_revised(q, rm, it, rt, [lone], predictor=kn.PRED_PERSONALIZED)
    aug = pc.aug_of(train, q, rm, it, rt)
    assert pc.bits(got) == pc.bits([oracle.Model(*aug).users_avg(q)])
    ids, _ = e.recommend_revised(q, rm, it, rt, _n_items(train, []), predictor=kn.PRED_PERSONALIZED)
    assert lone not in ids.tolist() and len(ids) == len(np.unique(aug[1])) - int((aug[0] == q).sum())
    e.close()


def test_file_order_and_non_dyadic_ratings(kn, oracle, syn100k):
    """shuffled file rows and ratings whose sums round: the own term's place and every fold order show"""
    full = pc.syn100k(syn100k, shuffled=True)
    users = pc.pick_users(full)[:5]
    train, rows = pc.hold_out(full, users, 3)
    e = kn.Engine(k=40)
    e.fit(*train)
    _check(kn, oracle, e, train, "update", [(q, pc.NONE_I) + rows[q] for q in users], oracle.SIM_COSINE)
    queries = [(users[1],) + pc.revise_queries(train, users[1])["mixed"], (users[3],) + pc.revise_queries(train, users[3])["rerated"]]
    _check(kn, oracle, e, train, "revise", queries, oracle.SIM_COSINE)
    q = 70_001
    _check(kn, oracle, e, train, "query", [(q, pc.NONE_I) + rows[users[0]]], oracle.SIM_COSINE)
    e.close()


# ---- the hand set: the edges of the fold -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_fold_edges_hand_set(kn, oracle, sim_name):
    osim, esim = _sims(kn, oracle, sim_name)
    train = pc.edge_set()
    qs = pc.edge_queries(train)
    e = kn.Engine(k=10, similarity=esim)
    e.fit(*train)
    fold_in = [qs[n] for n in qs if n.startswith("new_")]
    update = [qs[n] for n in qs if n.startswith("update_")]
    _check(kn, oracle, e, train, "query", fold_in, osim, ns=(3, 7))
    _check(kn, oracle, e, train, "update", update + fold_in, osim, ns=(3, 7))
    _check(kn, oracle, e, train, "revise", list(qs.values()), osim, ns=(3, 7))
    # the item that only the query user rates: one term, not the mean (cosine: S(u, u) of a 6-row user; Jaccard: 1.0)
    q, rm, it, rt = qs["new_6"]
    got = e.predict_for(q, it, rt, [pc.NEW_ITEM, pc.UNKNOWN_ITEM], predictor=kn.PRED_PERSONALIZED)
    mean = oracle.Model(*pc.aug_of(train, q, rm, it, rt)).users_avg(q)
    assert got[0] != mean and pc.bits(got[1:]) == pc.bits([mean])
    assert pc.bits(e.predict_for(q, it, rt, [pc.NEW_ITEM])) == pc.bits([mean])  # the kNN predictor answers the mean there
    e.close()


# ---- chunks ---------------------------------------------------------------------------------------------------------------------
def _mixed_batch(full):
    """65 queries as (user, removed, items, ratings): update, revise and fold-in queries interleaved, query 30 repeats an item
    (refused), query 40 names the user of query 1 again with other rows"""
    rng = np.random.default_rng(29)
    u, c = np.unique(full[0], return_counts=True)
    fitted = [int(x) for x in rng.choice(u[c > 14], 44, replace=False)]
    train, rows = pc.hold_out(full, fitted[:22], 3)
    queries = []
    for j in range(22):
        queries.append((fitted[j], pc.NONE_I) + rows[fitted[j]])
        kind = ("removed", "rerated", "mixed")[j % 3]
        queries.append((fitted[22 + j],) + pc.revise_queries(train, fitted[22 + j])[kind])
        n = (1, 4, 5, 40)[j % 4]
        queries.append((30_000 + j, pc.NONE_I, rng.choice(np.arange(1, 1600, dtype=np.int32), n, replace=False).astype(np.int32),
                        rng.integers(1, 6, n).astype(np.float64)))
    queries = queries[:65]
    queries[30] = (30_500, pc.NONE_I, np.array([7, 9, 7], dtype=np.int32), np.array([3.0, 4.0, 5.0]))
    queries[40] = (queries[1][0], pc.NONE_I, np.array([pc.NEW_ITEM], dtype=np.int32), np.array([4.5]))
    assert len(queries) == 65
    return train, queries


def _trace(capfd):
    return [ln[len("knncf-dispatch "):] for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch ")]


def test_mixed_batch_in_chunks(kn, oracle, syn100k, monkeypatch, capfd):
    """the same 65 queries at the default budget (64 + 1), at C = 33 and C = 31 (both similarity kernels, strides 64, 32, 4, 1)
    and as 65 single calls: identical rows, a dozen of them the oracle's, the refused query untouched, and only the new fold in
    the dispatch trace"""
    full = pc.syn100k(syn100k)
    train, queries = _mixed_batch(full)
    P = kn.PRED_PERSONALIZED
    n_users, n_items = len(np.unique(train[0])), len(np.unique(train[1]))
    want_items = np.concatenate([np.unique(train[1])[::5], [pc.UNKNOWN_ITEM, pc.NEW_ITEM]]).astype(np.int32)
    bad = 30
    want_status = [kn.E_DUPLICATE if b == bad else kn.OK for b in range(65)]
    monkeypatch.setenv(TRACE, "1")
    runs = []
    for chunk, strides in ((0, [64, 1]), (33, [64, 32]), (31, [32, 32, 4])):
        e = kn.Engine(k=20, workspace_bytes=_workspace_for(chunk, n_users, n_items) if chunk else 0)
        e.fit(*train)
        if chunk:
            assert _chunk(e, _workspace_for(chunk, n_users, n_items)) == chunk
        capfd.readouterr()
        pr, st = e.predict_revised_batch(queries, [want_items] * 65, predictor=P)
        assert st.tolist() == want_status
        assert _trace(capfd) == [f"qb_fold_all stride={s}" for s in strides]  # no gather, no sort, no neighbour lists
        rc, st = e.recommend_revised_batch(queries, 3, predictor=P)
        assert st.tolist() == want_status
        assert _trace(capfd) == [f"qb_fold_all stride={s}" for s in strides]
        runs.append((pr, rc))
        if chunk == 0:
            # the refused row at the C boundary: count 0, sentinels untouched
            args, keep = e._batch_args("revise", queries)
            i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
            ids, vals = np.full((65, 3), -77, dtype=np.int32), np.full((65, 3), -77.5)
            cnt, sts = np.full(65, -1, dtype=np.int32), np.full(65, 99, dtype=np.int32)
            assert e._lib.knncf_revise_recommend_batch(e._h, P, *args, 3, ids.reshape(-1).ctypes.data_as(i32p),
                                                       vals.reshape(-1).ctypes.data_as(f64p), cnt.ctypes.data_as(i32p),
                                                       sts.ctypes.data_as(i32p)) == kn.OK
            assert sts.tolist() == want_status and cnt[bad] == 0 and cnt.tolist().count(3) == 64
            assert ids[bad].tolist() == [-77] * 3 and vals[bad].tolist() == [-77.5] * 3
            assert "query 30:" in e._lib.knncf_last_error(e._h).decode()
            capfd.readouterr()
            single = []
            for b, (q, rm, it, rt) in enumerate(queries):
                if b == bad:
                    with pytest.raises(kn.KnncfError) as ex:
                        e.predict_revised(q, rm, it, rt, want_items, predictor=P)
                    assert ex.value.status == kn.E_DUPLICATE
                    single.append(None)
                    continue
                single.append((e.predict_revised(q, rm, it, rt, want_items, predictor=P), e.recommend_revised(q, rm, it, rt, 3, predictor=P)))
            assert _trace(capfd) == ["qb_fold_all stride=1"] * 128
        e.close()
    monkeypatch.delenv(TRACE)
    for b in range(65):
        if b == bad:
            for pr, rc in runs:
                assert np.isnan(pr[b]).all() and len(rc[b][0]) == 0
            continue
        for pr, rc in runs[1:] + [([x[0] if x else None for x in single], [x[1] if x else None for x in single])]:
            assert pc.bits(pr[b]) == pc.bits(runs[0][0][b]), b
            _same_pair(rc[b], runs[0][1][b], b)
    for b in (0, 1, 2, 3, 4, 5, 29, 31, 40, 41, 63, 64):
        q, rm, it, rt = queries[b]
        want, (reco,) = pc.oracle_answers(oracle, pc.aug_of(train, q, rm, it, rt), q, oracle.SIM_COSINE, want_items, [3])
        assert pc.bits(runs[0][0][b]) == pc.bits(want), b
        _same_pair(runs[0][1][b], reco, b)


# ---- past 2048 users --------------------------------------------------------------------------------------------------------------
def test_past_the_table_limit(kn, oracle):
    """2 100 users: beyond the handle's k cap and the fitted path's U x U table, neither of which this path has"""
    full = pc.wide_set()
    users = [17, 1033, 2100]
    train, rows = pc.hold_out(full, users, 2)
    assert len(np.unique(train[0])) == 2100
    e = kn.Engine(k=30)
    e.fit(*train)
    queries = [(q, pc.NONE_I) + rows[q] for q in users]
    queries.append((9001, pc.NONE_I, np.array([5, 77, 123, 250, 299, pc.NEW_ITEM], dtype=np.int32), np.array([4.5, 1.0, 3.5, 2.0, 5.0, 3.0])))
    _check(kn, oracle, e, train, "update", queries, oracle.SIM_COSINE, ns=(3,))
    e.close()


# ---- state and refusals ----------------------------------------------------------------------------------------------------------
def test_handle_state_and_k(kn, oracle, syn100k, tmp_path):
    full = pc.syn100k(syn100k)
    users = pc.pick_users(full)[:3]
    train, rows = pc.hold_out(full, users, 3)
    P = kn.PRED_PERSONALIZED
    want_items = np.unique(train[1])[::3].astype(np.int32)
    answers = []
    for k in (10, 300):
        e = kn.Engine(k=k)
        e.fit(*train)
        e.neighbors(int(train[0][-1]))  # something in the table
        stored = e.neighbors(users[1])
        e.neighbors_save(str(tmp_path / "before.bin"))
        e.reset_timings()
        got = []
        for q in users:
            got.append((e.predict_with(q, *rows[q], want_items, predictor=P), e.recommend_with(q, *rows[q], 5, predictor=P),
                        e.predict_with(q, [], [], want_items, predictor=P)))
        rc, st = e.recommend_with_batch([(q,) + rows[q] for q in users], 5, predictor=P)
        for b in range(3):
            _same_pair(rc[b], got[b][1], b)
        e.neighbors_save(str(tmp_path / "after.bin"))
        assert (tmp_path / "before.bin").read_bytes() == (tmp_path / "after.bin").read_bytes()
        _same_pair(stored, e.neighbors(users[1]), "stored list")
        t = e.timings()
        assert t["predict_ms"] > 0 and t["prep_ms"] > 0  # the fold; the file-order rater copies, built by the first such call
        e.reset_timings()
        e.predict_with(users[0], *rows[users[0]], want_items, predictor=P)
        t = e.timings()
        assert t["predict_ms"] > 0 and t["prep_ms"] == 0
        answers.append(got)
        e.close()
    for a, b in zip(*answers):  # the handle's k plays no part
        assert pc.bits(a[0]) == pc.bits(b[0]) and pc.bits(a[2]) == pc.bits(b[2])
        _same_pair(a[1], b[1], "k")
    # no additional rows for a fitted user: the Personalized answer on train itself
    q = users[0]
    want, _ = pc.oracle_answers(oracle, train, q, oracle.SIM_COSINE, want_items, [])
    assert pc.bits(answers[0][0][2]) == pc.bits(want)


def test_refusals(kn, syn100k):
    train = pc.syn100k(syn100k)
    q = int(train[0][0])
    P = kn.PRED_PERSONALIZED
    it, rt = np.array([pc.NEW_ITEM], dtype=np.int32), np.array([3.0])

    def status_of(call):
        with pytest.raises(kn.KnncfError) as ex:
            call()
        return ex.value.status

    e = kn.Engine(k=10)
    assert status_of(lambda: e.recommend_with(q, it, rt, 3, predictor=P)) == kn.E_STATE  # before a fit
    e.fit(*train)
    assert len(e.recommend_with(q, it, rt, 3, predictor=P)[0]) == 3
    # the explanations refuse the predictor, as they refuse every predictor but the kNN one
    i32p, f64p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    p = lambda a, t: a.ctypes.data_as(t)
    want = np.array([1, 2], dtype=np.int32)
    raters, sims, devs = np.empty(8, dtype=np.int32), np.empty(8), np.empty(8)
    cnt, sums, preds = np.zeros(2, dtype=np.int32), np.zeros(4), np.zeros(2)
    out = (p(raters, i32p), p(sims, f64p), p(devs, f64p), p(cnt, i32p), p(sums, f64p), p(preds, f64p))
    rows = (p(it, i32p), p(rt, f64p), 1, p(want, i32p), 2)
    us, off, poff, st = np.array([q], dtype=np.int32), np.array([0, 1], dtype=np.int64), np.array([0, 2], dtype=np.int64), np.zeros(1, dtype=np.int32)
    csr = (p(off, i64p), p(it, i32p), p(rt, f64p), 1, p(poff, i64p), p(want, i32p))
    lib = e._lib
    for pred, status in ((P, kn.E_UNSUPPORTED), (kn.PRED_BASELINE, kn.E_UNSUPPORTED), (kn.PRED_KNN, kn.OK)):
        assert lib.knncf_update_explain(e._h, pred, q, *rows, 0, 4, *out) == status
        assert lib.knncf_revise_explain(e._h, pred, q, None, 0, *rows, 0, 4, *out) == status
        assert lib.knncf_update_explain_batch(e._h, pred, p(us, i32p), *csr, 0, 4, *out, p(st, i32p)) == status
        assert lib.knncf_revise_explain_batch(e._h, pred, p(us, i32p), p(np.zeros(2, dtype=np.int64), i64p), None, *csr, 0, 4, *out,
                                              p(st, i32p)) == status
    new = (p(it, i32p), p(rt, f64p), 1, p(want, i32p), 2)
    assert lib.knncf_query_explain(e._h, P, 77_000, *new, 0, 4, *out) == kn.E_UNSUPPORTED
    # every other predictor stays refused by the predict / recommend forms
    ids, vals, c = np.empty(4, dtype=np.int32), np.empty(4), C.c_int32()
    assert lib.knncf_update_recommend(e._h, kn.PRED_BASELINE, q, p(it, i32p), p(rt, f64p), 1, 4, p(ids, i32p), p(vals, f64p), C.byref(c)) == kn.E_UNSUPPORTED
    assert lib.knncf_update_recommend(e._h, P, q, p(it, i32p), p(rt, f64p), 1, 4, p(ids, i32p), p(vals, f64p), C.byref(c)) == kn.OK
    e.close()
    e1 = kn.Engine(k=10, similarity=kn.SIM_ONE)
    e1.fit(*train)
    assert status_of(lambda: e1.recommend_with(q, it, rt, 3, predictor=P)) == kn.E_UNSUPPORTED
    assert status_of(lambda: e1.predict_for_batch([(77_000, it, rt)], [[1]], predictor=P)) == kn.E_UNSUPPORTED
    e1.close()
    es = kn.Engine(k=10, shard_rank=0, shard_count=2)  # a shard handle
    es.fit(*train)
    assert status_of(lambda: es.predict_with(q, it, rt, [1], predictor=P)) == kn.E_UNSUPPORTED
    assert status_of(lambda: es.recommend_revised_batch([(q, [], it, rt)], 3, predictor=P)) == kn.E_UNSUPPORTED
    es.close()
