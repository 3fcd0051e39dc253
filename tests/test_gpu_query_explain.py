"""knncf_query_explain* / knncf_update_explain* / knncf_revise_explain* (csrc/foldin.hip k_qb_explain): the neighbour terms
behind fold-in, update and revise predictions, bit for bit.

The expected terms come from tests/explain_model.TermModel on aug = train without the user's removed rows ++ the additional
rows, on a fresh pipeline whose first call is the query user's neighbourhood (tests/query_explain_cases.py);
tests/test_query_explain_premises.py proves from the oracle alone that the inputs have the term counts, ties and
zero-similarity neighbours claimed here.  Every comparison is == on int32 ids and on fp64 bit patterns.  The engines are shared
by the tests of this file: the query calls are read-only on the handle (test 6)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import explain_model
from tests import query_explain_cases as qc
from tests import revise_cases as rc
from tests.explain_model import BY_WEIGHT, SUM_ORDER

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
SENT_I, SENT_F = -7, 7.5
NAMES = ("raters", "sims", "devs", "counts", "sums", "predictions")
i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def engines(kn, oracle, syn100k):
    """(similarity name, k) -> (engine fitted on syn-100k, the oracle's similarity kind), made on first use"""
    made = {}
    kinds = {"cosine": (kn.SIM_COSINE, oracle.SIM_COSINE), "jaccard": (kn.SIM_JACCARD, oracle.SIM_JACCARD)}

    def get(sim_name, k):
        if (sim_name, k) not in made:
            made[sim_name, k] = kn.Engine(k=k, similarity=kinds[sim_name][0]).fit(*rc.syn100k(syn100k))
        return made[sim_name, k], kinds[sim_name][1]

    yield get
    for e in made.values():
        e.close()


def _view(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and np.array_equal(_view(g), _view(w)), (what, name)


def _explain(e, query, pred_items, cap, order):
    """the single call of the query's family: fold-in for a user train does not hold, revise with removals, update otherwise"""
    q, removed, items, ratings = query
    if len(removed):
        return e.explain_revised(q, removed, items, ratings, pred_items, cap, order=order)
    if q in qc.ABSENT_USERS or q == qc.DENSE_USER:
        return e.explain_for(q, items, ratings, pred_items, cap, order=order)
    return e.explain_with(q, items, ratings, pred_items, cap, order=order)


def _predict(e, query, pred_items):
    q, removed, items, ratings = query
    if len(removed):
        return e.predict_revised(q, removed, items, ratings, pred_items)
    if q in qc.ABSENT_USERS or q == qc.DENSE_USER:
        return e.predict_for(q, items, ratings, pred_items)
    return e.predict_with(q, items, ratings, pred_items)


def _callers_fold(sims, devs, counts):
    """the caller's left fold of the returned terms, column by column (separate multiply and add: no FMA)"""
    num, den = np.zeros(len(counts)), np.zeros(len(counts))
    for c in range(sims.shape[1]):
        live = c < counts
        s, d = np.where(live, sims[:, c], 0.0), np.where(live, devs[:, c], 0.0)
        num = np.where(live, num + d * s, num)
        den = np.where(live, den + np.abs(s), den)
    return np.stack([num, den], axis=1)


def _check_query(e, oracle, tag, train, query, osim, k, pred_items, caps, what):
    """both orders at every cap against the model; predictions against the predict call; the caller's fold"""
    tm = qc.term_model(oracle, tag, train, query, osim, k)
    rows = [tm.row(query[0], int(i)) for i in pred_items]
    predicted = _predict(e, query, pred_items)
    for cap in caps:
        for order in (SUM_ORDER, BY_WEIGHT):
            got = _explain(e, query, pred_items, cap, order)
            _assert_same(got, qc.expected(rows, cap, order), (what, cap, order))
            assert np.array_equal(_view(got[5]), _view(predicted)), (what, cap, order)
            if order == SUM_ORDER and (got[3] <= cap).all():
                assert np.array_equal(_view(_callers_fold(got[1], got[2], got[3])), _view(got[4])), (what, cap)
    return rows


# ---- 1. syn-100k against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [300, 10])
@pytest.mark.parametrize("which", range(13))
def test_fitted_users_syn100k_cosine(engines, oracle, syn100k, which, k):
    train = rc.syn100k(syn100k)
    q = rc.pick_users(train)[which]
    e, osim = engines("cosine", k)
    for name, query in qc.syn_queries(train, q).items():
        pred_items = rc.pred_items(train, q, query[1], query[2])
        rows = _check_query(e, oracle, "syn100k", train, query, osim, k, pred_items, (16, 256), (q, name, k))
        counts = np.array([r.count for r in rows])
        assert (counts == 0).any() and counts.max() <= 256, (q, name)  # cap = 256 truncates nothing ...
        assert k == 10 or name != "mixed" or (counts > 16).sum() >= 200, q  # ... and cap = 16 hundreds of rows


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("k", [300, 10])
def test_absent_users_syn100k_cosine(engines, oracle, syn100k, k, n):
    train = rc.syn100k(syn100k)
    query = qc.absent_query(train, n)
    assert query[0] not in set(train[0].tolist())
    e, osim = engines("cosine", k)
    pred_items = rc.pred_items(train, query[0], query[1], query[2])
    _check_query(e, oracle, "syn100k", train, query, osim, k, pred_items, (16, 256), (query[0], k))


def test_fitted_users_syn100k_jaccard(engines, oracle, syn100k):
    train = rc.syn100k(syn100k)
    e, osim = engines("jaccard", 50)
    for q in rc.pick_users(train)[:3]:
        query = qc.syn_queries(train, q)["mixed"]
        _check_query(e, oracle, "syn100k", train, query, osim, 50, rc.pred_items(train, q, query[1], query[2]), (16, 256), q)


# ---- 2. window edges: 64-entry trips of the walk, the 256 terms of one BY_WEIGHT pass, ties ---------------------------------------
@pytest.mark.parametrize("n", qc.DENSE_SIZES)
def test_window_edges_on_the_dense_train(kn, oracle, n):
    train = explain_model.dense_train(n, qc.DENSE_SEED)
    k = qc.dense_k(n)
    e = kn.Engine(k=k).fit(*train)
    rows = _check_query(e, oracle, f"dense{n}", train, qc.dense_query(), oracle.SIM_COSINE, k, qc.DENSE_ITEMS, (n, 5), n)
    assert rows[0].count == n and rows[-1].count == 0
    if n == 131:
        mags = np.abs(rows[0].terms(BY_WEIGHT)[1])
        assert (mags[:-1] == mags[1:]).any()  # ties, placed by summation order (Row.by_weight)
        up = qc.dense_update(train)
        rows = _check_query(e, oracle, "dense131", train, up, oracle.SIM_COSINE, k, qc.DENSE_ITEMS, (n, 5), "update")
        assert rows[0].count == 130 and up[0] not in rows[0].raters.tolist()
    e.close()


# ---- 3. zero-similarity neighbours ----------------------------------------------------------------------------------------------
def test_zero_similarity_neighbours_are_listed_and_are_no_terms(kn, oracle):
    case = explain_model.disjoint_case()
    train = case.train
    query = qc.disjoint_query(case)
    cold, private = qc.cold_private_item(case)
    background = np.unique(train[1][train[1] <= 120]).astype(np.int32)
    pred_items = np.concatenate([[private], background]).astype(np.int32)
    e = kn.Engine(k=qc.DISJOINT_K).fit(*train)
    _check_query(e, oracle, "disjoint", train, query, oracle.SIM_COSINE, qc.DISJOINT_K, pred_items, (160, 5), "disjoint")
    raters, sims, devs, counts, sums, preds = e.explain_for(query[0], query[2], query[3], pred_items, 160)
    ids, nsims = e.neighbors_for(query[0], query[2], query[3])
    assert len(ids) == 160 and cold in ids.tolist() and (nsims == 0.0).sum() == 62
    mean = e.predict_for(query[0], query[2], query[3], [qc.ABSENT_ITEM])[0]
    assert counts[0] == 0 and sums[0].tolist() == [0.0, 0.0] and _view(preds[:1])[0] == _view(np.array([mean]))[0]
    listed = np.array([np.isin(train[0][train[1] == i], ids).sum() for i in background])
    assert (counts[1:] <= listed).all() and (listed - counts[1:]).max() == 27
    zero = set(ids[nsims == 0.0].tolist())
    assert not zero & set(raters[raters >= 0].tolist())
    e.close()


# ---- 4. row kinds on the hand set -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lone_item_removed", "lone_item_rerated", "all_removed", "into_small_a", "into_small_b", "long_row_mixed"])
def test_row_kinds_on_the_hand_set(kn, oracle, name):
    train = rc.small_set()
    query = rc.small_queries(train)[name]
    q, removed, items, ratings = query
    aug = rc.aug_of(train, *query)
    own = aug[1][aug[0] == q]
    pred_items = np.concatenate([np.arange(1, 32), own, [rc.UNKNOWN_ITEM]]).astype(np.int32)
    e = kn.Engine(k=10).fit(*train)
    rows = _check_query(e, oracle, "small", train, query, oracle.SIM_COSINE, 10, pred_items, (40, 2), name)
    got = e.explain_revised(q, removed, items, ratings, pred_items, 40)
    mean = e.predict_revised(q, removed, items, ratings, [rc.UNKNOWN_ITEM])
    assert got[3][-1] == 0 and got[4][-1].tolist() == [0.0, 0.0] and _view(got[5][-1:])[0] == _view(mean)[0]  # an unknown id
    assert q not in got[0].reshape(-1).tolist()  # never its own term, the rows on its own items included
    assert sum(rows[31 + j].count for j in range(len(own))) > 0
    if name == "lone_item_removed":  # the item has left aug
        at = rc.LONE_ITEM - 1
        assert got[3][at] == 0 and got[4][at].tolist() == [0.0, 0.0] and _view(got[5][at:at + 1])[0] == _view(mean)[0]
    if name in ("all_removed", "into_small_a", "into_small_b"):
        assert len(own) <= 4
    e.close()


# ---- 5. batches -----------------------------------------------------------------------------------------------------------------
def _raw_batch(kn, e, queries, pred_items, cap, order, null_terms=False, null_sums=False):
    """knncf_revise_explain_batch through the C ABI on sentinel-filled outputs: (status, outputs ..., statuses)"""
    qargs, keep = e._batch_args("revise", queries)
    poff = np.zeros(len(queries) + 1, dtype=np.int64)
    poff[1:] = np.cumsum([len(x) for x in pred_items])
    pi = np.ascontiguousarray(np.concatenate(pred_items), dtype=np.int32)
    m = int(poff[-1])
    w = max(cap, 0)
    raters = np.full((m, w), SENT_I, dtype=np.int32)
    sims, devs = np.full((m, w), SENT_F), np.full((m, w), SENT_F)
    counts = np.full(m, SENT_I, dtype=np.int32)
    sums, preds = np.full((m, 2), SENT_F), np.full(m, SENT_F)
    st = np.full(len(queries), SENT_I, dtype=np.int32)
    p = lambda a, t: a.ctypes.data_as(t) if a.size else None
    terms = (None, None, None) if null_terms else (p(raters, i32p), p(sims, f64p), p(devs, f64p))
    status = e._lib.knncf_revise_explain_batch(e._h, kn.PRED_KNN, *qargs, p(poff, i64p), p(pi, i32p), order, cap, *terms, p(counts, i32p),
                                               None if null_sums else p(sums, f64p), None if null_sums else p(preds, f64p), p(st, i32p))
    return status, (raters, sims, devs, counts, sums, preds), st, poff


@pytest.fixture(scope="module")
def batch100k(syn100k):
    """41 queries of all three kinds as revise queries (user, removed, items, ratings), and the requested items of each"""
    train = rc.syn100k(syn100k)
    queries = [query for q in rc.pick_users(train) for query in qc.syn_queries(train, q).values()]
    queries += [qc.absent_query(train, n) for n in (0, 1)]
    pred_items = [rc.pred_items(train, q, removed, items)[::7] for q, removed, items, _ in queries]
    return train, queries, pred_items


@pytest.fixture(scope="module")
def singles100k(engines, batch100k):
    """(cap, order) -> the single call's answer for each of the 41 queries"""
    e, _ = engines("cosine", 300)
    _, queries, pred_items = batch100k
    return {(cap, order): [_explain(e, query, pi, cap, order) for query, pi in zip(queries, pred_items)]
            for cap, order in ((16, SUM_ORDER), (16, BY_WEIGHT), (256, BY_WEIGHT))}


def _bad_query(train):
    """a removal of an item the user did not rate: KNNCF_E_INVALID for that query alone"""
    q = rc.pick_users(train)[0]
    free = np.setdiff1d(np.unique(train[1]), train[1][train[0] == q])[:1].astype(np.int32)
    return q, free, qc.NONE_I, qc.NONE_R


@pytest.mark.parametrize("cap,order", [(16, SUM_ORDER), (16, BY_WEIGHT)])
@pytest.mark.parametrize("size", [72, 40, 5])
def test_batches_mix_the_families_and_equal_the_single_calls(kn, engines, batch100k, singles100k, monkeypatch, capfd, size, cap, order):
    """72 queries: a chunk of 64 and one of 8; 40: one chunk of at least 32 answerable queries (every train row read once for
    the chunk); 5: fewer (one similarity pass per query).  One failed query sits in the middle."""
    train, queries, pred_items = batch100k
    e, _ = engines("cosine", 300)
    pick = [j % len(queries) for j in range(size)]
    bad = size // 2
    qs = [queries[j] for j in pick]
    pis = [pred_items[j] for j in pick]
    qs[bad], pick[bad] = _bad_query(train), None
    monkeypatch.setenv(TRACE, "1")
    capfd.readouterr()
    answers, st = e.explain_revised_batch(qs, pis, cap, order=order)
    launches = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch qb_explain")]
    assert launches == [f"knncf-dispatch qb_explain order={order}"] * (-(-size // 64))  # one launch per chunk
    assert st.tolist() == [kn.OK if j is not None else kn.E_INVALID for j in pick]
    for b, j in enumerate(pick):
        if j is not None:
            _assert_same(answers[b], singles100k[cap, order][j], (size, b))
    failed = answers[bad]  # the wrapper's padding
    assert (failed[3] == 0).all() and (failed[0] == -1).all() and np.isnan(failed[1]).all() and np.isnan(failed[5]).all()
    assert "query " + str(bad) in e._lib.knncf_last_error(e._h).decode()


def test_a_failed_query_leaves_its_rows_untouched(kn, engines, batch100k, singles100k):
    train, queries, pred_items = batch100k
    e, _ = engines("cosine", 300)
    qs, pis = [queries[0], _bad_query(train), queries[1]], [pred_items[0], pred_items[3], pred_items[1]]
    for cap, order in ((16, SUM_ORDER), (256, BY_WEIGHT)):
        status, out, st, poff = _raw_batch(kn, e, qs, pis, cap, order)
        assert status == kn.OK and st.tolist() == [kn.OK, kn.E_INVALID, kn.OK]
        lo, hi = int(poff[1]), int(poff[2])
        assert (out[3][lo:hi] == 0).all()
        for a in (out[0], out[1], out[2], out[4], out[5]):
            assert (a[lo:hi] == (SENT_I if a.dtype == np.int32 else SENT_F)).all()
        for b, j in ((0, 0), (2, 1)):  # the neighbours' answers are the single calls'; the cells beyond the terms keep the sentinel
            want = singles100k[cap, order][j]
            rows = slice(int(poff[b]), int(poff[b + 1]))
            for name, g, w in zip(NAMES[3:], out[3:], want[3:]):
                assert np.array_equal(_view(g[rows]), _view(w)), (name, b)
            beyond = np.arange(cap)[None, :] >= np.minimum(want[3], cap)[:, None]
            assert np.array_equal(out[0][rows][~beyond], want[0][~beyond]) and (out[0][rows][beyond] == SENT_I).all()
            for g, w in ((out[1], want[1]), (out[2], want[2])):
                assert np.array_equal(_view(g[rows][~beyond]), _view(w[~beyond])) and (g[rows][beyond] == SENT_F).all()


def test_row_sub_ranges_of_a_small_workspace(kn, engines, batch100k, singles100k, monkeypatch, capfd):
    train, queries, pred_items = batch100k
    cap, order, workspace = 256, BY_WEIGHT, 8 << 20
    small = kn.Engine(k=300, workspace_bytes=workspace).fit(*train)
    chunk = max(1, min(64, (workspace // 2) // (64 * small.num_users + 96 * small.num_items)))  # the rules of include/knncf.h
    rows = max(1, (workspace // 2) // (20 * cap + 28))
    qs, pis = queries[:30], pred_items[:30]
    per_chunk = [sum(len(x) for x in pis[c:c + chunk]) for c in range(0, len(qs), chunk)]
    assert max(per_chunk) > 2 * rows  # at least three sub-ranges in a chunk
    monkeypatch.setenv(TRACE, "1")
    capfd.readouterr()
    answers, st = small.explain_revised_batch(qs, pis, cap, order=order)
    launches = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch qb_explain")]
    assert len(launches) == sum(-(-m // rows) for m in per_chunk)
    assert (st == kn.OK).all()
    for b in range(len(qs)):
        _assert_same(answers[b], singles100k[cap, order][b], b)  # the default handle's
    small.close()


# ---- 6. read-only; cap == 0 -----------------------------------------------------------------------------------------------------
def test_read_only_on_the_handle_and_cap_zero(kn, syn100k, batch100k, tmp_path):
    train, queries, pred_items = batch100k
    e = kn.Engine(k=40).fit(*train)
    e.neighbors(int(train[0][-1]))  # something in the table
    stored = e.neighbors(queries[0][0])
    e.neighbors_save(str(tmp_path / "before.bin"))
    qs, pis = queries[:6] + queries[-2:], pred_items[:6] + pred_items[-2:]
    with_terms = [_explain(e, query, pi, 40, BY_WEIGHT) for query, pi in zip(qs, pis)]
    e.explain_revised_batch(qs, pis, 40)
    status, out, st, poff = _raw_batch(kn, e, qs, pis, 0, SUM_ORDER, null_terms=True)  # cap == 0: no term arrays needed
    assert status == kn.OK and (st == kn.OK).all()
    for b, want in enumerate(with_terms):
        rows = slice(int(poff[b]), int(poff[b + 1]))
        for g, w in zip(out[3:], want[3:]):
            assert np.array_equal(_view(g[rows]), _view(w)), b
    status, out, st, poff = _raw_batch(kn, e, qs, pis, 0, SUM_ORDER, null_terms=True, null_sums=True)  # sums, predictions: optional
    assert status == kn.OK and np.array_equal(out[3], np.concatenate([w[3] for w in with_terms])) and (out[4] == SENT_F).all()
    for cap, order, null_terms in ((-1, SUM_ORDER, False), (4, 2, False), (4, -1, False), (4, SUM_ORDER, True)):
        status, out, st, poff = _raw_batch(kn, e, qs, pis, cap, order, null_terms=null_terms)  # refused: nothing is written
        assert status == kn.E_INVALID, (cap, order)
        assert all((a == (SENT_I if a.dtype == np.int32 else SENT_F)).all() for a in out) and (st == SENT_I).all()
    e.neighbors_save(str(tmp_path / "after.bin"))
    assert (tmp_path / "before.bin").read_bytes() == (tmp_path / "after.bin").read_bytes()
    again = e.neighbors(queries[0][0])
    assert again[0].tolist() == stored[0].tolist() and np.array_equal(_view(again[1]), _view(stored[1]))
    e.close()
