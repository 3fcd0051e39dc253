"""knncf_query_recommend_explain* / knncf_update_recommend_explain* / knncf_revise_recommend_explain* (csrc/foldin.hip
k_qb_reco_rows in front of k_qb_explain / k_qb_explain_all): the top n of a query and the terms behind each, from one pass.

Expected values come from the CPU oracle directly (test 1) and from the two existing calls on the same engine — recommend, then
explain with pred_items = the recommended items (tests 2 to 5).  tests/test_recommend_explain_premises.py proves from the oracle
alone that the inputs (tests/recommend_explain_cases.py) have the counts claimed here.  Every comparison is == on int32 cells
and on fp64 bit patterns, and the raw calls write into sentinel-filled outputs: a cell is the two calls' value or the
sentinel."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import query_explain_cases as qc
from tests import recommend_explain_cases as cases
from tests import revise_cases as rc
from tests.explain_model import BY_WEIGHT, SUM_ORDER

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
SENT_I, SENT_F = -7, 7.5
NAMES = ("items", "preds", "counts", "raters", "sims", "devs", "term_counts", "sums", "statuses")
i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def engines(kn, syn100k):
    """(train name, similarity name) -> (engine, train), made on first use: "dense64" / "dense257" (k = every train user),
    "small" (the hand set, k = 5), "syn100k" (k = 40)"""
    made = {}
    sims = {"cosine": kn.SIM_COSINE, "jaccard": kn.SIM_JACCARD}

    def get(name, sim="cosine"):
        if (name, sim) not in made:
            if name.startswith("dense"):
                train = cases.dense_train(int(name[5:]))
                k = qc.dense_k(int(name[5:]))
            elif name == "small":
                train, k = rc.small_set(), 5
            else:
                train, k = rc.syn100k(syn100k), 40
            made[name, sim] = (kn.Engine(k=k, similarity=sims[sim]).fit(*train), train)
        return made[name, sim]

    yield get
    for e, _ in made.values():
        e.close()


def _view(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_same(got, want, what, names=NAMES):
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape and np.array_equal(_view(g), _view(w)), (what, name)


def _sentinels(B, n, cap):
    rows = B * n
    return [np.full((B, n), SENT_I, dtype=np.int32), np.full((B, n), SENT_F), np.full(B, SENT_I, dtype=np.int32),
            np.full((rows, cap), SENT_I, dtype=np.int32), np.full((rows, cap), SENT_F), np.full((rows, cap), SENT_F),
            np.full(rows, SENT_I, dtype=np.int32), np.full((rows, 2), SENT_F), np.full(B, SENT_I, dtype=np.int32)]


def _ptr(a, t):
    return a.ctypes.data_as(t) if a.size else None


def _raw(e, fam, queries, n, cap, order, predictor, null=()):
    """knncf_<fam>_recommend_explain_batch through the C ABI on sentinel-filled outputs: (status, the nine arrays of NAMES);
    `null` names the outputs passed as null pointers"""
    qargs, keep = e._batch_args(fam, [cases.as_family(fam, q) for q in queries])
    out = _sentinels(len(queries), max(n, 0), max(cap, 0))
    types = (i32p, f64p, i32p, i32p, f64p, f64p, i32p, f64p, i32p)
    ptrs = [None if name in null else _ptr(a, t) for name, a, t in zip(NAMES, out, types)]
    status = getattr(e._lib, f"knncf_{fam}_recommend_explain_batch")(e._h, predictor, *qargs, n, order, cap, *ptrs)
    return status, out


def _raw_single(e, fam, query, n, cap, order, predictor):
    """the single form on sentinel-filled outputs: (status, the first eight arrays of NAMES, as a batch of one shapes them)"""
    q, removed, items, ratings = query
    out = _sentinels(1, n, cap)[:-1]
    types = (i32p, f64p, i32p, i32p, f64p, f64p, i32p, f64p)
    rm = (_ptr(removed, i32p), len(removed)) if fam == "revise" else ()
    it, rt = np.ascontiguousarray(items, dtype=np.int32), np.ascontiguousarray(ratings, dtype=np.float64)
    status = getattr(e._lib, f"knncf_{fam}_recommend_explain")(e._h, predictor, int(q), *rm, _ptr(it, i32p), _ptr(rt, f64p), len(it), n, order,
                                                              cap, *[_ptr(a, t) for a, t in zip(out, types)])
    return status, out


def _two_calls(e, fam, queries, n, cap, order, predictor, null=()):
    """what the fused call must leave in sentinel-filled outputs, from <fam>_recommend_batch and then <fam>_explain_batch (or
    _explain_personalized_batch) with pred_items = the recommended items"""
    qs = [cases.as_family(fam, q) for q in queries]
    reco, st = e._recommend_qb(fam, qs, n, predictor)
    expl, st2 = e._explain_qb(fam, qs, [r[0] for r in reco], cap, order, predictor)
    assert st.tolist() == st2.tolist()
    out = _sentinels(len(qs), n, cap)
    ids, preds, counts, raters, sims, devs, term_counts, sums, statuses = out
    statuses[:] = st
    for b, ((items_b, preds_b), terms_b) in enumerate(zip(reco, expl)):
        c = len(items_b)
        counts[b] = c
        ids[b, :c], preds[b, :c] = items_b, preds_b
        assert np.array_equal(_view(terms_b[5]), _view(preds_b)), b  # the explained prediction is the recommended one
        for j in range(c):
            r, t = b * n + j, min(int(terms_b[3][j]), cap)
            term_counts[r] = terms_b[3][j]
            if "sums" not in null:
                sums[r] = terms_b[4][j]
            raters[r, :t], sims[r, :t], devs[r, :t] = terms_b[0][j, :t], terms_b[1][j, :t], terms_b[2][j, :t]
    return out


def _predictor(kn, name):
    return {"knn": kn.PRED_KNN, "personalized": kn.PRED_PERSONALIZED}[name]


# ---- 1. against the oracle directly ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.DENSE_SIZES)
def test_dense_rows_against_the_oracle(engines, oracle, n):
    e, train = engines(f"dense{n}")
    for name, query in cases.dense_queries(train).items():
        tm = qc.term_model(oracle, f"dense{n}", train, query, oracle.SIM_COSINE, qc.dense_k(n))
        items, preds = tm.pipeline.recommend(query[0], cases.N_RECO)
        rows = tm.rows([query[0]] * len(items), items)
        call = e.recommend_explain_for if name == "fold_in" else e.recommend_explain_with
        for order in (SUM_ORDER, BY_WEIGHT):
            for cap in (8, 64):  # 8 truncates rows, 64 none
                got = call(query[0], query[2], query[3], cases.N_RECO, cap, order=order)
                assert got[0].tolist() == items.tolist() and np.array_equal(_view(got[1]), _view(preds)), (name, order, cap)
                _assert_same(got[2:], qc.expected(rows, cap, order)[:5], (name, order, cap), NAMES[3:8])


# ---- 2. against the two existing calls: the families, both predictors, both similarities ----------------------------------------
@pytest.mark.parametrize("predictor", ["knn", "personalized"])
@pytest.mark.parametrize("sim", ["cosine", "jaccard"])
@pytest.mark.parametrize("data", ["small", "syn100k"])
def test_families_against_recommend_then_explain(kn, engines, data, sim, predictor):
    e, train = engines(data, sim)
    queries = cases.small_cases()[1] if data == "small" else cases.syn_cases(train)
    groups = cases.by_family(train, queries)
    assert set(groups) == ({"revise"} if data == "small" else {"query", "update", "revise"})
    pred = _predictor(kn, predictor)
    beyond = e.num_items + 5
    for n, cap, order, null in ((3, 16, BY_WEIGHT, ()), (cases.N_RECO, 8, SUM_ORDER, ()), (0, 4, SUM_ORDER, ()),
                                (beyond, 0, SUM_ORDER, ("raters", "sims", "devs", "sums"))):
        for fam, at in groups.items():
            qs = [queries[j] for j in at]
            status, got = _raw(e, fam, qs, n, cap, order, pred, null)
            assert status == kn.OK, (fam, n)
            _assert_same(got, _two_calls(e, fam, qs, n, cap, order, pred, null), (data, sim, predictor, fam, n))
            counts = got[2]
            assert (got[8] == kn.OK).all() and (counts == 0).all() == (n == 0)
            if data == "small" and n == cases.N_RECO:
                assert counts.tolist() == [27, 27, 26, 29, 18, 18, 19]  # different counts in one chunk, below the widest
            if n == beyond:
                assert (counts < n).all() and (counts > 0).all()


# ---- 3. 64 + 1 queries per chunk: an empty, a short and a refused slot inside ------------------------------------------------------
@pytest.fixture(scope="module")
def dense_batch():
    return cases.dense_batch()


@pytest.mark.parametrize("predictor", ["knn", "personalized"])
@pytest.mark.parametrize("n,cap,order", [(3, 16, BY_WEIGHT), (cases.N_RECO, 64, SUM_ORDER)])
def test_a_batch_of_65_with_empty_short_and_refused_slots(kn, engines, dense_batch, predictor, n, cap, order):
    e, train = engines("dense257")
    pred = _predictor(kn, predictor)
    status, got = _raw(e, "query", dense_batch, n, cap, order, pred)
    assert status == kn.OK
    _assert_same(got, _two_calls(e, "query", dense_batch, n, cap, order, pred), (predictor, n))
    ids, preds, counts, raters, sims, devs, term_counts, sums, st = got
    assert st[cases.BATCH_REFUSED] == kn.E_DUPLICATE and (np.delete(st, cases.BATCH_REFUSED) == kn.OK).all()
    assert counts[cases.BATCH_REFUSED] == 0 and counts[cases.BATCH_EMPTY] == 0 and counts[cases.BATCH_SHORT] == 2
    for b in (cases.BATCH_REFUSED, cases.BATCH_EMPTY):  # no cell of the row, no explain cell of its rows
        rows = slice(b * n, (b + 1) * n)
        assert (ids[b] == SENT_I).all() and (preds[b] == SENT_F).all() and (term_counts[rows] == SENT_I).all()
        assert (raters[rows] == SENT_I).all() and (sims[rows] == SENT_F).all() and (devs[rows] == SENT_F).all() and (sums[rows] == SENT_F).all()
    b = cases.BATCH_SHORT
    assert (ids[b, 2:] == SENT_I).all() and (term_counts[b * n + 2:(b + 1) * n] == SENT_I).all() and (term_counts[b * n:b * n + 2] > 0).all()
    assert "query " + str(cases.BATCH_REFUSED) in e._lib.knncf_last_error(e._h).decode()


# ---- 4. small workspaces: the results depend on neither C nor R ------------------------------------------------------------------
@pytest.mark.parametrize("predictor", ["knn", "personalized"])
@pytest.mark.parametrize("chunk", sorted(cases.WORKSPACES))
def test_small_workspaces_give_the_default_budgets_bits(kn, engines, dense_batch, monkeypatch, capfd, chunk, predictor):
    e, train = engines("dense257")
    pred = _predictor(kn, predictor)
    n, cap, order = cases.N_RECO, 64, BY_WEIGHT
    status, want = _raw(e, "query", dense_batch, n, cap, order, pred)
    workspace = cases.WORKSPACES[chunk]
    small = kn.Engine(k=qc.dense_k(257), workspace_bytes=workspace).fit(*train)
    assert cases.chunk_of(workspace, small.num_users, small.num_items) == chunk
    R = cases.sub_range_of(workspace, cap, predictor == "personalized")
    monkeypatch.setenv(TRACE, "1")
    capfd.readouterr()
    status, got = _raw(small, "query", dense_batch, n, cap, order, pred)
    lines = [ln[len("knncf-dispatch "):] for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch qb_")]
    monkeypatch.delenv(TRACE)
    assert status == kn.OK
    _assert_same(got, want, (chunk, predictor))
    per_chunk = [int(want[2][c:c + chunk].sum()) for c in range(0, 65, chunk)]
    if chunk == 2:
        assert R == (15 if predictor == "personalized" else 31) and max(per_chunk) == 66  # cuts inside a query's 33 rows and across slots
    kernel = "qb_explain_all " if predictor == "personalized" else "qb_explain "
    assert sum(ln.startswith(kernel) for ln in lines) == sum(-(-m // R) for m in per_chunk)
    assert sum(ln.startswith("qb_reco_rows ") for ln in lines) == sum(m > 0 for m in per_chunk)
    small.close()


# ---- 5. single forms ------------------------------------------------------------------------------------------------------------
def _single_cases(train):
    """family -> query on the dense train: the fold-in user, a fitted user with one more item, a fitted user without one of its items"""
    u = int(np.unique(train[0])[3])
    mine = train[1][train[0] == u].astype(np.int32)
    both = cases.dense_queries(train)
    return {"query": both["fold_in"], "update": both["update"], "revise": (u, mine[-1:].copy(), cases.NONE_I, cases.NONE_R)}


@pytest.mark.parametrize("predictor", ["knn", "personalized"])
@pytest.mark.parametrize("fam", ["query", "update", "revise"])
def test_single_forms_are_the_batch_of_one(kn, engines, fam, predictor):
    e, train = engines("dense64")
    pred = _predictor(kn, predictor)
    query = _single_cases(train)[fam]
    for n, cap, order in ((cases.N_RECO, 8, BY_WEIGHT), (3, 64, SUM_ORDER), (0, 4, SUM_ORDER)):
        status, want = _raw(e, fam, [query], n, cap, order, pred)
        assert status == kn.OK and want[8].tolist() == [kn.OK] and want[2][0] == min(n, 33 if fam == "query" else 32 if fam == "update" else 34)
        status, got = _raw_single(e, fam, query, n, cap, order, pred)
        assert status == kn.OK
        _assert_same(got, want[:8], (fam, predictor, n))
    # a per-query refusal is the call's status: *count = 0 and nothing else is written
    q, removed, items, ratings = query
    twice = (q, removed, np.array([7, 9, 7], dtype=np.int32), np.array([4.0, 2.0, 3.0]))
    status, got = _raw_single(e, fam, twice, 3, 4, SUM_ORDER, pred)
    assert status == kn.E_DUPLICATE and got[2].tolist() == [0]
    want = _sentinels(1, 3, 4)[:-1]
    want[2][:] = 0
    _assert_same(got, want, (fam, "refused"))
    # the wrappers cut to the count
    call = {"query": e.recommend_explain_for, "update": e.recommend_explain_with}.get(fam)
    answer = call(q, items, ratings, 3, 64, predictor=pred) if call else e.recommend_explain_revised(q, removed, items, ratings, 3, 64, predictor=pred)
    status, want = _raw(e, fam, [query], 3, 64, SUM_ORDER, pred)
    assert answer[0].tolist() == want[0][0].tolist() and np.array_equal(_view(answer[1]), _view(want[1][0]))
    assert answer[5].tolist() == want[6].tolist() and np.array_equal(_view(answer[6]), _view(want[7]))
    live = np.arange(64)[None, :] < np.minimum(want[6], 64)[:, None]
    assert np.array_equal(answer[2][live], want[3][live]) and (answer[2][~live] == -1).all() and np.isnan(answer[3][~live]).all()
    assert np.array_equal(_view(answer[3][live]), _view(want[4][live])) and np.array_equal(_view(answer[4][live]), _view(want[5][live]))


# ---- 6. dispatch traces ---------------------------------------------------------------------------------------------------------
def _qb_lines(capfd):
    return [ln[len("knncf-dispatch "):] for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch qb_")]


def test_dispatch_of_a_fused_knn_call(kn, engines, dense_batch, monkeypatch, capfd):
    e, _ = engines("dense257")
    monkeypatch.setenv(TRACE, "1")
    for order in (SUM_ORDER, BY_WEIGHT):
        capfd.readouterr()
        status, got = _raw(e, "query", dense_batch, 3, 16, order, kn.PRED_KNN)
        rows = int(got[2][:64].sum())
        assert rows == 61 * 3 + 2
        assert _qb_lines(capfd) == [f"qb_reco_rows C=64 n=3 rows={rows}", f"qb_explain order={order}",
                                    "qb_reco_rows C=1 n=3 rows=3", f"qb_explain order={order}"]


def test_dispatch_of_a_fused_personalized_call_folds_once_per_chunk(kn, engines, dense_batch, monkeypatch, capfd):
    e, _ = engines("dense257")
    qs = [cases.as_family("query", q) for q in dense_batch]
    e.recommend_for_batch(qs[:1], 3, predictor=kn.PRED_PERSONALIZED)  # (the rater copies of the first Personalized call)
    monkeypatch.setenv(TRACE, "1")
    capfd.readouterr()
    status, got = _raw(e, "query", dense_batch, 3, 16, BY_WEIGHT, kn.PRED_PERSONALIZED)
    assert _qb_lines(capfd) == ["qb_fold_all stride=64", "qb_reco_rows C=64 n=3 rows=185", f"qb_explain_all order={BY_WEIGHT} cap=16 rows=185",
                                "qb_fold_all stride=1", "qb_reco_rows C=1 n=3 rows=3", f"qb_explain_all order={BY_WEIGHT} cap=16 rows=3"]
    reco, _ = e.recommend_for_batch(qs, 3, predictor=kn.PRED_PERSONALIZED)
    e.explain_for_batch(qs, [r[0] for r in reco], 16, order=BY_WEIGHT, predictor=kn.PRED_PERSONALIZED)
    lines = _qb_lines(capfd)
    assert [ln for ln in lines if ln.startswith("qb_fold_all")] == ["qb_fold_all stride=64", "qb_fold_all stride=1"] * 2  # two per chunk
    assert not any(ln.startswith("qb_reco_rows") for ln in lines)


# ---- 7. handle state and statuses -----------------------------------------------------------------------------------------------
def test_read_only_on_the_handle_and_repeatable(kn, tmp_path):
    train = cases.dense_train(64)
    e = kn.Engine(k=10).fit(*train)
    stored = e.neighbors(int(train[0][-1]))  # something in the table
    e.neighbors_save(str(tmp_path / "before.bin"))
    queries = cases.dense_batch()[:12]
    first = {}
    for pred in (kn.PRED_KNN, kn.PRED_PERSONALIZED):
        status, first[pred] = _raw(e, "query", queries, 5, 16, BY_WEIGHT, pred)
        assert status == kn.OK
    for pred in (kn.PRED_KNN, kn.PRED_PERSONALIZED):
        status, again = _raw(e, "query", queries, 5, 16, BY_WEIGHT, pred)
        _assert_same(again, first[pred], pred)
    e.neighbors_save(str(tmp_path / "after.bin"))
    assert (tmp_path / "before.bin").read_bytes() == (tmp_path / "after.bin").read_bytes()
    again = e.neighbors(int(train[0][-1]))
    assert again[0].tolist() == stored[0].tolist() and np.array_equal(_view(again[1]), _view(stored[1]))
    e.close()


def test_handle_level_statuses_and_argument_refusals(kn):
    train = cases.dense_train(64)
    queries = cases.dense_batch()[:3]

    def refused(e, status, n=3, cap=4, order=SUM_ORDER, pred=kn.PRED_KNN, null=()):
        res, out = _raw(e, "query", queries, n, cap, order, pred, null)
        assert res == status, (status, n, cap, order, pred, null)
        _assert_same(out, _sentinels(3, max(n, 0), max(cap, 0)), (status, n, cap, order, pred, null))  # nothing is written
        if not null and n >= 0 and cap >= 0:
            res, out = _raw_single(e, "query", queries[0], n, cap, order, pred)
            want = _sentinels(1, n, cap)[:-1]
            want[2][:] = 0  # a single form has set *count = 0
            assert res == status
            _assert_same(out, want, ("single", status, n, cap, order, pred))

    fresh = kn.Engine(k=10)
    refused(fresh, kn.E_STATE)
    fresh.close()
    one = kn.Engine(k=10, similarity=kn.SIM_ONE).fit(*train)
    refused(one, kn.E_UNSUPPORTED)
    one.close()
    shard = kn.Engine(k=10, shard_rank=0, shard_count=2).fit(*train)
    refused(shard, kn.E_UNSUPPORTED)
    shard.close()
    four = np.isin(train[0], np.unique(train[0])[:4])
    few = kn.Engine(k=10).fit(train[0][four], train[1][four], train[2][four])
    assert few.num_users == 4
    refused(few, kn.E_UNSUPPORTED)
    few.close()
    e = kn.Engine(k=10).fit(*train)
    for pred in (0, 4, 7):
        refused(e, kn.E_UNSUPPORTED, pred=pred)
    refused(e, kn.E_INVALID, cap=-1)
    refused(e, kn.E_INVALID, n=-1)
    refused(e, kn.E_INVALID, order=2)
    refused(e, kn.E_INVALID, order=-1)
    refused(e, kn.E_INVALID, null=("term_counts",))
    for name in ("raters", "sims", "devs", "items", "preds", "counts", "statuses"):
        refused(e, kn.E_INVALID, null=(name,))
    # what may be null: sums; the term arrays with cap == 0; everything but counts and statuses with n == 0
    status, want = _raw(e, "query", queries, 3, 4, SUM_ORDER, kn.PRED_KNN)
    status, got = _raw(e, "query", queries, 3, 4, SUM_ORDER, kn.PRED_KNN, null=("sums",))
    assert status == kn.OK and (got[7] == SENT_F).all()
    _assert_same(got[:7], want[:7], "null sums")
    status, got = _raw(e, "query", queries, 3, 0, SUM_ORDER, kn.PRED_KNN, null=("raters", "sims", "devs", "sums"))
    assert status == kn.OK and np.array_equal(got[6], want[6]) and np.array_equal(got[0], want[0])
    status, got = _raw(e, "query", queries, 0, 4, SUM_ORDER, kn.PRED_KNN, null=("items", "preds", "raters", "sims", "devs", "term_counts", "sums"))
    assert status == kn.OK and got[2].tolist() == [0, 0, 0] and got[8].tolist() == [kn.OK] * 3
    assert e._lib.knncf_query_recommend_explain_batch(e._h, kn.PRED_KNN, None, None, None, None, 0, 3, SUM_ORDER, 4, *[None] * 9) == kn.OK
    e.close()
