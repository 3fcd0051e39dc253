"""knncf_explain*: the neighbour terms behind kNN predictions, bit for bit.

The expected terms come from tests/explain_model.py, which derives them from the CPU oracle's neighbour lists, deviations and
the training file (test_explain_model.py shows on the CPU that their fold IS the oracle's wsd and prediction).  Every
comparison is == on int32 ids and on fp64 bit patterns.  Raw calls through the C ABI with sentinel-filled outputs prove which
cells a call writes; KNNCF_DEBUG_TRACE_DISPATCH lines on the library's stderr show which kernel instantiation ran."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import explain_model
from tests.explain_model import BY_WEIGHT, SUM_ORDER
from tests.test_gpu_recommend_batch import _table

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
NO_BITMAPS = "KNNCF_DEBUG_NO_ITEM_BITMAPS"
SETTINGS = [("cosine", 10), ("cosine", 300), ("jaccard", 50)]
SENT_I, SENT_F = -7, 7.5
ABSENT_USER, ABSENT_ITEM = 987_654, 876_543
i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _sims(kn, oracle, name):
    return {"cosine": (kn.SIM_COSINE, oracle.SIM_COSINE), "jaccard": (kn.SIM_JACCARD, oracle.SIM_JACCARD)}[name]


def _train(d):
    return d.train.users, d.train.items, d.train.ratings


def _raw(kn, e, users, items, cap, order=SUM_ORDER, null_terms=False, null_sums=False):
    """knncf_explain_batch through the C ABI on sentinel-filled outputs: (status, raters, sims, devs, counts, sums, preds)"""
    u, i = np.ascontiguousarray(users, dtype=np.int32), np.ascontiguousarray(items, dtype=np.int32)
    n = len(u)
    w = max(cap, 0)
    raters = np.full((n, w), SENT_I, dtype=np.int32)
    sims, devs = np.full((n, w), SENT_F), np.full((n, w), SENT_F)
    counts = np.full(n, SENT_I, dtype=np.int32)
    sums, preds = np.full((n, 2), SENT_F), np.full(n, SENT_F)
    p = lambda a, t: None if a.size == 0 else a.ctypes.data_as(t)
    terms = (None, None, None) if null_terms else (p(raters, i32p), p(sims, f64p), p(devs, f64p))
    st = e._lib.knncf_explain_batch(e._h, p(u, i32p), p(i, i32p), n, order, cap, *terms, p(counts, i32p),
                                    None if null_sums else p(sums, f64p), None if null_sums else p(preds, f64p))
    return st, raters, sims, devs, counts, sums, preds


def _assert_rows(got, want_rows, order, what):
    """the wrapper's result against the model's rows: ids, sims, devs, counts, sums, predictions; padding beyond the terms"""
    raters, sims, devs, counts, sums, preds = got
    cap = raters.shape[1]
    assert counts.tolist() == [r.count for r in want_rows], what
    assert np.array_equal(_bits(sums), _bits([[r.num, r.den] for r in want_rows])), what
    assert np.array_equal(_bits(preds), _bits([r.prediction for r in want_rows])), what
    for j, row in enumerate(want_rows):
        r, s, d = row.terms(order)
        m = min(row.count, cap)
        assert raters[j, :m].tolist() == r[:m].tolist(), (what, j)
        assert np.array_equal(_bits(sims[j, :m]), _bits(s[:m])) and np.array_equal(_bits(devs[j, :m]), _bits(d[:m])), (what, j)
        assert (raters[j, m:] == -1).all() and np.isnan(sims[j, m:]).all() and np.isnan(devs[j, m:]).all(), (what, j)


def _same(a, b):
    return all(np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def _lines(capfd):
    return [ln[len("knncf-dispatch "):] for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch explain")]


# ---- shared, unchanged state --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows100k(syn100k):
    """about 200 rows over 40 users, shuffled, some repeated; one absent user, one absent item, one row on an item of the
    user's own training rows"""
    d = syn100k
    users, counts = np.unique(d.test.users, return_counts=True)
    picked = users[np.argsort(counts, kind="stable")][np.linspace(0, len(users) - 1, 40).astype(int)]
    rng = np.random.default_rng(5)
    at = np.concatenate([rng.permutation(np.flatnonzero(d.test.users == u))[:5] for u in picked])
    u, i = d.test.users[at].astype(np.int32), d.test.items[at].astype(np.int32)
    u = np.concatenate([u, u[:6], [ABSENT_USER, u[0], d.train.users[123]]]).astype(np.int32)
    i = np.concatenate([i, i[:6], [i[0], ABSENT_ITEM, d.train.items[123]]]).astype(np.int32)
    assert ABSENT_USER not in set(d.train.users.tolist()) and ABSENT_ITEM not in set(d.train.items.tolist())
    order = rng.permutation(len(u))
    return u[order], i[order]


@pytest.fixture(scope="module")
def model100k(oracle, syn100k):
    return oracle.Model(*_train(syn100k))


@pytest.fixture(scope="module")
def want100k(oracle, model100k, rows100k):
    """(similarity, k) -> the model's rows of rows100k, computed once in the batch's row order"""
    cache = {}

    def get(sim_name, k, osim):
        if (sim_name, k) not in cache:
            cache[sim_name, k] = explain_model.TermModel(oracle, model100k, osim, k).rows(*rows100k)
        return cache[sim_name, k]

    return get


# ---- 1. against the oracle model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [SUM_ORDER, BY_WEIGHT])
@pytest.mark.parametrize("sim_name,k", SETTINGS)
def test_against_the_oracle_model(kn, oracle, syn100k, rows100k, want100k, sim_name, k, order):
    ksim, osim = _sims(kn, oracle, sim_name)
    want = want100k(sim_name, k, osim)
    assert sum(r.count >= 2 for r in want) >= (150 if k == 300 else 1)
    e = kn.Engine(k=k, similarity=ksim).fit(*_train(syn100k))
    cap = max(r.count for r in want)
    _assert_rows(e.explain_batch(*rows100k, cap, order=order), want, order, (sim_name, k, order))
    # the single call is the batch of one row (cap=None: min(k, U - 1))
    for j in (0, 57, len(want) - 1):
        r, s, d, c, (num, den), pred = e.explain(int(rows100k[0][j]), int(rows100k[1][j]), order=order)
        wr, ws, wd = want[j].terms(order)
        assert c == want[j].count and r.tolist() == wr.tolist() and np.array_equal(_bits(s), _bits(ws)) and np.array_equal(_bits(d), _bits(wd))
        assert np.array_equal(_bits([num, den, pred]), _bits([want[j].num, want[j].den, want[j].prediction]))
    e.close()


# ---- 2. self-consistency on the whole test set ---------------------------------------------------------------------------
def test_fold_and_combine_of_the_whole_test_set(kn, syn100k):
    d = syn100k
    tu = np.concatenate([d.test.users, [ABSENT_USER]]).astype(np.int32)
    ti = np.concatenate([d.test.items, [d.test.items[0]]]).astype(np.int32)
    k = 40
    e, twin = (kn.Engine(k=k).fit(*_train(d)) for _ in range(2))
    raters, sims, devs, counts, sums, preds = e.explain_batch(tu, ti, k)
    assert counts.max() <= k and counts.max() >= 2
    num, den = np.zeros(len(tu)), np.zeros(len(tu))
    for c in range(k):  # the caller's left fold, column by column (separate multiply and add: no FMA)
        live = c < counts
        s, dv = np.where(live, sims[:, c], 0.0), np.where(live, devs[:, c], 0.0)
        num = np.where(live, num + dv * s, num)
        den = np.where(live, den + np.abs(s), den)
    assert np.array_equal(_bits(num), _bits(sums[:, 0])) and np.array_equal(_bits(den), _bits(sums[:, 1]))
    avg = {int(u): e.user_avg(int(u)) for u in np.unique(d.test.users)}
    ua = np.array([avg.get(int(u), -1.0) for u in tu])
    with np.errstate(invalid="ignore", divide="ignore"):
        wsd = np.where(den > 0, num / den, 0.0)
    x = ua + wsd
    scale = np.where(x > ua, 5 - ua, np.where(x < ua, ua - 1, 1.0))
    combined = np.where(ua < 0, e.global_avg(), ua + wsd * scale)
    assert np.array_equal(_bits(combined), _bits(preds))
    assert np.array_equal(_bits(twin.predict_batch(kn.PRED_KNN, tu, ti)), _bits(preds))
    e.close()
    twin.close()


# ---- 3. cap edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [SUM_ORDER, BY_WEIGHT])
def test_cap_edges_leave_the_cells_beyond_the_terms_untouched(kn, oracle, syn100k, rows100k, want100k, order):
    want = want100k("cosine", 300, oracle.SIM_COSINE)
    chosen = next(j for j, r in enumerate(want) if 4 <= r.count <= 40)
    count = want[chosen].count
    e = kn.Engine(k=300).fit(*_train(syn100k))
    ref = None
    for cap in (0, 1, count - 1, count, count + 1):
        st, raters, sims, devs, counts, sums, preds = _raw(kn, e, *rows100k, cap, order, null_terms=cap == 0)
        assert st == kn.OK, cap
        if ref is None:
            ref = (counts, sums, preds)
            assert counts.tolist() == [r.count for r in want]
        assert _same((counts, sums, preds), ref), cap  # independent of cap
        for j, row in enumerate(want):
            r, s, d = row.terms(order)
            m = min(row.count, cap)
            assert raters[j, :m].tolist() == r[:m].tolist(), (cap, j)
            assert np.array_equal(_bits(sims[j, :m]), _bits(s[:m])) and np.array_equal(_bits(devs[j, :m]), _bits(d[:m])), (cap, j)
            assert (raters[j, m:] == SENT_I).all() and (sims[j, m:] == SENT_F).all() and (devs[j, m:] == SENT_F).all(), (cap, j)
    st, *_, counts, sums, preds = _raw(kn, e, *rows100k, 3, order, null_sums=True)  # sums and predictions may be null
    assert st == kn.OK and _same((counts,), ref[:1]) and (sums == SENT_F).all() and (preds == SENT_F).all()
    e.close()


# ---- 4. match-count and class edges -----------------------------------------------------------------------------------------
def _class_of(kcap):
    return next(c for c in (64, 128, 256, 512, 1024, 2048) if kcap <= c)


@pytest.mark.parametrize("neighbours", [63, 64, 65, 128, 129, 512, 513, 1024, 1025, 2048])
def test_match_count_and_class_edges(kn, oracle, monkeypatch, capfd, neighbours):
    tr = explain_model.dense_train(neighbours + 1, seed=neighbours)
    assert np.bincount(np.unique(tr[0], return_inverse=True)[1]).min() > 4
    u, i = explain_model.dense_rows(tr)
    want = explain_model.TermModel(oracle, oracle.Model(*tr), oracle.SIM_COSINE, 2048).rows(u, i)
    assert [r.count for r in want[:3]] == [neighbours] * 3  # everybody else is a term of the common item's rows
    monkeypatch.setenv(TRACE, "1")
    e = kn.Engine(k=2048).fit(*tr)
    for order in (SUM_ORDER, BY_WEIGHT):
        capfd.readouterr()
        got = e.explain_batch(u, i, neighbours, order=order)
        assert _lines(capfd) == [f"explain CAP={_class_of(neighbours)} bits=1 order={order}"]
        _assert_rows(got, want, order, (neighbours, order))
    e.close()


# ---- 5. zero-similarity neighbours, 6. ties under BY_WEIGHT ---------------------------------------------------------------
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_zero_similarity_neighbours_are_listed_and_are_no_terms(kn, oracle, sim_name):
    c = explain_model.disjoint_case()
    ksim, osim = _sims(kn, oracle, sim_name)
    k = c.num_users
    u, i = c.test[0][:60].astype(np.int32), c.test[1][:60].astype(np.int32)
    want = explain_model.TermModel(oracle, oracle.Model(*c.train), osim, k).rows(u, i)
    e = kn.Engine(k=k, similarity=ksim).fit(*c.train)
    got = e.explain_batch(u, i, k - 1)
    _assert_rows(got, want, SUM_ORDER, sim_name)
    cold = set(c.groups["cold"].tolist())
    warm = next(int(x) for x in u if int(x) not in cold)
    ids, sims = e.neighbors(warm)
    zero = set(ids[sims == 0.0].tolist())
    assert len(ids) == k - 1 and cold <= zero  # in the list ...
    for j in np.flatnonzero(u == warm):
        assert not zero & set(got[0][j, :got[3][j]].tolist())  # ... and absent from the terms
    e.close()


@pytest.mark.parametrize("sim_name", ["jaccard", "cosine"])
def test_ties_under_by_weight_keep_summation_order(kn, oracle, sim_name):
    c = explain_model.clone_case()
    ksim, osim = _sims(kn, oracle, sim_name)
    k = c.num_users
    u, i = c.test[0][:60].astype(np.int32), c.test[1][:60].astype(np.int32)
    want = explain_model.TermModel(oracle, oracle.Model(*c.train), osim, k).rows(u, i)
    e = kn.Engine(k=k, similarity=ksim).fit(*c.train)
    plain = e.explain_batch(u, i, k - 1, order=SUM_ORDER)
    heavy = e.explain_batch(u, i, k - 1, order=BY_WEIGHT)
    _assert_rows(plain, want, SUM_ORDER, sim_name)
    _assert_rows(heavy, want, BY_WEIGHT, sim_name)
    ties = 0
    for j, m in enumerate(plain[3].tolist()):
        a = sorted(zip(plain[0][j, :m].tolist(), _bits(plain[1][j, :m]).tolist(), _bits(plain[2][j, :m]).tolist()))
        b = sorted(zip(heavy[0][j, :m].tolist(), _bits(heavy[1][j, :m]).tolist(), _bits(heavy[2][j, :m]).tolist()))
        assert a == b, j  # a permutation of the same terms
        mag = np.abs(heavy[1][j, :m])
        assert (mag[:-1] >= mag[1:]).all(), j
        place = {r: q for q, r in enumerate(plain[0][j, :m].tolist())}  # (a rater occurs once per item)
        tied = np.flatnonzero(mag[:-1] == mag[1:])
        ties += len(tied)
        for q in tied:
            assert place[int(heavy[0][j, q])] < place[int(heavy[0][j, q + 1])], (j, q)
    assert ties > 0
    e.close()


# ---- 7. without the rater bitmaps -------------------------------------------------------------------------------------------
def test_no_bitmaps_equals_the_bitmap_run(kn, oracle, syn100k, rows100k, monkeypatch, capfd):
    monkeypatch.setenv(TRACE, "1")
    cases = [("syn100k", _train(syn100k), rows100k, 300, 512)]
    for neighbours in (65, 1025):
        tr = explain_model.dense_train(neighbours + 1, seed=neighbours)
        cases.append((f"dense{neighbours}", tr, explain_model.dense_rows(tr), 2048, _class_of(neighbours)))
    for name, tr, (u, i), k, cap_class in cases:
        monkeypatch.delenv(NO_BITMAPS, raising=False)
        with_bits = kn.Engine(k=k).fit(*tr)
        monkeypatch.setenv(NO_BITMAPS, "1")  # read by the fit
        without = kn.Engine(k=k).fit(*tr)
        cap = min(k, with_bits.num_users - 1)
        for order in (SUM_ORDER, BY_WEIGHT):
            capfd.readouterr()
            a = with_bits.explain_batch(u, i, cap, order=order)
            assert _lines(capfd) == [f"explain CAP={cap_class} bits=1 order={order}"], name
            b = without.explain_batch(u, i, cap, order=order)
            assert _lines(capfd) == [f"explain CAP={cap_class} bits=0 order={order}"], name
            assert _same(a, b), (name, order)
        with_bits.close()
        without.close()


# ---- 8. chunks and forms ----------------------------------------------------------------------------------------------------
def test_chunks_and_forms_agree(kn, oracle, syn100k, rows100k, want100k, monkeypatch, capfd):
    import torch

    k = cap = 300
    u, i = rows100k
    n = len(u)
    workspace = 1 << 20
    chunk = max(1, (workspace // 2) // (20 * cap + 28))  # the rule of include/knncf.h
    assert -(-n // chunk) >= 3
    monkeypatch.setenv(TRACE, "1")
    small = kn.Engine(k=k, workspace_bytes=workspace).fit(*_train(syn100k))
    auto = kn.Engine(k=k).fit(*_train(syn100k))
    dev = kn.Engine(k=k).fit(*_train(syn100k))
    for order in (SUM_ORDER, BY_WEIGHT):
        capfd.readouterr()
        a = small.explain_batch(u, i, cap, order=order)
        assert len(_lines(capfd)) == -(-n // chunk)  # one launch per chunk
        b = auto.explain_batch(u, i, cap, order=order)
        assert len(_lines(capfd)) == 1
        t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        outs = [t(np.full((n, cap), -1, dtype=np.int32)), t(np.full((n, cap), np.nan)), t(np.full((n, cap), np.nan)),
                t(np.zeros(n, dtype=np.int32)), t(np.zeros((n, 2))), t(np.zeros(n))]
        dev.explain_batch_device(t(u), t(i), cap, *outs, order=order)
        assert len(_lines(capfd)) == 1
        c = tuple(x.cpu().numpy() for x in outs)
        assert _same(a, b) and _same(a, c), order
        _assert_rows(a, want100k("cosine", 300, oracle.SIM_COSINE), order, order)
    for e in (small, auto, dev):
        e.close()


# ---- 9. handle state --------------------------------------------------------------------------------------------------------
def test_handle_state_is_predict_batchs(kn, syn100k, rows100k, tmp_path):
    d = syn100k
    u, i = rows100k
    test = (d.test.users, d.test.items, d.test.ratings)
    a, b = (kn.Engine(k=30).fit(*_train(d)) for _ in range(2))
    first = a.explain_batch(u, i, 30)
    preds = b.predict_batch(kn.PRED_KNN, u, i)
    assert np.array_equal(_bits(first[5]), _bits(preds))
    ta, tb = _table(a, tmp_path / "a.nb"), _table(b, tmp_path / "b.nb")
    assert ta == tb and sum(s >= 0 for s in ta["seq"]) >= 30  # the lists of the rows' known users, numbered alike
    assert open(tmp_path / "a.nb", "rb").read()[:48] == open(tmp_path / "b.nb", "rb").read()[:48]
    again = a.explain_batch(u, i, 30)  # lists that exist: nothing changes but the call count in the header
    assert _same(first, again)
    b.predict_batch(kn.PRED_KNN, u, i)
    assert _table(a, tmp_path / "a2.nb") == _table(b, tmp_path / "b2.nb")
    assert {k: v for k, v in ta.items() if k != "header"} == {k: v for k, v in _table(a, tmp_path / "a3.nb").items() if k != "header"}
    assert _bits(a.mae(kn.PRED_KNN, *test)).tolist() == _bits(b.mae(kn.PRED_KNN, *test)).tolist()
    a.close()
    b.close()


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(kn, syn100k, rows100k, tmp_path):
    tr = _train(syn100k)
    u, i = rows100k[0][:5], rows100k[1][:5]

    def untouched(res):
        return all((x == (SENT_I if x.dtype == np.int32 else SENT_F)).all() for x in res[1:])

    fresh = kn.Engine(k=10)
    res = _raw(kn, fresh, u, i, 4)
    assert res[0] == kn.E_STATE and untouched(res)
    fresh.close()
    one = kn.Engine(k=10, similarity=kn.SIM_ONE).fit(*tr)
    res = _raw(kn, one, u, i, 4)
    assert res[0] == kn.E_UNSUPPORTED and untouched(res)
    with pytest.raises(kn.KnncfError, match="similarityOne") as err:
        one.explain_batch(u, i, 4)
    assert err.value.status == kn.E_UNSUPPORTED
    one.close()
    shard = kn.Engine(k=10, shard_rank=0, shard_count=2).fit(*tr)
    res = _raw(kn, shard, u, i, 4)
    assert res[0] == kn.E_UNSUPPORTED and untouched(res)
    shard.close()
    e = kn.Engine(k=10).fit(*tr)
    before = _table(e, tmp_path / "before.nb")
    for order, cap in ((2, 4), (-1, 4), (SUM_ORDER, -1)):
        res = _raw(kn, e, u, i, cap, order)
        assert res[0] == kn.E_INVALID and untouched(res), (order, cap)
    res = _raw(kn, e, u, i, 4, null_terms=True)  # cap > 0 needs the term arrays
    assert res[0] == kn.E_INVALID and untouched(res)
    p = lambda a, t: a.ctypes.data_as(t)
    counts = np.full(5, SENT_I, dtype=np.int32)
    assert e._lib.knncf_explain_batch(e._h, p(u, i32p), p(i, i32p), -1, 0, 0, None, None, None, p(counts, i32p), None, None) == kn.E_INVALID
    assert e._lib.knncf_explain_batch(e._h, None, None, 0, 0, 4, None, None, None, None, None, None) == kn.OK  # n == 0
    assert (counts == SENT_I).all() and _table(e, tmp_path / "after.nb") == before  # nothing built, nothing written
    e.close()
