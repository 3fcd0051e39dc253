"""Every k-dependent kernel instantiation against the CPU oracle, bit for bit, with a witness of which one ran.

The engine picks a kernel instantiation from kcap = min(k, U - 1) ("Dispatch by kcap"): five forms each of the
item-grouped and the row-grouped prediction kernel, six of the general one, six of the sweep kernel, four re-rank tiles for
each similarity, two id-sorts.  Each cell below sets KNNCF_DEBUG_TRACE_DISPATCH, reads the launchers' lines from the
library's stderr and asserts them next to the values, so that a moved threshold cannot leave a kernel unreached unnoticed.
KNNCF_DEBUG_NO_LDS_BITMAPS makes a small handle take the paths of more than 262 144 users (test_gpu_parity's wide-shape
test shows the same dispatch occurring by itself), KNNCF_DEBUG_NO_ITEM_BITMAPS those of a shape whose rater bitmaps do not
fit in device memory.

Every data set here has more than 4 ratings per train user: no pair's summation order depends on the build history then
(SURVEY N6), so one handle driven through many k by set_k is comparable with a fresh oracle pipeline per k."""
import importlib

import numpy as np
import pytest

from tests.test_gpu_k_sweep import _with_unknowns

pytestmark = pytest.mark.gpu
MAE_TOL = 1e-9
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
PATH_ENV = {"default": None, "no_lds_bitmaps": "KNNCF_DEBUG_NO_LDS_BITMAPS", "no_item_bitmaps": "KNNCF_DEBUG_NO_ITEM_BITMAPS"}
BOUNDARY_KS = (64, 65, 128, 129, 256, 257, 320, 321, 384, 385, 512, 513)
TAIL_ROWS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
BIG_KS = (1024, 1025, 2048)
BIG_SWEEP_KS = (10, 512, 513, 1024, 1025, 2048)
PERSONALIZED_USERS = (100, 200, 300, 500, 1500)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _cols(rs):
    return rs.users, rs.items, rs.ratings


def _assert_dense_rows(tr):
    assert np.bincount(np.unique(tr[0], return_inverse=True)[1]).min() > 4


# ---- the expected dispatch, written out from the table in DESIGN.md (not computed by the code under test) ----------------
def _grouped_form(kcap):
    for top, form in ((64, "TR=1 G=4"), (128, "TR=2 G=4"), (256, "TR=4 G=2"), (320, "TR=5 G=2"), (512, "TR=8 G=1")):
        if kcap <= top:
            return form
    return None


def _general_cap(kcap):
    return next(c for c in (64, 128, 256, 512, 1024, 2048) if kcap <= c)


def _rerank_tile(kcap):
    return next(t for top, t in ((384, 512), (512, 1024), (1024, 2048), (2048, 4096)) if kcap <= top)


def _bitonic_m(kcap):
    m = 128
    while m < kcap:
        m *= 2
    return m


def _predict_line(path, kcap):
    if path == "no_item_bitmaps" or kcap > 512:
        return f"predict general CAP={_general_cap(kcap)}"
    return f"predict {'items' if path == 'default' else 'rows'} {_grouped_form(kcap)}"


def _idsort_line(path, kcap):
    """the id-sorted copies are made for the kernels that probe global memory: everything but the item-grouped form"""
    if path == "no_lds_bitmaps":
        return f"idsort bitonic m={_bitonic_m(kcap)}"
    return None if _predict_line(path, kcap).startswith("predict items") else "idsort rank"


def _knn_lines(path, kcap, jaccard):
    lines = {f"rerank TILE={_rerank_tile(kcap)} jaccard={int(jaccard)}", _predict_line(path, kcap)}
    if _idsort_line(path, kcap):
        lines.add(_idsort_line(path, kcap))
    return lines


def _trace(capfd):
    return [ln[len("knncf-dispatch "):] for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch ")]


# ---- shared, unchanged state: data, oracle answers per (data, similarity, k), one fitted handle per (data, similarity, path)
@pytest.fixture(scope="module")
def ml100k(syn100k):
    tr, te = _with_unknowns(syn100k)
    _assert_dense_rows(tr)
    return tr, te


@pytest.fixture(scope="module")
def wide2400(synth):
    d = synth.syn_scaled(2400, 500, 160_000, seed=43, half_stars=True, shuffle=True)
    tr = _cols(d.train)
    _assert_dense_rows(tr)
    return tr, tuple(a[:4000] for a in _cols(d.test))


@pytest.fixture(scope="module")
def answers(oracle):
    """(name, tr, te, sim, k) -> (MAE, predictions of every row of te, the pipeline that made them)"""
    models, cache = {}, {}

    def get(name, tr, te, sim, k):
        if (name, sim, k) not in cache:
            if name not in models:
                models[name] = oracle.Model(*tr)
            p = models[name].pipeline(sim, k)
            want, preds = p.mae(*te, True)
            preds.setflags(write=False)
            cache[name, sim, k] = (want, preds, p)
        return cache[name, sim, k]

    return get


@pytest.fixture(scope="module")
def handles(kn):
    """fitted engines, made on first use by _handle() while the path's environment is set (the fit reads NO_ITEM_BITMAPS)"""
    made = {}
    yield made
    for e in made.values():
        e.close()


def _handle(kn, handles, monkeypatch, name, tr, sim, path):
    monkeypatch.setenv(TRACE, "1")
    for env in PATH_ENV.values():
        if env:
            monkeypatch.delenv(env, raising=False)
    if PATH_ENV[path]:
        monkeypatch.setenv(PATH_ENV[path], "1")
    if (name, sim, path) not in handles:
        handles[name, sim, path] = kn.Engine(k=10, similarity=sim, flags=kn.FLAG_VERIFY_BOUND).fit(*tr)
    return handles[name, sim, path]


def _check_knn_cell(kn, e, capfd, answer, te, k, path, jaccard, list_users):
    want, opreds, p = answer
    kcap = min(k, e.num_users - 1)
    e.set_k(k)
    e.reset_timings()
    capfd.readouterr()
    preds = e.predict_batch(kn.PRED_KNN, te[0], te[1])
    mae = e.mae(kn.PRED_KNN, *te)
    lists = [e.neighbors(int(u)) for u in list_users]
    lines = _trace(capfd)
    assert set(lines) == _knn_lines(path, kcap, jaccard), (k, path)
    assert lines.count(_predict_line(path, kcap)) == 2, (k, path)  # predict_batch and mae, one launch each
    bad = np.nonzero(_bits(preds) != _bits(opreds))[0]
    assert len(bad) == 0, (k, path, len(bad), bad[:8].tolist(), preds[bad[:8]].tolist(), opreds[bad[:8]].tolist())
    assert abs(mae - want) <= MAE_TOL, (k, path, mae, want)
    for u, (ids, sims) in zip(list_users, lists):
        oids, osims = p.neighbors(int(u))
        assert len(ids) == kcap and ids.tolist() == oids.tolist(), (k, path, int(u))
        assert np.array_equal(_bits(sims), _bits(osims)), (k, path, int(u))
    assert e.timings()["max_bound_violation"] <= 0.0, (k, path)


def test_no_trace_unless_asked(kn, ml100k, handles, monkeypatch, capfd):
    tr, te = ml100k
    e = _handle(kn, handles, monkeypatch, "ml100k", tr, kn.SIM_COSINE, "default")
    monkeypatch.delenv(TRACE)
    e.set_k(300)
    capfd.readouterr()
    e.mae(kn.PRED_KNN, *te)
    e.mae_sweep((10, 300), *te)
    assert "knncf-dispatch" not in capfd.readouterr().err


# ---- a. boundary k at the ml-100k shape -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", BOUNDARY_KS)
@pytest.mark.parametrize("path", list(PATH_ENV))
def test_boundary_k_cosine(kn, oracle, ml100k, answers, handles, monkeypatch, capfd, path, k):
    tr, te = ml100k
    e = _handle(kn, handles, monkeypatch, "ml100k", tr, kn.SIM_COSINE, path)
    if k == 513:
        assert _predict_line(path, k) == "predict general CAP=1024"
    _check_knn_cell(kn, e, capfd, answers("ml100k", tr, te, oracle.SIM_COSINE, k), te, k, path, False, np.unique(tr[0])[::23])


# ---- b. Jaccard over the re-rank tiles ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (384, 385, 512, 513))
@pytest.mark.parametrize("path", ["default", "no_lds_bitmaps"])
def test_boundary_k_jaccard(kn, oracle, ml100k, answers, handles, monkeypatch, capfd, path, k):
    tr, te = ml100k
    e = _handle(kn, handles, monkeypatch, "ml100k", tr, kn.SIM_JACCARD, path)
    _check_knn_cell(kn, e, capfd, answers("ml100k", tr, te, oracle.SIM_JACCARD, k), te, k, path, True, np.unique(tr[0])[::23])


# ---- the sweep kernel's CAP = 512 and CAP = 1024 forms, with and without the LDS bitmap (CAP = 2048: part d) ---------------
@pytest.mark.parametrize("kmax", (512, 513))
@pytest.mark.parametrize("path", list(PATH_ENV))
def test_boundary_k_sweep(kn, oracle, ml100k, answers, handles, monkeypatch, capfd, path, kmax):
    tr, te = ml100k
    e = _handle(kn, handles, monkeypatch, "ml100k", tr, kn.SIM_COSINE, path)
    ks = tuple(k for k in BOUNDARY_KS if k <= kmax)
    capfd.readouterr()
    maes, preds = e.mae_sweep(ks, *te, predictions=True)
    lines = _trace(capfd)
    cap = 512 if kmax <= 512 else 1024
    assert set(lines) == {f"rerank TILE={_rerank_tile(kmax)} jaccard=0", f"sweep CAP={cap} bits={int(path == 'default')}"}, (path, kmax)
    assert lines.count(f"sweep CAP={cap} bits={int(path == 'default')}") == 1
    for q, k in enumerate(ks):
        want, opreds, _ = answers("ml100k", tr, te, oracle.SIM_COSINE, k)
        assert np.array_equal(_bits(preds[q]), _bits(opreds)), (path, k)
        assert abs(maes[q] - want) <= MAE_TOL, (path, k)


# ---- c. row-count tails at k = 300 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATH_ENV))
def test_row_count_tails(kn, oracle, ml100k, answers, handles, monkeypatch, capfd, path):
    """a wave of the row-grouped kernel takes 32 rows and a workgroup 128, the item-grouped kernel's chunk is 64 rows: prefixes
    around those sizes, then all rows of the three users with the most test rows together with single rows of three users
    (rows of one user that exceed G, straddle a 32-row chunk, or stand alone).  The data has one user with exactly one test
    row; it is one of the three, the other two are the next lightest users with their first test row only."""
    tr, te = ml100k
    k = 300
    e = _handle(kn, handles, monkeypatch, "ml100k", tr, kn.SIM_COSINE, path)
    _, opreds, _ = answers("ml100k", tr, te, oracle.SIM_COSINE, k)
    e.set_k(k)
    known = te[0][:-2]  # (without the two appended unknown rows)
    users, first, counts = np.unique(known, return_index=True, return_counts=True)
    order = np.argsort(counts, kind="stable")
    heavy, light = users[order[-3:]], order[:3]
    assert counts[order[-3:]].min() > 128 and counts[light[0]] == 1
    pick = np.sort(np.concatenate([np.nonzero(np.isin(known, heavy))[0], first[light]]))
    for n, rows in [(n, np.arange(n)) for n in TAIL_ROWS] + [("users", pick)]:
        capfd.readouterr()
        preds = e.predict_batch(kn.PRED_KNN, te[0][rows], te[1][rows])
        lines = _trace(capfd)
        assert lines.count(_predict_line(path, k)) == 1 and set(lines) <= _knn_lines(path, k, False), (path, n, lines)
        assert np.array_equal(_bits(preds), _bits(opreds[rows])), (path, n)


# ---- d. beyond 1024 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", BIG_KS)
def test_k_1024_to_2048(kn, oracle, wide2400, answers, handles, monkeypatch, capfd, k):
    tr, te = wide2400
    e = _handle(kn, handles, monkeypatch, "wide2400", tr, kn.SIM_COSINE, "default")
    assert _knn_lines("default", k, False) == {f"rerank TILE={2048 if k == 1024 else 4096} jaccard=0",
                                               f"predict general CAP={1024 if k == 1024 else 2048}", "idsort rank"}
    _check_knn_cell(kn, e, capfd, answers("wide2400", tr, te, oracle.SIM_COSINE, k), te, k, "default", False, np.unique(te[0])[::97])


def test_k_1025_jaccard(kn, oracle, wide2400, answers, handles, monkeypatch, capfd):
    tr, te = wide2400
    e = _handle(kn, handles, monkeypatch, "wide2400", tr, kn.SIM_JACCARD, "default")
    assert "rerank TILE=4096 jaccard=1" in _knn_lines("default", 1025, True)
    _check_knn_cell(kn, e, capfd, answers("wide2400", tr, te, oracle.SIM_JACCARD, 1025), te, 1025, "default", True, np.unique(te[0])[::97])


@pytest.mark.parametrize("path", ["default", "no_item_bitmaps"])
def test_sweep_to_2048(kn, oracle, wide2400, answers, handles, monkeypatch, capfd, path):
    tr, te = wide2400
    e = _handle(kn, handles, monkeypatch, "wide2400", tr, kn.SIM_COSINE, path)
    capfd.readouterr()
    maes, preds = e.mae_sweep(BIG_SWEEP_KS, *te, predictions=True)
    lines = _trace(capfd)
    sweep = f"sweep CAP=2048 bits={int(path == 'default')}"
    assert set(lines) == {"rerank TILE=4096 jaccard=0", sweep} and lines.count(sweep) == 1, (path, lines)
    loop = []
    for q, k in enumerate(BIG_SWEEP_KS):
        want, opreds, _ = answers("wide2400", tr, te, oracle.SIM_COSINE, k)
        assert np.array_equal(_bits(preds[q]), _bits(opreds)), (path, k)
        assert abs(maes[q] - want) <= MAE_TOL, (path, k)
        e.set_k(k)
        loop.append(e.mae(kn.PRED_KNN, *te))
    assert np.array_equal(_bits(maes), _bits(loop)), path


# ---- e. PERSONALIZED through the item-grouped and the general kernel (kcap = U) -------------------------------------------
@pytest.fixture(scope="module")
def personalized_sets(synth, oracle):
    """U -> (train, the test rows plus 200 training pairs, the oracle's Model)"""
    out = {}

    def get(n_users):
        if n_users not in out:
            d = synth.syn_scaled(n_users, 150, 40 * n_users, seed=9100 + n_users)
            tr = _cols(d.train)
            _assert_dense_rows(tr)
            assert len(np.unique(tr[0])) == n_users
            rows = tuple(np.concatenate([a, b[:200]]) for a, b in zip(_cols(d.test), tr))
            out[n_users] = (tr, rows, oracle.Model(*tr))
        return out[n_users]

    return get


@pytest.mark.parametrize("sim", ["cosine", "jaccard"])
@pytest.mark.parametrize("n_users,path", [(u, "default") for u in PERSONALIZED_USERS] + [(200, "no_item_bitmaps"), (1500, "no_item_bitmaps")])
def test_personalized_kcap_is_u(kn, oracle, personalized_sets, handles, monkeypatch, capfd, n_users, path, sim):
    tr, rows, model = personalized_sets(n_users)
    ksim, osim = (kn.SIM_COSINE, oracle.SIM_COSINE) if sim == "cosine" else (kn.SIM_JACCARD, oracle.SIM_JACCARD)
    e = _handle(kn, handles, monkeypatch, f"personalized{n_users}", tr, ksim, path)
    expect = {("default", 100): "predict items TR=2 G=4", ("default", 200): "predict items TR=4 G=2",
              ("default", 300): "predict items TR=5 G=2", ("default", 500): "predict items TR=8 G=1",
              ("default", 1500): "predict general CAP=2048", ("no_item_bitmaps", 200): "predict general CAP=256",
              ("no_item_bitmaps", 1500): "predict general CAP=2048"}[path, n_users]
    assert expect == _predict_line(path, n_users)
    _, opreds = model.pipeline(osim, -1).mae(*rows, True)
    capfd.readouterr()
    preds = e.predict_batch(kn.PRED_PERSONALIZED, rows[0], rows[1])
    assert _trace(capfd) == [expect], (n_users, path, sim)
    bad = np.nonzero(_bits(preds) != _bits(opreds))[0]
    assert len(bad) == 0, (n_users, path, sim, len(bad), bad[:8].tolist())
