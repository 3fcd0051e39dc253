"""Tied and one-sided similarity rows against the oracle: the rows that leave select.hip's ordinary path.

Everything between the MFMA filter and the exact fp64 re-rank is built around a spread-out similarity row; the i.i.d. inputs
of the other GPU tests never leave that path (they assert fallback_rows == 0).  tests/degenerate.py plants the rows real
rating files have — cold users (similarity exactly 0.0 with everybody), clones (ties hundreds wide, values of about 1.0),
two polarised camps (a k-th value far below the histogram), constant users (all-zero rows) — and this file pins, bit for bit
against the oracle: the shortlist overflow (`s_out > cap`) and the store overflow (`s_count > GCAP`) of k_tail_select, a final
threshold in bin 0, maximum-length shortlists in the re-rank (plain and sliced), exact cosine ties cut at rank k, and every
rebuild branch of build_neighbors (per-row exact path directly; redo_marked first, whole-matrix and per row block).
tests/test_degenerate_premises.py proves from the oracle alone that the inputs are what they claim to be.

Each test prints its path witnesses (fallback_rows, select_launches, gemm_launches, shortlist_total) before asserting them."""
import importlib

import numpy as np
import pytest

from tests import degenerate as dg
from tests.test_gpu_fold_in import _check as _check_fold_in

pytestmark = pytest.mark.gpu
MAE_TOL = 1e-9
K = dg.K
HEAD_ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def refs(oracle):
    """the oracle's model of a case and its bulk kNN table (cosine) of a set of users, each computed once and left unchanged"""
    models, tables = {}, {}

    class Refs:
        @staticmethod
        def model(name):
            if name not in models:
                models[name] = oracle.Model(*dg.case(name).train)
            return models[name]

        @staticmethod
        def table(name, k, groups):
            key = (name, k, groups)
            if key not in tables:
                c = dg.case(name)
                users = np.unique(np.concatenate([dg.ordinary_sample(name) if g == "ordinary" else c.groups[g] for g in groups]))
                tables[key] = Refs.model(name).knn_table(k, users=users)
            return tables[key]

        @staticmethod
        def pipeline(name, sim, k, users):
            """(users, their neighbour lists, the mask of their test rows, those rows' MAE and predictions) from the per-pair
            closures: single-threaded, so for a few dozen users"""
            key = (name, sim, k)
            if key not in tables:
                test = dg.case(name).test
                p = Refs.model(name).pipeline(sim, k)
                lists = [p.neighbors(int(u)) for u in users]
                mask = np.isin(test[0], users)
                tables[key] = (users, lists, mask) + p.mae(*(a[mask] for a in test), True)
            return tables[key]

    return Refs


def _engine(kn, train, k=K, sim=0, flags=0, **kw):
    e = kn.Engine(k=k, similarity=sim, flags=kn.FLAG_VERIFY_BOUND | flags, **kw)
    e.fit(*train)
    return e


def _symmetric(monkeypatch, on):
    if on:
        monkeypatch.delenv("KNNCF_DEBUG_NO_SYMMETRIC_GEMM", raising=False)
    else:
        monkeypatch.setenv("KNNCF_DEBUG_NO_SYMMETRIC_GEMM", "1")


def _witness(label, e):
    t = e.timings()
    print(f"[witness] {label}: fallback_rows={t['fallback_rows']} select_launches={t['select_launches']} "
          f"gemm_launches={t['gemm_launches']} shortlist_total={t['shortlist_total']} head_items={t['head_items']}")
    assert t["max_bound_violation"] <= 0.0
    return t


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _lists_equal_table(e, table):
    ids, sims, counts = e.neighbors_batch(table.row_user)
    assert counts.tolist() == [table.width] * table.rows
    bad = np.flatnonzero((ids != table.ids).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} of {table.rows} neighbour lists differ, first user {table.row_user[bad[0]]}"
    assert np.array_equal(_bits(sims), _bits(table.sims))


def _rows_equal_table(kn, e, table, test, preds):
    """the predictions (bitwise) and the MAE of every test row of the table's users; preds: the engine's, aligned with test"""
    mask = np.isin(test[0], table.row_user)
    rows = tuple(a[mask] for a in test)
    assert mask.sum() >= table.rows // 2
    want, opreds = table.mae(*rows)
    diff = np.flatnonzero(_bits(preds[mask]) != _bits(opreds))
    assert len(diff) == 0, f"{len(diff)} of {mask.sum()} predictions differ, first user {rows[0][diff[0]]}"
    got = e.mae(kn.PRED_KNN, *rows)
    print(f"[figure] MAE over {mask.sum()} sampled rows: engine {got!r} oracle {want!r}")
    assert abs(got - want) <= MAE_TOL


def _equal_pipeline(kn, e, want, test, preds):
    """the same against Refs.pipeline's lists and predictions (the oracle's per-pair closures, any similarity)"""
    users, lists, mask, want_mae, opreds = want
    ids, sims, counts = e.neighbors_batch(users)
    for row, u in enumerate(users):
        oids, osims = lists[row]
        assert ids[row, :counts[row]].tolist() == oids.tolist(), f"user {u}"
        assert _bits(sims[row, :counts[row]]).tolist() == _bits(osims).tolist(), f"user {u}"
    assert np.array_equal(_bits(preds[mask]), _bits(opreds))
    got = e.mae(kn.PRED_KNN, *(a[mask] for a in test))
    print(f"[figure] MAE over {mask.sum()} sampled rows: engine {got!r} oracle {want_mae!r}")
    assert abs(got - want_mae) <= MAE_TOL


# ---- 1 (and 8): shortlist overflow, few rows: straight to the per-row exact path ---------------------------------------------
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("sim", ["cosine", "jaccard"])
def test_shortlist_overflow_few_rows(kn, oracle, refs, monkeypatch, sim, symmetric):
    """cold(20 480, 40) + 50 constant users, k = 300, a whole-matrix build through predict_batch: a cold row holds 0.0 in
    (nearly) every column, its final threshold lets all ~20 479 of them through, the shortlist holds 16 384: 40 marked rows,
    fewer than max(64, count / 200), rebuilt one by one (launch_exact_row + 64-bit radix sort + k_fallback_write).
    The constant users' cosine rows are all-zero too (premises file): their test rows come in a second call, a partial build,
    which must add exactly one fallback row each — under Jaccard they are ordinary rows and add none."""
    _symmetric(monkeypatch, symmetric)
    jac = sim == "jaccard"
    c = dg.case("cold40")
    cold, const = c.groups["cold"], c.groups["constant"]
    is_const = np.isin(c.test[0], const)
    e = _engine(kn, c.train, sim=kn.SIM_JACCARD if jac else kn.SIM_COSINE)
    preds = np.full(len(c.test[0]), np.nan)
    preds[~is_const] = e.predict_batch(kn.PRED_KNN, c.test[0][~is_const], c.test[1][~is_const])
    t = _witness(f"1 cold40 {sim} symmetric={symmetric}, whole-matrix build", e)
    assert t["fallback_rows"] == 40 and t["gemm_launches"] == 1 and t["select_launches"] == 1
    preds[is_const] = e.predict_batch(kn.PRED_KNN, c.test[0][is_const], c.test[1][is_const])
    t = _witness(f"8 cold40 {sim} symmetric={symmetric}, + the 50 constant users' rows", e)
    assert t["fallback_rows"] == 40 + (0 if jac else 50) and t["select_launches"] == 2
    if jac:
        users = np.unique(np.concatenate([cold, const[::10], dg.ordinary_sample("cold40")[::50]]))
        _equal_pipeline(kn, e, refs.pipeline("cold40", oracle.SIM_JACCARD, K, users), c.test, preds)
    else:
        table = refs.table("cold40", K, ("ordinary", "cold", "constant"))
        _lists_equal_table(e, table)
        _rows_equal_table(kn, e, table, c.test, preds)
    # every queried user was built by the two calls above or is an ordinary row: nothing else fell back
    assert _witness("1 cold40 after the list queries", e)["fallback_rows"] == 40 + (0 if jac else 50)
    e.close()


# ---- 2: shortlist overflow, many rows: redo_marked first, then the per-row path ------------------------------------------------
@pytest.mark.parametrize("path", ["symmetric", "row_blocks"])
def test_shortlist_overflow_many_rows(kn, refs, monkeypatch, path):
    """cold(20 480, 160): more marked rows than max(64, count / 200) = 102, so the build first sends them through select +
    re-rank again with the plain thresholds (one more select launch than the 40-row build's single one), they overflow again,
    and every one of them ends on the per-row exact path.  row_blocks: a 6 GB workspace cuts the users into >= 3 row blocks of
    row-block GEMMs; rows are dealt longest first, so the last block holds all 160 cold rows and runs the per-block redo."""
    _symmetric(monkeypatch, path == "symmetric")
    c = dg.case("cold160")
    e = _engine(kn, c.train, workspace_bytes=(6 << 30) if path == "row_blocks" else 0)
    preds = e.predict_batch(kn.PRED_KNN, c.test[0], c.test[1])
    t = _witness(f"2 cold160 {path}", e)
    blocks = 1 if path == "symmetric" else t["gemm_launches"]
    assert t["gemm_launches"] == 1 if path == "symmetric" else blocks >= 3
    assert t["fallback_rows"] == 160 and t["select_launches"] == blocks + 1
    table = refs.table("cold160", K, ("ordinary", "cold"))
    _lists_equal_table(e, table)
    _rows_equal_table(kn, e, table, c.test, preds)
    assert e.timings()["fallback_rows"] == 160
    e.close()


# ---- 3: store overflow ----------------------------------------------------------------------------------------------------------
def test_store_overflow_wide_rows(kn, refs):
    """cold(70 000, 24) over sparse background rows, queried through neighbors_batch only: a partial row-block build over five
    column tiles with the anticipation active.  A cold row's 8750 groups of 8 columns all qualify (every maximum is 0.0), the
    provisional store holds 8192: `s_count > GCAP`, the row is marked before a shortlist exists."""
    c = dg.case("cold_wide")
    table = refs.table("cold_wide", K, ("ordinary", "cold"))
    assert table.rows == 24 + len(dg.ordinary_sample("cold_wide"))
    e = _engine(kn, c.train)
    _lists_equal_table(e, table)
    t = _witness("3 cold_wide, partial build of 24 cold + 13 background rows", e)
    assert t["fallback_rows"] == 24 and t["gemm_launches"] == 1 and t["select_launches"] == 1
    e.close()


# ---- 4: threshold in bin 0, full-length shortlists ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "sliced", "bf16"])
def test_threshold_in_bin_zero_full_length_shortlists(kn, refs, monkeypatch, variant):
    """camps(12 000, 100), k = 300: a camp-A row's k-th value is about -0.5, below HIST_LO: the final threshold sits in bin 0
    and all U - 1 columns become candidates — the cap (16 384) covers them, so no row falls back and the re-rank works through
    11 999-entry shortlists (plain: LDS-sized trips; sliced: KNNCF_DEBUG_SLICE_ROWS slices every row 8 ways).  Camp-B rows are
    ordinary, with thresholds near the histogram's top bin."""
    if variant == "sliced":
        monkeypatch.setenv("KNNCF_DEBUG_SLICE_ROWS", "100000")
    else:
        monkeypatch.delenv("KNNCF_DEBUG_SLICE_ROWS", raising=False)
    c = dg.case("camps12k")
    U = c.num_users
    e = _engine(kn, c.train, flags=kn.FLAG_BF16_FILTER if variant == "bf16" else 0)
    preds = e.predict_batch(kn.PRED_KNN, c.test[0], c.test[1])
    t = _witness(f"4 camps12k {variant}", e)
    assert t["fallback_rows"] == 0 and t["gemm_launches"] == 1 and t["select_launches"] == 1
    assert t["shortlist_total"] >= 100 * (U - 1)
    table = refs.table("camps12k", K, ("ordinary", "camp_a"))
    _lists_equal_table(e, table)
    _rows_equal_table(kn, e, table, c.test, preds)
    assert e.timings()["fallback_rows"] == 0
    e.close()


# ---- 5: bin 0 beyond the cap -----------------------------------------------------------------------------------------------------
def test_threshold_in_bin_zero_beyond_the_cap(kn, refs):
    """camps(20 480, 100): the same rows no longer fit the shortlist: 100 marked rows (<= max(64, 20 480 / 200) = 102: no
    second select pass), each rebuilt by the per-row exact path — strongly negative values through its 64-bit sort keys"""
    c = dg.case("camps20k")
    e = _engine(kn, c.train)
    preds = e.predict_batch(kn.PRED_KNN, c.test[0], c.test[1])
    t = _witness("5 camps20k", e)
    assert t["fallback_rows"] == 100 and t["gemm_launches"] == 1 and t["select_launches"] == 1
    table = refs.table("camps20k", K, ("ordinary", "camp_a"))
    _lists_equal_table(e, table)
    _rows_equal_table(kn, e, table, c.test, preds)
    assert e.timings()["fallback_rows"] == 100
    e.close()


# ---- 6 (and 8): exact cosine ties at rank k --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,head,f32", [(300, 64, False), (300, HEAD_ALL, False), (1000, 64, False), (1000, HEAD_ALL, False),
                                        (300, 64, True)])
def test_exact_cosine_ties_at_rank_k(kn, oracle, refs, k, head, f32):
    """clones(3 200, 4, 700) + 50 constant users: k = 300 cuts inside the ~1.0 ties of a clone's own group, k = 1000 inside
    another group's; the tied approximate values come from head + tail (64 dense items) and from the GEMM alone; ties are
    broken by Set order of the users.  Every clone, every constant user, every 7th background user; recommendations of clones
    (their predictions tie massively as well) singly and as a batch."""
    c = dg.case("clones")
    e = _engine(kn, c.train, k=k, flags=kn.FLAG_F32_PANEL if f32 else 0, head_items=head)
    preds = e.predict_batch(kn.PRED_KNN, c.test[0], c.test[1])
    t = _witness(f"6 clones k={k} head={head:#x} f32_panel={f32}", e)
    assert t["fallback_rows"] == 0 and t["gemm_launches"] == 1 and t["head_items"] == min(head, e.num_items)
    table = refs.table("clones", k, ("ordinary", "clones", "constant"))
    assert table.rows == 2800 + 50 + 50
    _lists_equal_table(e, table)
    _rows_equal_table(kn, e, table, c.test, preds)
    assert e.timings()["fallback_rows"] == 0
    if not f32 and (k, head) in ((300, 64), (1000, HEAD_ALL)):
        p = refs.model("clones").pipeline(oracle.SIM_COSINE, k)
        batch = np.concatenate([c.groups[f"clones{g}"][5:21] for g in range(4)])  # 64 clones, 16 of every prototype
        want = [p.recommend(int(u), 10) for u in batch]
        for j in (0, 16, 32, 48):
            ids, pr = e.recommend(kn.PRED_KNN, int(batch[j]), 10)
            assert ids.tolist() == want[j][0].tolist() and _bits(pr).tolist() == _bits(want[j][1]).tolist(), batch[j]
        items, pr, counts = e.recommend_batch(kn.PRED_KNN, batch, 10)
        for j in range(len(batch)):
            assert items[j, :counts[j]].tolist() == want[j][0].tolist(), batch[j]
            assert _bits(pr[j, :counts[j]]).tolist() == _bits(want[j][1]).tolist(), batch[j]
    e.close()


# ---- 7: fold-in against degenerate fits ------------------------------------------------------------------------------------------
def _user_rows(train, u):
    m = train[0] == u
    return train[1][m], train[2][m]


def test_fold_in_against_a_cold_fit(kn, oracle):
    """on the fit of case 1: a query identical to a cold user's ratings (one neighbour of about 1.0, then 0.0 ties in Set
    order), and one that shares no item with anybody (nothing but the tie)"""
    c = dg.case("cold40")
    e = _engine(kn, c.train)
    it, rt = _user_rows(c.train, int(c.groups["cold"][0]))
    some = np.unique(c.train[1])[::400]
    for q, qi, qr in ((10_000_001, it, rt),
                      (10_000_002, np.arange(5_000_001, 5_000_007, dtype=np.int32), np.array([1.0, 5.0, 3.0, 4.0, 2.0, 5.0]))):
        oids, osims = _check_fold_in(kn, oracle, e, c.train, q, qi, qr, oracle.SIM_COSINE, K, np.concatenate([some, qi, [999_999]]), ns=(3,))
        assert osims[-1] == 0.0 and (osims[0] > 0.99) == (q == 10_000_001)  # (the case is what it claims to be)
    e.close()


def test_fold_in_against_a_clone_fit(kn, oracle):
    """on the fit of case 6: a query identical to a prototype — 700 neighbours of about 1.0 for k = 300"""
    c = dg.case("clones")
    e = _engine(kn, c.train)
    it, rt = _user_rows(c.train, int(c.groups["clones0"][0]))
    some = np.unique(c.train[1])[::40]
    oids, osims = _check_fold_in(kn, oracle, e, c.train, 10_000_003, it, rt, oracle.SIM_COSINE, K, np.concatenate([some, [999_999]]), ns=(3, 25))
    assert abs(osims[-1] - 1.0) < 1e-12 and np.isin(oids, c.groups["clones0"]).all()
    e.close()
