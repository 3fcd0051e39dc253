"""The streamed Personalized predictor (csrc/personalized.hip: k_ptiles, k_sim_rows, k_fold_rows; api.cpp: plan_personal_rows /
predict_personal_rows) at the sizes its kernels and its block plan are built around, bit for bit against
oracle.Model(*train).pipeline(sim, -1).  The fits and batches are those of tests/personalized_edges.py;
tests/test_personalized_edge_premises.py proves on the CPU that each of them sits on the edge it is named for, and that the
slips they are planted against would show in the bits:
  S  the stair: users of 511 .. 1025 items (k_sim_rows' 512-item chunks), items of 511 .. 1030 raters (its 512 look-ahead
     registers and the second pass behind them), items of 1 .. 193 raters (k_fold_rows' trips of 64), one column tile; and
     stairs of 512 and 513 users, with no entry and with exactly one entry behind those registers,
  T  8191 .. 16385 users: 1, 1, 2, 2 and 3 column tiles, the last one a single column at 8193 and 16385,
  B  13 users with a similarity row in 13, 7, 3, 3, 2, 1 and 1 equal blocks, rows without one before, between and after them,
and batches of 1 .. 9 rows for the 4 rows per workgroup of k_fold_rows.  KNNCF_DEBUG_TRACE_DISPATCH's sim_rows / fold_rows
lines are the witness of which path ran and of how the plan cut a batch."""
import importlib
import re

import numpy as np
import pytest

from tests import personalized_edges as pe
from tests import personalized_explain_model as pm
from tests.test_gpu_personalized_explain import _free_device_bytes

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
STREAM = "KNNCF_DEBUG_PERSONALIZED_STREAM"
MAE_TOL = pe.MAE_TOL
SIMS = ["cosine", "jaccard"]
STAIR_IDS = [("all", 0)] + [(group, n) for group, sizes in pe.STAIR_GROUPS.items() for n in sizes]


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _sims(kn, oracle, name):
    return {"cosine": (kn.SIM_COSINE, oracle.SIM_COSINE), "jaccard": (kn.SIM_JACCARD, oracle.SIM_JACCARD)}[name]


def _train(case):
    return pe.stair().train if case == "stair" else pe.tiles(case).train


def _lines(capfd):
    """([(similarity, users, tiles) of every sim_rows line], [rows of every fold_rows line]) since the last look"""
    err = capfd.readouterr().err
    rows = re.findall(r"^knncf-dispatch sim_rows sim=(\w+) users=(\d+) tiles=(\d+)$", err, flags=re.M)
    return [(s, int(u), int(t)) for s, u, t in rows], [int(x) for x in re.findall(r"^knncf-dispatch fold_rows rows=(\d+)$", err, flags=re.M)]


# ---- shared, unchanged state ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def want(oracle):
    """(case, batch name, similarity name) -> (the oracle's MAE, its predictions) of a batch sorted by user, computed once;
    case "stair" or a number of users of case T"""
    models, made = {}, {}

    def get(case, name, batch, sim_name):
        key = (case, name, sim_name)
        if key not in made:
            if case not in models:
                models.clear()  # (one model at a time: the cases are asked for in runs)
                models[case] = oracle.Model(*_train(case))
            osim = {"cosine": oracle.SIM_COSINE, "jaccard": oracle.SIM_JACCARD}[sim_name]
            made[key] = models[case].pipeline(osim, -1).mae(batch.users, batch.items, batch.ratings, True)
        return made[key]

    return get


@pytest.fixture(scope="module")
def stair_engine(kn, oracle):
    """similarity name -> a handle fitted with the stair, at the default workspace"""
    made = {}

    def get(sim_name):
        if sim_name not in made:
            made[sim_name] = kn.Engine(k=10, similarity=_sims(kn, oracle, sim_name)[0]).fit(*pe.stair().train)
        return made[sim_name]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def stair_streamed(kn, stair_engine):
    """similarity name -> the streamed predictions of the stair batch, made once under the hook"""
    made = {}

    def get(sim_name):
        if sim_name not in made:
            b = pe.stair_batch()
            e = stair_engine(sim_name)
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv(STREAM, "1")
                e.reset_timings()
                made[sim_name] = e.predict_batch(kn.PRED_PERSONALIZED, b.users, b.items)
                assert e.timings()["rerank_ms"] > 0  # the streamed rows ran
        return made[sim_name]

    return get


# ---- 1. the stair through the streamed kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,size", STAIR_IDS, ids=[g if g == "all" else f"{g}{n}" for g, n in STAIR_IDS])
@pytest.mark.parametrize("sim_name", SIMS)
def test_stair_streamed(kn, want, stair_engine, stair_streamed, monkeypatch, sim_name, group, size):
    """one id per seam, so that a failure names it: chunkN the rows of the user with N items, passN / foldN the rows on the
    item with N raters; "all" every row of the batch, the MAE, the batch in a shuffled order and single calls"""
    b = pe.stair_batch()
    mae, preds = want("stair", "stair", b, sim_name)
    got = stair_streamed(sim_name)
    if group != "all":
        rows = pe.stair_group_rows(b, group, size)
        assert len(rows) >= 18 and np.array_equal(_bits(got[rows]), _bits(preds[rows]))
        return
    assert np.array_equal(_bits(got), _bits(preds))
    e = stair_engine(sim_name)
    monkeypatch.setenv(STREAM, "1")
    assert abs(e.mae(kn.PRED_PERSONALIZED, b.users, b.items, b.ratings) - mae) <= MAE_TOL
    mixed, perm = b.shuffled(5)
    assert np.array_equal(_bits(e.predict_batch(kn.PRED_PERSONALIZED, mixed.users, mixed.items)), _bits(preds[perm]))
    for n in (1025, 513):
        for j in pe.stair_group_rows(b, "pass", n).tolist():
            assert _bits([e.predict(kn.PRED_PERSONALIZED, int(b.users[j]), int(b.items[j]))])[0] == _bits(preds)[j], (n, j)


@pytest.mark.parametrize("sim_name", SIMS)
@pytest.mark.parametrize("N", pe.SHORT_STAIRS)
def test_second_pass_seam(kn, oracle, monkeypatch, capfd, N, sim_name):
    """stairs of 512 and 513 users: no item, and then exactly one entry of one item, behind k_sim_rows' look-ahead registers"""
    train, b = pe.stair(N).train, pe.short_stair_batch(N)
    mae, preds = oracle.Model(*train).pipeline(_sims(kn, oracle, sim_name)[1], -1).mae(b.users, b.items, b.ratings, True)
    monkeypatch.setenv(STREAM, "1")
    monkeypatch.setenv(TRACE, "1")
    e = kn.Engine(k=10, similarity=_sims(kn, oracle, sim_name)[0]).fit(*train)
    capfd.readouterr()
    got = e.predict_batch(kn.PRED_PERSONALIZED, b.users, b.items)
    assert _lines(capfd) == ([(sim_name, len(np.unique(b.users)) - 1, 1)], [len(b)])
    assert np.array_equal(_bits(got), _bits(preds))
    assert abs(e.mae(kn.PRED_PERSONALIZED, b.users, b.items, b.ratings) - mae) <= MAE_TOL
    e.close()


# ---- 2. the stair through the U x U table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim_name", SIMS)
def test_stair_table_path(kn, want, stair_engine, stair_streamed, monkeypatch, capfd, sim_name):
    b = pe.stair_batch()
    mae, preds = want("stair", "stair", b, sim_name)
    streamed = stair_streamed(sim_name)
    e = stair_engine(sim_name)
    monkeypatch.delenv(STREAM, raising=False)
    monkeypatch.setenv(TRACE, "1")
    e.reset_timings()
    capfd.readouterr()
    got = e.predict_batch(kn.PRED_PERSONALIZED, b.users, b.items)
    assert _lines(capfd) == ([], []) and e.timings()["rerank_ms"] == 0  # below 2048 users, hook unset: no streamed launch
    assert np.array_equal(_bits(got), _bits(preds)) and np.array_equal(_bits(got), _bits(streamed))
    assert abs(e.mae(kn.PRED_PERSONALIZED, b.users, b.items, b.ratings) - mae) <= MAE_TOL


# ---- 3. the column tiles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim_name", SIMS)
@pytest.mark.parametrize("U", pe.TILE_USERS)
def test_tiles(kn, oracle, want, monkeypatch, capfd, U, sim_name):
    b = pe.tile_batch(U)
    mae, preds = want(U, "tiles", b, sim_name)
    monkeypatch.setenv(TRACE, "1")
    e = kn.Engine(k=10, similarity=_sims(kn, oracle, sim_name)[0]).fit(*pe.tiles(U).train)
    assert e.num_users == U
    capfd.readouterr()
    got = e.predict_batch(kn.PRED_PERSONALIZED, b.users, b.items)
    sim_lines, fold_lines = _lines(capfd)
    n_users = len(np.unique(b.users)) - 1  # (all but the unknown user have a row on a train item)
    assert sim_lines == [(sim_name, n_users, pe.TILE_COUNTS[U])] and fold_lines == [len(b)]
    assert np.array_equal(_bits(got), _bits(preds))
    t = e.timings()
    assert t["rerank_ms"] > 0 and t["predict_ms"] > 0
    assert abs(e.mae(kn.PRED_PERSONALIZED, b.users, b.items, b.ratings) - mae) <= MAE_TOL
    mixed, perm = b.shuffled(U)
    assert np.array_equal(_bits(e.predict_batch(kn.PRED_PERSONALIZED, mixed.users, mixed.items)), _bits(preds[perm]))
    e.close()


# ---- 4. the block plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim_name", SIMS)
def test_blocks(kn, oracle, want, stair_engine, monkeypatch, capfd, sim_name):
    train = pe.stair().train
    mixed = pe.block_batch()
    order = np.argsort(mixed.users, kind="stable")
    _, sorted_preds = want("stair", "blocks", mixed.take(order), sim_name)
    preds = np.empty(len(mixed))
    preds[order] = sorted_preds
    n = len(mixed)
    monkeypatch.setenv(STREAM, "1")
    monkeypatch.setenv(TRACE, "1")
    roomy = stair_engine(sim_name)
    capfd.readouterr()
    base = roomy.predict_batch(kn.PRED_PERSONALIZED, mixed.users, mixed.items)
    assert _lines(capfd) == ([(sim_name, 13, 1)], [n])
    assert np.array_equal(_bits(base), _bits(preds))
    for asked in pe.BLOCK_REQUESTS:
        workspace = pe.workspace_for(asked, pe.STAIR_N)
        tight = kn.Engine(k=10, similarity=_sims(kn, oracle, sim_name)[0], workspace_bytes=workspace).fit(*train)
        capfd.readouterr()
        got = tight.predict_batch(kn.PRED_PERSONALIZED, mixed.users, mixed.items)
        sim_lines, fold_lines = _lines(capfd)
        users = pe.BLOCK_USERS_PER_LAUNCH[asked]
        assert sim_lines == [(sim_name, m, 1) for m in users], asked
        assert fold_lines == pe.block_fold_rows(train, mixed, users) and sum(fold_lines) == n and len(fold_lines) == len(users), asked
        assert np.array_equal(_bits(got), _bits(base)) and np.array_equal(_bits(got), _bits(preds)), asked
        free = _free_device_bytes()  # a repeated call of the same shape allocates no device memory
        again = tight.predict_batch(kn.PRED_PERSONALIZED, mixed.users, mixed.items)
        assert _free_device_bytes() >= free and np.array_equal(_bits(again), _bits(got)), asked
        tight.close()


# ---- 5. rows per workgroup of the fold --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim_name", SIMS)
@pytest.mark.parametrize("n", pe.ROW_COUNTS)
def test_row_counts(kn, want, stair_engine, monkeypatch, capfd, n, sim_name):
    b = pe.count_batch(n)
    order = np.argsort(b.users, kind="stable")
    _, sorted_preds = want("stair", f"count{n}", b.take(order), sim_name)
    preds = np.empty(n)
    preds[order] = sorted_preds
    monkeypatch.setenv(STREAM, "1")
    monkeypatch.setenv(TRACE, "1")
    e = stair_engine(sim_name)
    capfd.readouterr()
    got = e.predict_batch(kn.PRED_PERSONALIZED, b.users, b.items)
    sim_lines, fold_lines = _lines(capfd)
    assert fold_lines == [n] and [ln[1] for ln in sim_lines] == [len({int(u) for u, i in zip(b.users, b.items)
                                                                       if u != pe.ABSENT_USER and i != pe.ABSENT_ITEM})]
    assert np.array_equal(_bits(got), _bits(preds))


# ---- 6. the other reader of the rows: k_explain_all behind the same plan ----------------------------------------------------------
@pytest.mark.parametrize("sim_name", SIMS)
@pytest.mark.parametrize("case", ["stair", 16385])
def test_explain_reads_the_same_rows(kn, oracle, want, stair_engine, stair_streamed, case, sim_name):
    if case == "stair":
        b, e, predicted = pe.stair_batch(), stair_engine(sim_name), stair_streamed(sim_name)
    else:
        b = pe.tile_batch(case)
        e = kn.Engine(k=10, similarity=_sims(kn, oracle, sim_name)[0]).fit(*pe.tiles(case).train)
        predicted = e.predict_batch(kn.PRED_PERSONALIZED, b.users, b.items)
    _, preds = want(case, "stair" if case == "stair" else "tiles", b, sim_name)
    rows = pm.PersonalTermModel(oracle, oracle.Model(*_train(case)), _sims(kn, oracle, sim_name)[1]).rows(b.users, b.items)
    raters, sims, devs, counts, sums, got = e.explain_personalized_batch(b.users, b.items, 0)
    assert np.array_equal(_bits(got), _bits(predicted)) and np.array_equal(_bits(got), _bits(preds))
    assert counts.tolist() == [r.count for r in rows]
    assert np.array_equal(_bits(sums), _bits([[r.num, r.den] for r in rows]))
    if case != "stair":
        e.close()


# ---- 7. re-fits: the tile count and the stride of the tile table change ------------------------------------------------------------
@pytest.mark.parametrize("sim_name", SIMS)
def test_refit_across_tile_counts(kn, oracle, want, monkeypatch, capfd, sim_name):
    """3 tiles, then 1 (the stair, streamed under the hook), then 2 with a last tile of one column, on one handle: each fit
    answers as the oracle does, which is what the fresh handles of the tests above answer"""
    monkeypatch.setenv(STREAM, "1")
    monkeypatch.setenv(TRACE, "1")
    e = kn.Engine(k=10, similarity=_sims(kn, oracle, sim_name)[0])
    for case in (16385, "stair", 8193):
        b = pe.stair_batch() if case == "stair" else pe.tile_batch(case)
        mae, preds = want(case, "stair" if case == "stair" else "tiles", b, sim_name)
        e.fit(*_train(case))
        capfd.readouterr()
        got = e.predict_batch(kn.PRED_PERSONALIZED, b.users, b.items)
        sim_lines, fold_lines = _lines(capfd)
        assert [ln[2] for ln in sim_lines] == [1 if case == "stair" else pe.TILE_COUNTS[case]] and fold_lines == [len(b)], case
        assert np.array_equal(_bits(got), _bits(preds)), case
        assert abs(e.mae(kn.PRED_PERSONALIZED, b.users, b.items, b.ratings) - mae) <= MAE_TOL, case
    e.close()
