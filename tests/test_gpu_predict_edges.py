"""The four kNN prediction kernels at their match-count, run and bitmap edges, against the CPU oracle bit for bit, with a witness
of which kernel ran.

k_predict_knn_items, k_predict_knn_rows, k_predict_knn (predict.hip) and k_predict_knn_sweep (ksweep.hip) each spell out the
ordering rule of knn_terms.h themselves: which of a user's neighbours rated the item (probe), those matches in training-file
order (rank), the fp64 left fold over them.  What steers their code paths is the number of matches of a row, the shape of the
runs in the sorted batch and the bitmap width ceil(U / 64); tests/predict_edges.py plants all three and
tests/test_predict_edge_premises.py proves the plants from the data and the oracle alone.  Every cell here sets
KNNCF_DEBUG_TRACE_DISPATCH and asserts the launcher's line — written out below as a literal per case — next to the values.

Every comparison is with oracle.Model(*train).pipeline(sim, k).mae(*test, True): predictions bit for bit, MAEs within MAE_TOL."""
import importlib

import numpy as np
import pytest

from tests import predict_edges as pe

pytestmark = pytest.mark.gpu
MAE_TOL = 1e-9
K = 2048
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
PATH_ENV = {"default": None, "no_lds_bitmaps": "KNNCF_DEBUG_NO_LDS_BITMAPS", "no_item_bitmaps": "KNNCF_DEBUG_NO_ITEM_BITMAPS"}
# ---- the expected dispatch of every case, written out (DESIGN.md "Dispatch by kcap"; kcap = U - 1) -----------------------
GROUPED_FORM = {65: "TR=1 G=4", 66: "TR=2 G=4", 129: "TR=2 G=4", 257: "TR=4 G=2", 258: "TR=5 G=2", 321: "TR=5 G=2",
                322: "TR=8 G=1", 513: "TR=8 G=1"}
BITONIC_M = {65: 128, 66: 128, 129: 128, 257: 256, 258: 512, 321: 512, 322: 512, 513: 512}
GENERAL_CAP = {("no_item_bitmaps", 65): 64, ("no_item_bitmaps", 129): 128, ("no_item_bitmaps", 513): 512,
               ("default", 514): 1024, ("default", 1025): 1024, ("default", 2049): 2048}
SWEEP_CAP = {65: 512, 129: 512, 513: 512, 1025: 1024, 2049: 2048}
SWEEP_CELLS = [(U, "default", "cosine") for U in (65, 129, 513, 1025, 2049)] + [(129, "no_item_bitmaps", "cosine"), (513, "no_item_bitmaps", "cosine"),
                                                                               (129, "default", "jaccard")]


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _sims(kn, oracle, sim):
    return (kn.SIM_COSINE, oracle.SIM_COSINE) if sim == "cosine" else (kn.SIM_JACCARD, oracle.SIM_JACCARD)


def _trace(capfd):
    return [ln[len("knncf-dispatch "):] for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch ")]


def _stage(lines, stage):
    return [ln for ln in lines if ln.startswith(stage + " ")]


# ---- shared, unchanged state: the oracle's model per case, its answers per (case, similarity, k, batch), the fitted handles ----
@pytest.fixture(scope="module")
def models(oracle):
    made = {}

    def get(U):
        if U not in made:
            made[U] = oracle.Model(*pe.case(U).train)
        return made[U]

    return get


@pytest.fixture(scope="module")
def batches():
    """name -> (users, items, ratings) of case U: 'planted' (the planted rows plus two unknown rows) or a run_batch form"""
    made = {}

    def get(U, name):
        if (U, name) not in made:
            b = pe.with_unknowns(pe.case(U)) if name == "planted" else pe.run_batch(pe.case(U), name)
            for a in b:
                a.setflags(write=False)
            made[U, name] = b
        return made[U, name]

    return get


@pytest.fixture(scope="module")
def answers(models, batches):
    """(U, oracle similarity, k, batch name) -> (MAE, predictions) of a fresh pipeline"""
    cache = {}

    def get(U, osim, k, name):
        if (U, osim, k, name) not in cache:
            want, preds = models(U).pipeline(osim, k).mae(*batches(U, name), True)
            preds.setflags(write=False)
            cache[U, osim, k, name] = (want, preds)
        return cache[U, osim, k, name]

    return get


@pytest.fixture(scope="module")
def handles(kn):
    """fitted engines, one per (case, similarity, path), made on first use while the path's environment is set"""
    made = {}
    yield made
    for e in made.values():
        e.close()


def _set_path(monkeypatch, path):
    monkeypatch.setenv(TRACE, "1")
    for env in PATH_ENV.values():
        if env:
            monkeypatch.delenv(env, raising=False)
    if PATH_ENV[path]:
        monkeypatch.setenv(PATH_ENV[path], "1")


def _handle(kn, handles, monkeypatch, U, sim, path):
    _set_path(monkeypatch, path)
    if (U, sim, path) not in handles:
        handles[U, sim, path] = kn.Engine(k=K, similarity=sim).fit(*pe.case(U).train)
    e = handles[U, sim, path]
    assert e.num_users == U
    return e


def _same_bits(got, want, what):
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


def _check_one_k(kn, e, capfd, batch, answer, predict_line, idsort_line, what):
    """predict_batch and mae over the batch: one launch of the expected kernel each, the oracle's bits, its MAE"""
    want, opreds = answer
    capfd.readouterr()
    preds = e.predict_batch(kn.PRED_KNN, batch[0], batch[1])
    mae = e.mae(kn.PRED_KNN, *batch)
    lines = _trace(capfd)
    assert _stage(lines, "predict") == [predict_line] * 2, (what, lines)
    assert not _stage(lines, "sweep"), (what, lines)
    if idsort_line is None:
        assert not _stage(lines, "idsort"), (what, lines)
    else:
        assert set(_stage(lines, "idsort")) <= {idsort_line}, (what, lines)
    _same_bits(preds, opreds, what)
    assert abs(mae - want) <= MAE_TOL, (what, mae, want)
    return preds, lines


def _check_planted(kn, oracle, handles, answers, batches, monkeypatch, capfd, U, path, sim, predict_line, idsort_line):
    ksim, osim = _sims(kn, oracle, sim)
    fresh = (U, ksim, path) not in handles
    e = _handle(kn, handles, monkeypatch, U, ksim, path)
    _, lines = _check_one_k(kn, e, capfd, batches(U, "planted"), answers(U, osim, K, "planted"), predict_line, idsort_line, (U, path, sim))
    if fresh and idsort_line:  # the id-sorted copies are made once, for the first kernel that probes global memory
        assert _stage(lines, "idsort") == [idsort_line], (U, path, lines)


# ---- a. match counts through the item-grouped kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("U,sim", [(U, "cosine") for U in pe.GROUPED_USERS] + [(129, "jaccard")])
def test_match_counts_items_kernel(kn, oracle, handles, answers, batches, monkeypatch, capfd, U, sim):
    _check_planted(kn, oracle, handles, answers, batches, monkeypatch, capfd, U, "default", sim, "predict items " + GROUPED_FORM[U], None)


# ---- b. ... through the row-grouped kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("U,sim", [(U, "cosine") for U in pe.GROUPED_USERS] + [(129, "jaccard")])
def test_match_counts_rows_kernel(kn, oracle, handles, answers, batches, monkeypatch, capfd, U, sim):
    _check_planted(kn, oracle, handles, answers, batches, monkeypatch, capfd, U, "no_lds_bitmaps", sim, "predict rows " + GROUPED_FORM[U],
                   f"idsort bitonic m={BITONIC_M[U]}")


# ---- c. ... through the general kernel: the binary-search probe (CAP = 64, 128, 512), the bitmap probe (CAP = 1024, 1024, 2048) ----
@pytest.mark.parametrize("path,U", list(GENERAL_CAP))
def test_match_counts_general_kernel(kn, oracle, handles, answers, batches, monkeypatch, capfd, path, U):
    _check_planted(kn, oracle, handles, answers, batches, monkeypatch, capfd, U, path, "cosine", f"predict general CAP={GENERAL_CAP[path, U]}", "idsort rank")


# ---- d. ... through the sweep -------------------------------------------------------------------------------------------------------
def _check_sweep(kn, e, capfd, ks, batch, want_of_k, sweep_line, what):
    capfd.readouterr()
    maes, preds = e.mae_sweep(ks, *batch, predictions=True)
    lines = _trace(capfd)
    assert _stage(lines, "sweep") == [sweep_line] and not _stage(lines, "predict"), (what, lines)
    assert preds.shape == (len(ks), len(batch[0]))
    for q, k in enumerate(ks):
        want, opreds = want_of_k(k)
        _same_bits(preds[q], opreds, (what, "k", k))
        assert abs(maes[q] - want) <= MAE_TOL, (what, k, maes[q], want)
    return maes


@pytest.mark.parametrize("U,path,sim", SWEEP_CELLS)
def test_match_counts_sweep(kn, oracle, handles, answers, batches, monkeypatch, capfd, U, path, sim):
    ksim, osim = _sims(kn, oracle, sim)
    e = _handle(kn, handles, monkeypatch, U, ksim, path)
    batch = batches(U, "planted")
    sweep_line = f"sweep CAP={SWEEP_CAP[U]} bits={int(path == 'default')}"
    assert sweep_line == {(65, "default"): "sweep CAP=512 bits=1", (129, "default"): "sweep CAP=512 bits=1", (513, "default"): "sweep CAP=512 bits=1",
                          (1025, "default"): "sweep CAP=1024 bits=1", (2049, "default"): "sweep CAP=2048 bits=1",
                          (129, "no_item_bitmaps"): "sweep CAP=512 bits=0", (513, "no_item_bitmaps"): "sweep CAP=512 bits=0"}[U, path]
    second = kn.Engine(k=K, similarity=ksim).fit(*pe.case(U).train)  # the same answers by set_k + mae, one k at a time
    loop = {}
    try:
        for ks in pe.sweep_ks(U - 1):
            maes = _check_sweep(kn, e, capfd, ks, batch, lambda k: answers(U, osim, k, "planted"), sweep_line, (U, path, sim, len(ks)))
            for k in ks:
                if k not in loop:
                    second.set_k(k)
                    loop[k] = second.mae(kn.PRED_KNN, *batch)
            assert np.array_equal(_bits(maes), _bits([loop[k] for k in ks])), (U, path, sim, len(ks))
    finally:
        second.close()


# ---- e. run structure -----------------------------------------------------------------------------------------------------------
def _check_unknown_rows(models, U, batch, preds, what):
    """an unknown user's row is the global average whatever its item; a known user's row on an unknown item is the user's mean"""
    c, m = pe.case(U), models(U)
    known_user, known_item = batch[0] <= U, np.isin(batch[1], c.train[1])
    assert (~known_user).sum() >= 3 and (known_user & ~known_item).sum() >= 2, what
    _same_bits(preds[~known_user], np.full(int((~known_user).sum()), m.average()), (what, "unknown users"))
    rows = np.flatnonzero(known_user & ~known_item)
    _same_bits(preds[rows], [m.users_avg(int(u)) for u in batch[0][rows]], (what, "unknown items"))


@pytest.mark.parametrize("U", pe.RUN_USERS)
def test_runs_items_kernel(kn, oracle, models, handles, answers, batches, monkeypatch, capfd, U):
    e = _handle(kn, handles, monkeypatch, U, kn.SIM_COSINE, "default")
    form = "items " + GROUPED_FORM[U]
    assert form == {65: "items TR=1 G=4", 257: "items TR=4 G=2", 513: "items TR=8 G=1"}[U]
    batch = batches(U, form)
    preds, _ = _check_one_k(kn, e, capfd, batch, answers(U, oracle.SIM_COSINE, K, form), "predict " + form, None, (U, form))
    _check_unknown_rows(models, U, batch, preds, (U, form))


@pytest.mark.parametrize("U", pe.RUN_USERS)
def test_runs_rows_kernel(kn, oracle, models, handles, answers, batches, monkeypatch, capfd, U):
    e = _handle(kn, handles, monkeypatch, U, kn.SIM_COSINE, "no_lds_bitmaps")
    form = "rows " + GROUPED_FORM[U]
    batch = batches(U, form)
    preds, _ = _check_one_k(kn, e, capfd, batch, answers(U, oracle.SIM_COSINE, K, form), "predict " + form, f"idsort bitonic m={BITONIC_M[U]}", (U, form))
    _check_unknown_rows(models, U, batch, preds, (U, form))


@pytest.mark.parametrize("U", pe.RUN_USERS)
def test_runs_sweep(kn, oracle, models, handles, answers, batches, monkeypatch, capfd, U):
    """the sweep walks the same item-sorted 64-row chunks and runs; k on both sides of the first trip, the last trip and the list's end"""
    e = _handle(kn, handles, monkeypatch, U, kn.SIM_COSINE, "default")
    form = "items " + GROUPED_FORM[U]
    batch = batches(U, form)
    kcap = U - 1
    ks = sorted({1, 63, 64, 65, kcap - 1, kcap, kcap + 7})
    capfd.readouterr()
    maes, preds = e.mae_sweep(ks, *batch, predictions=True)
    assert _stage(_trace(capfd), "sweep") == ["sweep CAP=512 bits=1"], (U, form)
    for q, k in enumerate(ks):
        want, opreds = answers(U, oracle.SIM_COSINE, k, form)
        _same_bits(preds[q], opreds, (U, form, "k", k))
        assert abs(maes[q] - want) <= MAE_TOL, (U, form, k)
        _check_unknown_rows(models, U, batch, preds[q], (U, form, "k", k))


# ---- f. rows another shard owns -----------------------------------------------------------------------------------------------------
def test_two_shards_partition_the_run_batch(kn, pkg, oracle, answers, batches, monkeypatch, capfd):
    """the protocol of test_gpu_parity.test_two_shards_on_one_gpu_equal_single_engine (view, exchange by device copy, commit):
    each shard's kernel sees its own rows only, so the planted runs are cut differently on either one"""
    import torch

    _set_path(monkeypatch, "default")
    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    U, form = 129, "items TR=2 G=4"
    c, batch = pe.case(U), batches(129, "items TR=2 G=4")
    want, opreds = answers(U, oracle.SIM_COSINE, K, form)
    dev = torch.device("cuda", 0)
    tr = tuple(torch.from_numpy(np.array(a)).to(dev) for a in c.train)
    te = tuple(torch.from_numpy(np.array(a)).to(dev) for a in batch)
    engines = [kn.Engine(k=K, shard_rank=r, shard_count=2) for r in range(2)]
    try:
        views = []
        for e in engines:
            e.fit_device(*tr)
            views.append(sharded.DeviceEngineAdapter(e, dev).shard_tensors())
        assert views[0]["user_range"][1] == views[1]["user_range"][0]
        for me, other in ((0, 1), (1, 0)):
            ulo, uhi = views[other]["user_range"]
            for key in ("user_avg", "user_norm"):
                views[me][key][ulo:uhi] = views[other][key][ulo:uhi]
        torch.cuda.synchronize()
        total, count, mine = 0.0, 0, []
        for e in engines:
            e.shard_commit()
            out = torch.full((len(batch[0]),), float("nan"), dtype=torch.float64, device=dev)
            capfd.readouterr()
            s, n = e.mae_device(kn.PRED_KNN, *te, pred_out=out)
            assert _stage(_trace(capfd), "predict") == ["predict items TR=2 G=4"]
            out = out.cpu().numpy()
            assert n == int((~np.isnan(out)).sum()) > 0
            total += s
            count += n
            mine.append(out)
    finally:
        for e in engines:
            e.close()
    owned = np.stack([~np.isnan(p) for p in mine])
    assert (owned.sum(axis=0) == 1).all() and count == len(batch[0])  # the owned rows partition the batch
    assert owned[0][batch[0] > U].all()  # (unknown users belong to shard 0)
    _same_bits(np.where(owned[0], mine[0], mine[1]), opreds, "shards")
    assert abs(total / count - want) <= MAE_TOL, (total / count, want)
