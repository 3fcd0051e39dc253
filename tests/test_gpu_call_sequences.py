"""Random call sequences on ONE handle against the stateful model of tests/call_sequences.py (what the sequences can tell
apart: tests/test_call_sequence_premises.py).  Each family's own test checks what its call leaves in the handle on a fresh
handle; here the clauses of include/knncf.h are composed: after every op the ids are == and the floats bit-equal to the
model's, a refused call leaves no trace, a read-only call leaves the knncf_neighbors_save bytes alone, a checkpoint carries the
memo history to a second handle in the middle of a sequence, and one handle lives through five fits of very different
shapes.  The mae scalars are compared within MAE_TOL of test_gpu_handle_reuse; the predictions behind them in bits."""
import importlib
import shutil
import os

import numpy as np
import pytest

from tests import call_sequences as cs
from tests.test_gpu_similarity_batch import _table

pytestmark = pytest.mark.gpu
SIMS = ("cosine", "jaccard")
MEMO = [(case, sim) for case in cs.MEMO_CASES for sim in SIMS]
MEMO_IDS = [f"{case.name}-{sim}" for case, sim in MEMO]


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    assert cs.MAE_TOL == 1e-9 and (mod.OK, mod.E_INVALID, mod.E_UNSUPPORTED) == (cs.OK, cs.E_INVALID, cs.E_UNSUPPORTED)
    assert (mod.PRED_BASELINE, mod.PRED_KNN, mod.PRED_PERSONALIZED) == (cs.PRED_BASELINE, cs.PRED_KNN, cs.PRED_PERSONALIZED)
    return mod


def _ksim(kn, sim):
    return {"cosine": kn.SIM_COSINE, "jaccard": kn.SIM_JACCARD}[sim]


def _step(player, model, j, op, tmp_path, what, table=None):
    """op j on the handle and on its model; returns the handle's defined checkpoint bytes afterwards when `table` (those
    before the op) is given"""
    got, want = player.play(op), model.call(op)
    assert cs.same(got, want), f"{what} op {j}: {op!r}"
    if table is None:
        return None
    after = _table(player.e, tmp_path, "state.bin")
    if cs.is_read_only(op.kind):
        assert after == table, f"{what} op {j} is read-only and changed the checkpoint: {op!r}"
    return after


@pytest.mark.parametrize("case, sim", MEMO, ids=MEMO_IDS)
def test_memo_sequences(kn, oracle, tmp_path, case, sim):
    ops = case.ops(oracle)
    model = case.model(oracle, sim)
    e = kn.Engine(k=case.k, similarity=_ksim(kn, sim)).fit(*case.train())
    player = cs.Player(kn, e, tmp_path, "e", case.train())
    table = _table(e, tmp_path, "state.bin")
    for j, op in enumerate(ops):
        table = _step(player, model, j, op, tmp_path, case.name, table)
    # a fresh handle that replays only what the model says the handle keeps: the same defined checkpoint bytes
    f = kn.Engine(k=case.k, similarity=_ksim(kn, sim)).fit(*case.train())
    replay = cs.Player(kn, f, tmp_path, "f", case.train())
    for op in ops:
        if not cs.is_read_only(op.kind) or op.kind == "neighbors_save":
            replay.play(op)
    assert _table(f, tmp_path, "replay.bin") == table, case.name
    f.close()
    e.close()


@pytest.mark.parametrize("case, sim", MEMO, ids=MEMO_IDS)
def test_checkpoint_mid_sequence(kn, oracle, tmp_path, case, sim):
    """save at op n / 2, load into a second handle fitted on the same rows: both finish the sequence against their models"""
    ops = case.ops(oracle)
    half = len(ops) // 2
    model = case.model(oracle, sim)
    e = kn.Engine(k=case.k, similarity=_ksim(kn, sim)).fit(*case.train())
    first = cs.Player(kn, e, tmp_path, "e", case.train())
    for j, op in enumerate(ops[:half]):
        _step(first, model, j, op, tmp_path, case.name)
    path = str(tmp_path / "half.nbr")
    e.neighbors_save(path)
    e2 = kn.Engine(k=model.k, similarity=_ksim(kn, sim)).fit(*model.train)
    e2.neighbors_load(path)
    model2 = model.replica()
    second = cs.Player(kn, e2, tmp_path, "e2", model.train)
    if os.path.exists(first.path):  # the sequence's own checkpoint, should its load come in the second half
        shutil.copy(first.path, second.path)
    for j, op in enumerate(ops[half:], half):
        _step(first, model, j, op, tmp_path, case.name + " first handle")
        _step(second, model2, j, op, tmp_path, case.name + " second handle")
    e.close()
    e2.close()


_expected = {}


def _life_expected(oracle, sim, life):
    """the model's answers of one life (the oracle on the CURRENT fit), computed once per similarity"""
    if (sim, life) not in _expected:
        fit, k0, _ = cs.LIVES[life]
        _expected[sim, life] = cs.play_on_model(cs.HandleModel(oracle, fit.train, cs.sim_of(oracle, sim), k0), cs.life_ops(oracle, life))
    return _expected[sim, life]


@pytest.mark.parametrize("variant", ["cosine", "jaccard", "no_item_bitmaps", "small_workspace"])
def test_handle_lives(kn, oracle, tmp_path, monkeypatch, variant):
    """one handle through the fits A (300 users), B (2 100 users: the streamed Personalized path, k = 1000 and 10), C (a memo fit:
    everything shrinks, short rows, the Personalized cosine refused), D (A's rows under large raw ids) and A again, each life a
    shuffled pass over every call kind, family and predictor.  After each life a fresh handle on the same rows repeats the
    life's kNN predictions bit for bit."""
    sim = "jaccard" if variant == "jaccard" else "cosine"
    if variant == "no_item_bitmaps":
        monkeypatch.setenv("KNNCF_DEBUG_NO_ITEM_BITMAPS", "1")
    workspace = cs.LIFE_WORKSPACE if variant == "small_workspace" else 0
    e = kn.Engine(k=300, similarity=_ksim(kn, sim), workspace_bytes=workspace)
    player = cs.Player(kn, e, tmp_path, "e")
    for life, (fit, k0, _) in enumerate(cs.LIVES):
        ops = cs.life_ops(oracle, life)
        want = _life_expected(oracle, sim, life)
        k = k0
        for j, op in enumerate(ops):
            assert cs.same(player.play(op), want[j]), f"life {life} ({fit.name}) op {j}: {op!r}"
            k = op.args[0] if op.kind == "set_k" else k
        rows = [op.args[1:3] for op in ops if op.kind in ("predict_batch", "mae") and op.args[0] == cs.PRED_KNN]
        users, items = (np.concatenate([r[c] for r in rows]) for c in (0, 1))
        if (np.unique(fit.train[0], return_counts=True)[1] <= 4).any():
            e.reset_neighbors()  # (a <= 4-rating fit: the handle's memo history is not a fresh handle's)
        f = kn.Engine(k=k, similarity=_ksim(kn, sim)).fit(*fit.train)
        assert cs.same(e.predict_batch(kn.PRED_KNN, users, items), f.predict_batch(kn.PRED_KNN, users, items)), f"life {life} ({fit.name})"
        f.close()
    e.close()
