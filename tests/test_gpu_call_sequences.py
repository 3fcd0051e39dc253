"""Random call sequences on ONE handle against the stateful model of tests/call_sequences.py (what the sequences can tell
apart: tests/test_call_sequence_premises.py).  Each family's own test checks what its call leaves in the handle on a fresh
handle; here the clauses of include/knncf.h are composed: after every op the ids are == and the floats bit-equal to the
model's, a refused call leaves no trace, a read-only call leaves the knncf_neighbors_save bytes alone, the users with a built
list are the model's, a checkpoint carries the memo history to a second handle in the middle of a sequence, and one handle
lives through five fits of very different shapes.  The sequences hold knncf_append and knncf_amend, which replace the fit and
keep lists — the amend also where the fit SHRINKS by a user or an item, on a handle whose scratch only grows —, the entered
calls, which build every missing list, with and without removals, and the bystander calls of all three families, which must
only read.  The mae scalars are compared within MAE_TOL of test_gpu_handle_reuse; the predictions behind them in bits."""
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
    assert (mod.E_NONFINITE, mod.E_DUPLICATE, mod.E_STATE) == (cs.E_NONFINITE, cs.E_DUPLICATE, cs.E_STATE)
    assert (mod.PRED_BASELINE, mod.PRED_KNN, mod.PRED_PERSONALIZED) == (cs.PRED_BASELINE, cs.PRED_KNN, cs.PRED_PERSONALIZED)
    assert mod.APPEND_MAX_CHANGERS == cs.APPEND_MAX_CHANGERS
    return mod


def _ksim(kn, sim):
    return {"cosine": kn.SIM_COSINE, "jaccard": kn.SIM_JACCARD}[sim]


def _built(table, order):
    """the raw ids with a build number in a parsed checkpoint; order: the fit's users in set order (dense index -> raw id)"""
    assert len(table["seq"]) == len(order)
    return sorted(int(u) for u, s in zip(order, table["seq"]) if s >= 0)


def _same_built(table, built, order, what):
    got = _built(table, order)
    assert got == sorted(built), f"{what}: the handle has built {got}, the model {sorted(built)}"


def _step(player, model, j, op, tmp_path, what, table=None):
    """op j on the handle and on its model; returns the handle's defined checkpoint bytes afterwards when `table` (those
    before the op) is given, having compared the users that have a list with the model's"""
    got, want = player.play(op), model.call(op)
    assert cs.same(got, want), f"{what} op {j}: {op!r}"
    if op.kind in cs.REFITS:  # (a refused or trivial call included: the numbers stay)
        _same_counts(player.e, model, f"{what} op {j}: {op!r}")
    if table is None:
        return None
    after = _table(player.e, tmp_path, "state.bin")
    # (a single entered call whose query is refused has still built the missing lists: its definition is not empty)
    # (... and the trivial amend "touches nothing": a call that may refit and whose definition is empty)
    if cs.is_read_only(op.kind) or (isinstance(want, cs.Refused) and not model.definition) or (op.kind in cs.REFITS and model.definition == []):
        assert after == table, f"{what} op {j} is read-only, refused or trivial and changed the checkpoint: {op!r}"
    _same_built(after, model.built, model.m.user_iteration_order().tolist(), f"{what} op {j}: {op!r}")
    return after


def _same_counts(e, model, what):
    """num_users / num_items of the handle against the model's fit: the only numbers that go DOWN on a living handle"""
    assert (e.num_users, e.num_items) == (len(model.known_users), len(model.known_items)), what


def _replay(player, op, definition):
    """what a handle that is independent of the code under test plays for an op: nothing for a read-only one, the older calls
    that define it for an append or an amend (fit(aug), neighbors_batch(K); nothing for a refused or a trivial one) and an entered
    call (neighbors_batch(M)) — K and M are the model's — and the op itself otherwise"""
    if definition is not None:
        for x in definition:
            out = player.play(x)
            assert not isinstance(out, cs.Refused), (op, x)
    elif not cs.is_read_only(op.kind) or op.kind == "neighbors_save":
        player.play(op)


@pytest.mark.parametrize("case, sim", MEMO, ids=MEMO_IDS)
def test_memo_sequences(kn, oracle, tmp_path, case, sim):
    ops = case.ops(oracle)
    model = case.model(oracle, sim)
    e = kn.Engine(k=case.k, similarity=_ksim(kn, sim)).fit(*case.train())
    player = cs.Player(kn, e, tmp_path, "e", case.train())
    table = _table(e, tmp_path, "state.bin")
    definitions = []
    for j, op in enumerate(ops):
        table = _step(player, model, j, op, tmp_path, case.name, table)
        definitions.append(model.definition)
        assert (model.definition is not None) == (op.kind in cs.REFITS or op.kind in cs.ENTERED), op
    # a fresh handle that replays only what the model says the handle keeps: the same defined checkpoint bytes
    f = kn.Engine(k=case.k, similarity=_ksim(kn, sim)).fit(*case.train())
    replay = cs.Player(kn, f, tmp_path, "f", case.train())
    for op, definition in zip(ops, definitions):
        _replay(replay, op, definition)
    assert _table(f, tmp_path, "replay.bin") == table, case.name
    f.close()
    e.close()


def _second_handle(kn, model, sim, path, tmp_path, first):
    """a handle fitted on the model's rows as they stand (the aug after an append) that loads the checkpoint at `path`, with
    the model of its state"""
    e2 = kn.Engine(k=model.k, similarity=_ksim(kn, sim)).fit(*model.train)
    e2.neighbors_load(path)
    second = cs.Player(kn, e2, tmp_path, "e2", model.train)
    if os.path.exists(first.path):  # the sequence's own checkpoint, should its load come later
        shutil.copy(first.path, second.path)
    return e2, second, model.replica()


@pytest.mark.parametrize("case, sim", MEMO, ids=MEMO_IDS)
def test_checkpoint_mid_sequence(kn, oracle, tmp_path, case, sim):
    """save at op n / 2, load into a second handle fitted on the rows as they stand then: both finish the sequence against their
    models"""
    ops = case.ops(oracle)
    half = len(ops) // 2
    model = case.model(oracle, sim)
    e = kn.Engine(k=case.k, similarity=_ksim(kn, sim)).fit(*case.train())
    first = cs.Player(kn, e, tmp_path, "e", case.train())
    for j, op in enumerate(ops[:half]):
        _step(first, model, j, op, tmp_path, case.name)
    path = str(tmp_path / "half.nbr")
    e.neighbors_save(path)
    e2, second, model2 = _second_handle(kn, model, sim, path, tmp_path, first)
    for j, op in enumerate(ops[half:], half):
        _step(first, model, j, op, tmp_path, case.name + " first handle")
        _step(second, model2, j, op, tmp_path, case.name + " second handle")
    e.close()
    e2.close()


@pytest.mark.parametrize("sim", SIMS)
def test_checkpoint_around_an_append(kn, oracle, tmp_path, sim):
    """a checkpoint saved before an append no longer loads afterwards (KNNCF_E_STATE: the fit is another one) and the refused
    load leaves the handle as it was; one saved after the append loads into a fresh handle fitted on aug, and both handles
    finish the sequence.  The append is the first of the sequence that meets built lists."""
    case = cs.MEMO_CASES[0]
    ops = case.ops(oracle)
    probe = case.model(oracle, sim)
    at = next(j for j, op in enumerate(ops) if not isinstance(probe.call(op), cs.Refused) and op.kind == "append" and probe.appends[-1]["built"])
    model = case.model(oracle, sim)
    e = kn.Engine(k=case.k, similarity=_ksim(kn, sim)).fit(*case.train())
    first = cs.Player(kn, e, tmp_path, "e", case.train())
    for j, op in enumerate(ops[:at]):
        _step(first, model, j, op, tmp_path, case.name)
    before = str(tmp_path / "before.nbr")
    e.neighbors_save(before)
    table = _step(first, model, at, ops[at], tmp_path, case.name, _table(e, tmp_path, "state.bin"))
    with pytest.raises(kn.KnncfError) as refused:
        e.neighbors_load(before)
    assert refused.value.status == kn.E_STATE
    assert _table(e, tmp_path, "state.bin") == table
    after = str(tmp_path / "after.nbr")
    e.neighbors_save(after)
    if os.path.exists(first.path):
        os.remove(first.path)  # (the sequence's own checkpoint is of the fit before the append: its load lies before `at`)
    e2, second, model2 = _second_handle(kn, model, sim, after, tmp_path, first)
    assert _table(e2, tmp_path, "second.bin") == table
    for j, op in enumerate(ops[at + 1:], at + 1):
        table = _step(first, model, j, op, tmp_path, case.name + " first handle", table)
        _step(second, model2, j, op, tmp_path, case.name + " second handle")
    assert _table(e2, tmp_path, "second.bin") == table
    e.close()
    e2.close()


_expected = {}


def _life_expected(oracle, sim, life):
    """the model's answers of one life (the oracle on the CURRENT fit), computed once per similarity: (answers, {op index of an
    accepted append or amend: (built users, the users of the fit in set order, (num_users, num_items)) after it}, the train set
    at the end of the life)"""
    if (sim, life) not in _expected:
        fit, k0, _ = cs.LIVES[life]
        model = cs.HandleModel(oracle, fit.train, cs.sim_of(oracle, sim), k0)
        out, appended = [], {}
        for j, op in enumerate(cs.life_ops(oracle, life)):
            out.append(model.call(op))
            if op.kind in cs.REFITS and not isinstance(out[-1], cs.Refused):
                appended[j] = (sorted(model.built), model.m.user_iteration_order().tolist(), (len(model.known_users), len(model.known_items)))
        _expected[sim, life] = (out, appended, model.train)
    return _expected[sim, life]


@pytest.mark.parametrize("variant", ["cosine", "jaccard", "no_item_bitmaps", "small_workspace"])
def test_handle_lives(kn, oracle, tmp_path, monkeypatch, variant):
    """one handle through the fits A (300 users), B (2 100 users: the streamed Personalized path, k = 1000 and 10), C (a memo fit:
    everything shrinks, short rows, the Personalized cosine refused), D (A's rows under large raw ids) and A again, each life a
    shuffled pass over every call kind, family and predictor with appends and amends among them: the fit grows within a life, and
    with an amend that takes a user or an item out it shrinks under scratch buffers of the larger size.  After every accepted
    append and amend the users with a list, num_users and num_items are the model's.  After each life a fresh handle on the rows as they stand then repeats the
    life's kNN predictions bit for bit."""
    sim = "jaccard" if variant == "jaccard" else "cosine"
    if variant == "no_item_bitmaps":
        monkeypatch.setenv("KNNCF_DEBUG_NO_ITEM_BITMAPS", "1")
    workspace = cs.LIFE_WORKSPACE if variant == "small_workspace" else 0
    e = kn.Engine(k=300, similarity=_ksim(kn, sim), workspace_bytes=workspace)
    player = cs.Player(kn, e, tmp_path, "e")
    for life, (fit, k0, _) in enumerate(cs.LIVES):
        ops = cs.life_ops(oracle, life)
        want, appended, train = _life_expected(oracle, sim, life)
        k = k0
        for j, op in enumerate(ops):
            assert cs.same(player.play(op), want[j]), f"life {life} ({fit.name}) op {j}: {op!r}"
            k = op.args[0] if op.kind == "set_k" else k
            if j in appended:
                _same_built(_table(e, tmp_path, "life.bin"), *appended[j][:2], f"life {life} ({fit.name}) op {j}: {op!r}")
                assert (e.num_users, e.num_items) == appended[j][2], f"life {life} ({fit.name}) op {j}: {op!r}"
        # the fit holds rows that an append or an amend brought (the row count alone may go either way now: amends take rows out)
        was, now = set(zip(fit.train[0].tolist(), fit.train[1].tolist())), set(zip(train[0].tolist(), train[1].tolist()))
        assert appended and len(now - was) > 0, life
        assert any(op.kind == "amend" and op.shape in cs.AMEND_SHRINKS and j in appended for j, op in enumerate(ops)), life
        rows = [op.args[1:3] for op in ops if op.kind in ("predict_batch", "mae") and op.args[0] == cs.PRED_KNN]
        users, items = (np.concatenate([r[c] for r in rows]) for c in (0, 1))
        if (np.unique(train[0], return_counts=True)[1] <= 4).any():
            e.reset_neighbors()  # (a <= 4-rating fit: the handle's memo history is not a fresh handle's)
        f = kn.Engine(k=k, similarity=_ksim(kn, sim)).fit(*train)
        assert cs.same(e.predict_batch(kn.PRED_KNN, users, items), f.predict_batch(kn.PRED_KNN, users, items)), f"life {life} ({fit.name})"
        f.close()
    e.close()


def _first_amend(oracle, case, sim, shape):
    """the index of the first amend of `shape` in the case's sequence that meets built lists (None: there is none)"""
    probe = case.model(oracle, sim)
    for j, op in enumerate(case.ops(oracle)):
        out = probe.call(op)
        if op.kind == "amend" and op.shape == shape and not isinstance(out, cs.Refused) and probe.appends[-1]["built"]:
            return j
    return None


@pytest.mark.parametrize("sim", SIMS)
def test_checkpoint_around_an_amend(kn, oracle, tmp_path, sim):
    """a checkpoint saved before the amend with which a user LEAVES no longer loads afterwards (KNNCF_E_STATE: the fit is another
    one) and the refused load leaves the handle as it was; one saved after it loads into a fresh handle fitted on aug — whose dense
    indices are shifted by the user that left — and both handles finish the sequence.  The amend is the first `leaver` of a memo
    sequence that meets built lists."""
    case, at = next((c, j) for c in cs.MEMO_CASES for j in [_first_amend(oracle, c, sim, "leaver")] if j is not None)
    ops = case.ops(oracle)
    model = case.model(oracle, sim)
    e = kn.Engine(k=case.k, similarity=_ksim(kn, sim)).fit(*case.train())
    first = cs.Player(kn, e, tmp_path, "e", case.train())
    for j, op in enumerate(ops[:at]):
        _step(first, model, j, op, tmp_path, case.name)
    before = str(tmp_path / "before.nbr")
    e.neighbors_save(before)
    users = len(model.known_users)
    table = _step(first, model, at, ops[at], tmp_path, case.name, _table(e, tmp_path, "state.bin"))
    assert model.appends[-1]["left_users"] == 1 and e.num_users == users - 1
    with pytest.raises(kn.KnncfError) as refused:
        e.neighbors_load(before)
    assert refused.value.status == kn.E_STATE
    assert _table(e, tmp_path, "state.bin") == table
    after = str(tmp_path / "after.nbr")
    e.neighbors_save(after)
    if os.path.exists(first.path):
        os.remove(first.path)  # (the sequence's own checkpoint is of the fit before the amend: its load lies before `at`)
    e2, second, model2 = _second_handle(kn, model, sim, after, tmp_path, first)
    assert _table(e2, tmp_path, "second.bin") == table
    for j, op in enumerate(ops[at + 1:], at + 1):
        table = _step(first, model, j, op, tmp_path, case.name + " first handle", table)
        _step(second, model2, j, op, tmp_path, case.name + " second handle")
    assert _table(e2, tmp_path, "second.bin") == table
    e.close()
    e2.close()


def _one_of_each(oracle, model, seed):
    """one op of every kind but fit, set_k, the checkpoint and the calls that change the fit, drawn on the model's fit: the
    queries of all three families, both entered `with` forms with removals, explain, recommend and the Personalized kinds"""
    rng = np.random.default_rng(seed)
    d = cs._Draw(rng, model, [model.k], [2, 3], [cs.Fit("same", model.train)])
    kinds = [k for k in cs.KINDS if k not in cs.CHECKPOINT + cs.REFITS + ("fit", "set_k", "reset_neighbors", "mae_sweep")]
    slots = [(k, None) for k in kinds if k not in cs.BYSTANDER] + [(k, fam) for k in cs.BYSTANDER for fam in cs.BYSTANDER_FAMILIES]
    slots += [("entered_with", "removed"), ("entered_with_batch", "removed"), ("predict_batch", cs.PRED_PERSONALIZED),
              ("recommend_batch", cs.PRED_PERSONALIZED), ("recommend", cs.PRED_KNN), ("mae", cs.PRED_KNN)]
    slots += [(f"{w}_q", (fam, cs.PRED_KNN)) for w in cs.QUERY_WHATS for fam in cs.FAMILIES]
    ops = [d.op(kind, variant) for kind, variant in slots]
    return ops + [cs.Op("mae_sweep", ([2, model.k], *d.rows(6)))]  # (last: it drops the memo)


@pytest.mark.parametrize("variant", ["cosine", "jaccard", "no_item_bitmaps", "small_workspace"])
def test_shrunken_fit_matches_a_fresh_handle(kn, oracle, tmp_path, monkeypatch, variant):
    """knncf.h "Amend": "leaves the fit: num_users shrinks" / "num_items shrinks", and "every later call on the handle answers bit
    for bit as a handle on which knncf_fit(aug) was called" — on a handle whose every scratch buffer has the size of the LARGER
    fit.  A memo fit of 40 users and 12 items, with a newcomer's lone item: every list built and one op of every kind played;
    then one user and the lone item are amended away in two calls; then one op of every kind again, against the model and
    against a fresh handle fitted on aug: ids equal, floats bit-equal, and the checkpoint bytes those of the fresh handle after
    neighbors_batch over the same users."""
    sim = "jaccard" if variant == "jaccard" else "cosine"
    if variant == "no_item_bitmaps":
        monkeypatch.setenv("KNNCF_DEBUG_NO_ITEM_BITMAPS", "1")
    workspace = cs.LIFE_WORKSPACE if variant == "small_workspace" else 0
    case = cs.MEMO_CASES[2]
    base = case.train()
    users, counts = np.unique(base[0], return_counts=True)
    items = np.unique(base[1])
    assert len(users) == 40 and len(items) == 12
    new_user, lone = cs.NEWCOMER + 1, cs.APPEND_ITEM + 1
    mine = np.append(items[:5], lone).astype(np.int32)
    train = (np.concatenate([base[0], np.full(6, new_user)]).astype(np.int32), np.concatenate([base[1], mine]).astype(np.int32),
             np.concatenate([base[2], [4.0, 2.0, 5.0, 3.0, 1.0, 4.5]]))
    leaver = int(users[counts <= 4][0])
    gone = train[1][train[0] == leaver]
    model = cs.HandleModel(oracle, train, cs.sim_of(oracle, sim), case.k)
    e = kn.Engine(k=case.k, similarity=_ksim(kn, sim), workspace_bytes=workspace).fit(*train)
    player = cs.Player(kn, e, tmp_path, "e", train)
    everybody = cs.Op("neighbors_batch", (np.asarray(sorted(model.known_users), np.int32),))
    for j, op in enumerate([everybody] + _one_of_each(oracle, model, 1) + [everybody]):
        _step(player, model, j, op, tmp_path, "the larger fit")
    none, nof = np.empty(0, np.int32), np.empty(0)
    shrinks = [cs.Op("amend", (np.full(len(gone), leaver), gone, none, none, nof), shape="leaver"),
               cs.Op("amend", (np.asarray([new_user]), np.asarray([lone]), none, none, nof), shape="lone_item")]
    table = _table(e, tmp_path, "state.bin")
    for j, op in enumerate(shrinks):
        if j:  # (a user that leaves is a plain refit: every list again, so that the second call has lists to carry)
            table = _step(player, model, j, cs.Op("neighbors_batch", (np.asarray(sorted(model.known_users), np.int32),)), tmp_path, "between", table)
        table = _step(player, model, j, op, tmp_path, "the shrinking amends", table)
    assert [(a["left_users"], a["left_items"]) for a in model.appends] == [(1, 0), (0, 1)]
    assert (e.num_users, e.num_items) == (40, 12) and leaver not in model.known_users and lone not in model.known_items
    if sim == "jaccard":
        assert model.appends[1]["carried"] >= 1 and not model.appends[1]["plain"]  # the second call carries: K is not empty
    # a fresh handle on aug in the state the header defines: fit(aug), neighbors_batch(K)
    f = kn.Engine(k=case.k, similarity=_ksim(kn, sim), workspace_bytes=workspace).fit(*model.train)
    fresh = cs.Player(kn, f, tmp_path, "f", model.train)
    for x in model.definition[1:]:
        fresh.play(x)
    assert _table(f, tmp_path, "fresh.bin") == table
    for j, op in enumerate(_one_of_each(oracle, model, 2)):
        got, want = player.play(op), model.call(op)
        assert cs.same(got, want), f"the shrunken fit op {j}: {op!r}"
        assert cs.same(got, fresh.play(op)), f"the shrunken fit against a fresh handle, op {j}: {op!r}"
        assert _table(e, tmp_path, "state.bin") == _table(f, tmp_path, "fresh.bin"), f"the shrunken fit op {j}: {op!r}"
    e.close()
    f.close()
