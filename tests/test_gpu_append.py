"""knncf_append on the GPU (csrc/append.hip): new ratings go into the fit and the kNN lists they cannot change are kept.  Every
answer is compared bit for bit with the oracle on aug = train ++ the rows; the handle's state (the parsed knncf_neighbors_save
file: header with the call counter, list lengths, build numbers, every built list) with a twin engine that ran fit(aug) and
neighbors_batch over the oracle's K in ascending raw id — existing code paths only.  The inputs are those of
tests/append_cases.py (tests/test_append_premises.py shows what they reach and that the S-rule holds).  The `knncf-dispatch
append` line of KNNCF_DEBUG_TRACE_DISPATCH says what a call carried and whether the table moved."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import append_cases as ac
from tests import bystander_cases as bc
from tests import update_entered_cases as uc
from tests.bystander_cases import NEW_ITEM, _users
from tests.query_helpers import UNKNOWN_ITEM, _bits
from tests.test_gpu_similarity_batch import _table

pytestmark = pytest.mark.gpu

i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
FILL = -7
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
COS, JAC = ac.COS, ac.JAC


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _engine(kn, train, k, sim=COS, built=None, **kw):
    """a fitted engine with the lists of `built` (raw ids; None: every user) built in one neighbors_batch"""
    e = kn.Engine(k=k, similarity=ac.sim_kind(kn, sim), **kw)
    e.fit(*train)
    built = _users(train) if built is None else built
    if len(built):
        e.neighbors_batch(np.asarray(built, dtype=np.int32))
    return e


def _trace(capfd):
    """the fields of every `append` line since the last read"""
    return [{k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ln)} for ln in capfd.readouterr().err.splitlines()
            if ln.startswith("knncf-dispatch append ")]


def _raw(kn, e, rows, cap):
    """knncf_append on a FILL-filled dropped array: (status, carried, dropped count, the array)"""
    u, i, r = (np.ascontiguousarray(a, dtype=t) for a, t in zip(rows, (np.int32, np.int32, np.float64)))
    a, b = C.c_int64(FILL), C.c_int64(FILL)
    ids = np.full(max(cap, 1), FILL, dtype=np.int32)
    p = e._ptr
    rc = e._lib.knncf_append(e._h, p(u, i32p), p(i, i32p), p(r, f64p), len(u), C.byref(a), C.byref(b), p(ids, i32p) if cap else None, cap)
    return rc, a.value, b.value, ids


def _grid(case):
    """(users, items) of a prediction grid on aug: every fourth user, the changers, one unknown user x a few train items, the
    appended items, an item unknown to aug"""
    users = sorted(set(_users(case.aug)[::4]) | set(case.users.tolist()) | {bc.UNKNOWN_USER})
    items = sorted(set(np.unique(case.train[1])[::9].tolist()) | set(case.items.tolist()) | {UNKNOWN_ITEM})
    uu, ii = np.meshgrid(np.asarray(users, dtype=np.int32), np.asarray(items, dtype=np.int32), indexing="ij")
    return uu.reshape(-1), ii.reshape(-1)


def _check_answers(kn, oracle, e, case, sim, first=()):
    """neighbors_batch over every user of aug and a PRED_KNN grid against ONE oracle pipeline on aug whose lists are asked for in
    the order the handle built them: `first` (the carried ones, ascending raw id), then the others in ascending raw id"""
    m = oracle.Model(*case.aug)
    p = m.pipeline(ac.sim_kind(oracle, sim), case.k)
    users = _users(case.aug)
    rest = [v for v in users if v not in set(first)]
    want = {v: p.neighbors(v) for v in list(first) + rest}
    ids, sims, counts = e.neighbors_batch(np.asarray(rest + list(first), dtype=np.int32))
    for row, v in enumerate(rest + list(first)):
        c = counts[row]
        assert ids[row, :c].tolist() == want[v][0].tolist(), (case.name, sim, v)
        assert _bits(sims[row, :c]) == _bits(want[v][1]), (case.name, sim, v)
    uu, ii = _grid(case)
    got = e.predict_batch(kn.PRED_KNN, uu, ii)
    assert _bits(got) == _bits([p.predict(int(u), int(i)) for u, i in zip(uu, ii)]), (case.name, sim)


def _twin_table(kn, case, sim, keep, tmp_path, **kw):
    twin = _engine(kn, case.aug, case.k, sim, built=keep, **kw)
    t = _table(twin, tmp_path, "twin")
    twin.close()
    return t


def _append_and_check(kn, oracle, case, sim, tmp_path, capfd, built=None, moved=None, plain=0):
    """the whole comparison of one append on a fresh engine; returns the engine (closed) trace fields"""
    fitted = _users(case.train)
    built = fitted if built is None else built
    keep, gone = ([], [v for v in oracle.Model(*case.aug).user_iteration_order().tolist() if v in set(built)]) if plain else \
        ac.split(oracle, case, sim, built)
    e = _engine(kn, case.train, case.k, sim, built=built)
    capfd.readouterr()
    carried, n_gone, ids = kn.Appends(e).append(*case.rows, return_dropped=True)
    line = _trace(capfd)
    assert (carried, n_gone, ids.tolist()) == (len(keep), len(gone), gone), (case.name, sim)
    assert len(line) == 1 and line[0] == {"changers": len(case.changers), "built": len(built), "carried": len(keep), "dropped": len(gone),
                                          "moved": line[0]["moved"], "plain": plain}
    if moved is not None:
        assert line[0]["moved"] == moved
    assert _table(e, tmp_path, "got") == _twin_table(kn, case, sim, keep, tmp_path), (case.name, sim)
    assert e.num_users == len(_users(case.aug)) and e.num_items == len(np.unique(case.aug[1]))
    _check_answers(kn, oracle, e, case, sim, first=keep)
    e.close()
    return keep, gone


# ---- 1. adds-3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
@pytest.mark.parametrize("k", uc.ADDS_KS)
def test_adds_3(kn, synth, oracle, tmp_path, capfd, monkeypatch, k, sim):
    monkeypatch.setenv(TRACE, "1")
    keep, gone = _append_and_check(kn, oracle, ac.adds_3(synth, k), sim, tmp_path, capfd, moved=0)
    if k < 59:
        assert len(keep) > 10 and len(gone) > 5
    else:
        assert keep == []  # every list holds the changer


# ---- 2. partial B ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_partial_b(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    """every third user built: the append builds nothing, K is a subset of B, a user without a list is not dropped"""
    monkeypatch.setenv(TRACE, "1")
    case = ac.adds_3(synth, 5)
    built = _users(case.train)[::3]
    keep, gone = _append_and_check(kn, oracle, case, sim, tmp_path, capfd, built=built, moved=0)
    assert set(keep) < set(built) and set(gone) < set(built) and len(keep) + len(gone) == len(built) and keep and gone
    # nothing built before: nothing carried, nothing dropped, the state of a fit
    _append_and_check(kn, oracle, case, sim, tmp_path, capfd, built=[], moved=0)


# ---- 3. joint append -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_joint(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    """two fitted changers and a newcomer in the middle of the set order, rows interleaved: the table moves, every carried list's
    ids go through the map (the twin's lists hold the new dense ids), and the new item is predictable (it is on the grid)"""
    monkeypatch.setenv(TRACE, "1")
    case = ac.joint(synth)
    keep, gone = _append_and_check(kn, oracle, case, sim, tmp_path, capfd, moved=1)
    assert len(keep) > 5 and NEW_ITEM in _grid(case)[1].tolist()


# ---- 4. fixed-size edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_users", uc.EDGE_FITS)
def test_mask_word_edges(kn, synth, oracle, tmp_path, capfd, monkeypatch, n_users):
    """fits of 64, 65, 128 and 129 users plus one newcomer: changers (hence dropped users) at dense 63, 64 and last, the last
    user's row moves into a new 64-user word where the fit has 64 or 128"""
    monkeypatch.setenv(TRACE, "1")
    case = ac.edge_fit(synth, oracle, n_users, 7)
    keep, gone = _append_and_check(kn, oracle, case, COS, tmp_path, capfd, moved=1)
    assert set(case.note["at"]) <= set(gone) and keep


@pytest.mark.parametrize("k", (63, 64, 65))
def test_list_block_edges(kn, synth, oracle, tmp_path, capfd, monkeypatch, k):
    """full lists of 63, 64 and 65 cells with the changer stored at cells 0, 63, 64 and last (uc.edge_changer)"""
    monkeypatch.setenv(TRACE, "1")
    train = uc.scaled(synth, uc.EDGE_USERS)
    c = uc.edge_changer(oracle, train, k)
    it, rt = uc.added_rows(train, c, n=4, rating=1.0)
    case = ac._append(f"list-edge-{k}", train, (np.full(4, c), it, rt), k)
    keep, gone = _append_and_check(kn, oracle, case, COS, tmp_path, capfd, moved=0)
    assert keep and len(gone) > 4


# ---- 5. k >= U - 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_short_lists(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    monkeypatch.setenv(TRACE, "1")
    case = ac.zero_weight(synth)  # a fitted changer: the stored length stays, the planted zero-weight user is carried
    keep, gone = _append_and_check(kn, oracle, case, sim, tmp_path, capfd, moved=0)
    assert keep == [case.note["planted"]]
    for k in (60, 300):  # with a newcomer the lists grow by a cell: the plain refit
        case = ac.with_newcomer(synth, ac.base_train(synth), k)
        assert ac.is_plain(case, sim)
        _append_and_check(kn, oracle, case, sim, tmp_path, capfd, plain=1)


# ---- 6. plain refits -----------------------------------------------------------------------------------------------------------
def test_plain_refits(kn, synth, oracle, tmp_path, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    train = ac.base_train(synth)
    four = ac.with_newcomer(synth, train, 5, n=4)
    _append_and_check(kn, oracle, four, COS, tmp_path, capfd, plain=1)       # the adjusted cosine with a 4-rating user in aug
    keep, _ = _append_and_check(kn, oracle, four, JAC, tmp_path, capfd, moved=1)  # Jaccard carries
    assert keep
    # one changer too many: five-rating newcomers
    n = kn.APPEND_MAX_CHANGERS + 1
    items = np.unique(train[1])[:5]
    rows = (np.repeat(np.arange(3000, 3000 + n), 5), np.tile(items, n), np.tile([4.0, 2.5, 3.0, 5.0, 1.5], n))
    _append_and_check(kn, oracle, ac._append("crowd", train, rows, 5), COS, tmp_path, capfd, plain=1)
    # a changer whose combined mean is negative
    c = 5
    it, rt = uc.added_rows(train, c, n=2, rating=-900.0)
    _append_and_check(kn, oracle, ac._append("negative", train, (np.full(2, c), it, rt), 5), COS, tmp_path, capfd, plain=1)


# ---- 7. refusals leave the handle alone ------------------------------------------------------------------------------------------
def test_refusals(kn, synth, tmp_path, capfd):
    case = ac.adds_3(synth, 5)
    train = case.train
    e = _engine(kn, train, 5)
    uu, ii = _grid(case)

    pred0 = _bits(e.predict_batch(kn.PRED_KNN, uu, ii))

    def untouched(call, name):
        """the call's result; the checkpoint bytes around it and the predictions after it are what they were"""
        t0 = _table(e, tmp_path, name + ".0")
        out = call()
        assert _table(e, tmp_path, name + ".1") == t0, name
        assert _bits(e.predict_batch(kn.PRED_KNN, uu, ii)) == pred0, name
        return out

    mine = bc._rows(train, 5)[0]
    free = uc.added_rows(train, 5, n=2)[0]
    bad = [((np.asarray([5, 5]), np.asarray([free[0], mine[0]]), np.asarray([3.0, 3.0])), kn.E_DUPLICATE),   # against train
           ((np.asarray([5, 7, 5]), np.asarray([free[0], free[0], free[0]]), np.asarray([3.0, 2.0, 4.0])), kn.E_DUPLICATE),  # inside the rows
           ((np.asarray([1000, 1000]), np.asarray([1, 2]), np.asarray([0.0, 2.0])), kn.E_NONFINITE),         # mean 1, a rating below: scale() == 0
           ((np.asarray([5]), free[:1], np.asarray([float("nan")])), kn.E_NONFINITE)]
    for n, (rows, status) in enumerate(bad):
        rc, a, b, ids = untouched(lambda: _raw(kn, e, rows, 8), f"bad{n}")
        assert (rc, a, b) == (status, FILL, FILL) and (ids == FILL).all(), (status, rc)
    u, i, r = (np.ascontiguousarray(x, dtype=t) for x, t in zip(case.rows, (np.int32, np.int32, np.float64)))
    p = e._ptr
    a, b = C.c_int64(FILL), C.c_int64(FILL)
    args = (p(u, i32p), p(i, i32p), p(r, f64p), len(u))
    for n, call in enumerate((lambda: e._lib.knncf_append(e._h, None, *args[1:], C.byref(a), C.byref(b), None, 0),
                              lambda: e._lib.knncf_append(e._h, *args[:3], -1, C.byref(a), C.byref(b), None, 0),
                              lambda: e._lib.knncf_append(e._h, *args, None, C.byref(b), None, 0),
                              lambda: e._lib.knncf_append(e._h, *args, C.byref(a), None, None, 0),
                              lambda: e._lib.knncf_append(e._h, *args, C.byref(a), C.byref(b), None, -1),
                              lambda: e._lib.knncf_append(e._h, *args, C.byref(a), C.byref(b), None, 4))):
        assert untouched(call, f"invalid{n}") == kn.E_INVALID
        assert (a.value, b.value) == (FILL, FILL)
    # n == 0: touches nothing, reports |B|
    rc, a, b, ids = untouched(lambda: _raw(kn, e, (np.empty(0), np.empty(0), np.empty(0)), 8), "empty")
    assert (rc, a, b) == (kn.OK, 60, 0) and (ids == FILL).all()
    assert kn.Appends(e).append([], [], []) == (60, 0)
    # dropped cells past the count keep their fill; a cap below the count truncates
    rc, a, b, ids = _raw(kn, e, case.rows, 3)
    assert rc == kn.OK and b > 3 and a + b == 60 and (ids[:3] != FILL).all()
    e.close()
    e = _engine(kn, train, 5)
    rc, a, b, ids = _raw(kn, e, case.rows, 64)
    assert rc == kn.OK and (ids[:b] != FILL).all() and (ids[b:] == FILL).all()
    e.close()
    # before a fit
    e = kn.Engine(k=5)
    assert _raw(kn, e, case.rows, 0)[0] == kn.E_STATE
    e.close()
    # KNNCF_SIM_ONE has no lists: 0 / 0, and the fit is the new one
    e = kn.Engine(k=5, similarity=kn.SIM_ONE).fit(*train)
    assert kn.Appends(e).append(*ac.joint(synth).rows) == (0, 0) and e.num_users == 61
    e.close()


@pytest.mark.parametrize("route", ["no-list", "plain", "sim-one"])
def test_refusals_thrown_by_the_refit(kn, synth, oracle, tmp_path, route):
    """test_refusals runs on a handle with every list built, where the marking throws the duplicate and the non-finite deviation.
    Without a built list, on a plain refit (k >= U and a newcomer: the stored length changes) and on a KNNCF_SIM_ONE handle no
    marking runs and the fit of the second Train throws them: the handle answers as before here too, and still takes an append"""
    case = ac.adds_3(synth, 300 if route == "plain" else 5)
    train = case.train
    if route == "sim-one":
        e = kn.Engine(k=5, similarity=kn.SIM_ONE).fit(*train)
    else:
        e = _engine(kn, train, case.k, built=[] if route == "no-list" else None)
    uu, ii = _grid(case)
    pred = kn.PRED_BASELINE if route == "sim-one" else kn.PRED_KNN

    def answers():
        """what can be asked without building a list (a kNN prediction would build some and end the no-list route)"""
        out = (e.num_users, e.num_items, _bits([e.global_avg(), e.user_avg(5)]))
        return out + (_bits(e.predict_batch(kn.PRED_BASELINE, uu, ii)),) if route == "sim-one" else out

    mine = bc._rows(train, 5)[0]
    free = uc.added_rows(train, 5, n=2)[0]
    items = np.unique(train[1])[:6]
    joins = (np.full(6, 1000), items, np.asarray([4.0, 2.5, 3.0, 5.0, 1.5, 3.5]))  # a newcomer of six rows beside the bad row
    bad = [((np.concatenate([joins[0], [5]]), np.concatenate([joins[1], [mine[0]]]), np.concatenate([joins[2], [3.0]])), kn.E_DUPLICATE),
           ((np.concatenate([joins[0], [5, 5]]), np.concatenate([joins[1], [free[0], free[0]]]), np.concatenate([joins[2], [3.0, 4.0]])), kn.E_DUPLICATE),
           ((np.concatenate([joins[0], [1001, 1001]]), np.concatenate([joins[1], [1, 2]]), np.concatenate([joins[2], [0.0, 2.0]])), kn.E_NONFINITE)]
    for n, (rows, status) in enumerate(bad):
        t0 = _table(e, tmp_path, f"{n}.0") if route != "sim-one" else None
        before = answers()
        rc, a, b, ids = _raw(kn, e, rows, 8)
        assert (rc, a, b) == (status, FILL, FILL) and (ids == FILL).all(), (route, status, rc)
        assert answers() == before, (route, status)
        assert route == "sim-one" or _table(e, tmp_path, f"{n}.1") == t0, (route, status)
    if route == "sim-one":
        assert kn.Appends(e).append(*joins) == (0, 0) and e.num_users == 61
    else:
        m = oracle.Model(*train)
        p = m.pipeline(oracle.SIM_COSINE, case.k)
        assert _bits(e.predict_batch(kn.PRED_KNN, uu, ii)) == _bits([p.predict(int(u), int(i)) for u, i in zip(uu, ii)])
        kn.Appends(e).append(*case.rows)
        _check_answers(kn, oracle, e, case, COS)
    e.close()


# ---- 8. sequences ----------------------------------------------------------------------------------------------------------------
def test_two_appends_and_the_predictors(kn, synth, oracle, tmp_path):
    first = ac.adds_3(synth, 5)
    second = ac.joint(synth, train=first.aug, newcomer=1001)
    t = synth.syn_scaled(60, 80, 1500, 3).test
    e = _engine(kn, first.train, 5)
    kn.Appends(e).append(*first.rows)
    # mae(PRED_KNN) right after an append rebuilds what is missing
    m = oracle.Model(*first.aug)
    want, per = m.pipeline(oracle.SIM_COSINE, 5).mae(t.users, t.items, t.ratings, return_predictions=True)
    # (the mean itself: the device adds the errors in a fixed tree, the oracle left to right — the twin's bits, and the oracle's
    # value within the reordering bound n * 2^-53 * sum|err| / n < 300 * 1.2e-16 * 4)
    twin = kn.Engine(k=5).fit(*first.aug)
    got = e.mae(kn.PRED_KNN, t.users, t.items, t.ratings)
    assert _bits([got]) == _bits([twin.mae(kn.PRED_KNN, t.users, t.items, t.ratings)]) and abs(got - want) <= 1e-12
    twin.close()
    assert _bits(e.predict_batch(kn.PRED_KNN, t.users, t.items)) == _bits(per)
    carried, gone = kn.Appends(e).append(*second.rows)
    assert carried > 0 and carried + gone == 60
    _check_answers(kn, oracle, e, second, COS)
    # PRED_PERSONALIZED after an append: the table was rebuilt
    m2 = oracle.Model(*second.aug)
    uu, ii = _grid(second)
    p2 = m2.pipeline(oracle.SIM_COSINE, -1)
    assert _bits(e.predict_batch(kn.PRED_PERSONALIZED, uu, ii)) == _bits([p2.predict(int(u), int(i)) for u, i in zip(uu, ii)])
    kn.Appends(e).append([1001], [UNKNOWN_ITEM], [2.0])  # one more row of the newcomer, on one more new item
    assert e.num_users == 61
    # a fit of other data afterwards is unaffected
    other = uc.scaled(synth, 65)
    e.fit(*other)
    twin = kn.Engine(k=5).fit(*other)
    users = np.asarray(_users(other), dtype=np.int32)
    got, ref = e.neighbors_batch(users), twin.neighbors_batch(users)
    assert got[0].tolist() == ref[0].tolist() and _bits(got[1]) == _bits(ref[1])
    assert _table(e, tmp_path, "refit") == _table(twin, tmp_path, "refit-twin")
    e.close(); twin.close()
