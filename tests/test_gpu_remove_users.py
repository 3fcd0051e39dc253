"""knncf_remove_users on the GPU (csrc/append.hip: k_am_flag_users, k_ap_holders, k_ap_remap's "gone"): users leave the fit and
the kNN lists that hold none of them are kept.  The comparison is test_gpu_amend.py's: every answer bit for bit with the oracle
on aug = train without the leavers' rows; the handle's state (the parsed knncf_neighbors_save file) with a twin engine that ran
fit(aug) and neighbors_batch over the oracle's K in ascending raw id — existing code paths only.  The inputs are those of
tests/remove_users_cases.py (tests/test_remove_users_premises.py shows what they reach and that the S-rule holds), but for the
tile edge, whose train set is built here so that the file rows are under the test's control.  KNNCF_DEBUG_TRACE_DISPATCH: the
`append` line says what a call carried, the `remove` line what the removal stage took out and how many lists held a leaver."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import amend_cases as am
from tests import append_cases as ac
from tests import bystander_cases as bc
from tests import remove_users_cases as ru
from tests import update_entered_cases as uc
from tests.bystander_cases import _rows, _users
from tests.query_helpers import UNKNOWN_ITEM, _bits
from tests.test_gpu_amend import FILL, MAX_CHANGERS, TRACE, _check_answers, _engine, _grid, _twin_table
from tests.test_gpu_similarity_batch import _table

pytestmark = pytest.mark.gpu

i32p = C.POINTER(C.c_int32)
NO_LDS = "KNNCF_DEBUG_NO_LDS_BITMAPS"
COS, JAC = ru.COS, ru.JAC


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _trace(capfd):
    """the fields of every `append`, `amend` and `remove` line since the last read (bitmap: "lds" or "global")"""
    out = {"append": [], "amend": [], "remove": []}
    for ln in capfd.readouterr().err.splitlines():
        m = re.match(r"knncf-dispatch (append|amend|remove) ", ln)
        if m:
            out[m.group(1)].append({k: int(v) if v.isdigit() else v for k, v in re.findall(r"(\w+)=(\w+)", ln)})
    return out


def _raw(e, users, cap, n=None):
    """knncf_remove_users on a FILL-filled dropped array: (status, carried, dropped count, the array)"""
    u = np.ascontiguousarray(users, dtype=np.int32)
    a, b = C.c_int64(FILL), C.c_int64(FILL)
    ids = np.full(max(cap, 1), FILL, dtype=np.int32)
    p = e._ptr
    rc = e._lib.knncf_remove_users(e._h, p(u, i32p), len(u) if n is None else n, C.byref(a), C.byref(b), p(ids, i32p) if cap else None, cap)
    return rc, a.value, b.value, ids


def _remove_on(kn, oracle, e, case, sim, built, tmp_path, capfd, plain=None, bitmap="lds", max_leavers=ru.MAX_LEAVERS):
    """knncf_remove_users of the case's leavers on engine e, whose built lists are `built`, and the whole comparison; (K, B ∩ S)"""
    plain = ru.is_plain(case, sim, max_leavers) if plain is None else plain
    keep, gone = ru.split(oracle, case, sim, built, plain=plain)
    leavers = case.note["leavers"]
    capfd.readouterr()
    carried, n_gone, ids = ru.remove_users(e, leavers, return_dropped=True)
    lines = _trace(capfd)
    assert (carried, n_gone, ids.tolist()) == (len(keep), len(gone), gone), (case.name, sim)
    assert lines["append"] == [{"changers": len(leavers), "built": len(built), "carried": len(keep), "dropped": len(gone),
                                "moved": 0 if plain else 1, "plain": int(plain)}], (case.name, lines)
    n_removed = len(case.removed_users)
    assert lines["remove"] == [{"users": len(leavers), "removed": n_removed, "kept_rows": len(case.train[0]) - n_removed,
                                "holders": len(set(gone) - set(leavers)), "bitmap": bitmap}] and lines["amend"] == [], (case.name, lines)
    assert _table(e, tmp_path, "got") == _twin_table(kn, case, sim, keep, tmp_path), (case.name, sim)
    assert e.num_users == len(_users(case.aug)) and e.num_items == len(np.unique(case.aug[1]))
    _check_answers(kn, oracle, e, case, sim, first=keep)
    return keep, gone


def _remove_and_check(kn, oracle, case, sim, tmp_path, capfd, built=None, **kw):
    """the whole comparison of one call on a fresh engine; returns (K, B ∩ S)"""
    built = _users(case.train) if built is None else built
    e = _engine(kn, case.train, case.k, sim, built=built)
    out = _remove_on(kn, oracle, e, case, sim, built, tmp_path, capfd, **kw)
    e.close()
    return out


# ---- 1. one leaver, two leavers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
@pytest.mark.parametrize("k", (5, 20, 57))
def test_one_leaver(kn, synth, oracle, tmp_path, capfd, monkeypatch, k, sim):
    monkeypatch.setenv(TRACE, "1")
    case = ru.one(synth, 23, k)
    grid = _grid(case)
    assert 23 in grid[0].tolist() and bc.UNKNOWN_USER in grid[0].tolist() and UNKNOWN_ITEM in grid[1].tolist()
    keep, gone = _remove_and_check(kn, oracle, case, sim, tmp_path, capfd)
    assert 23 in gone and len(gone) > 1 and (len(keep) > 10 or k == 57)


@pytest.mark.parametrize("sim", [COS, JAC])
@pytest.mark.parametrize("k", (5, 20))
def test_first_and_last_cell(kn, synth, oracle, tmp_path, capfd, monkeypatch, k, sim):
    """a leaver that stands in cell 0 of one stored list and in cell kcap - 1 of another"""
    monkeypatch.setenv(TRACE, "1")
    keep, gone = _remove_and_check(kn, oracle, ru.one(synth, ru.CELL_LEAVER, k), sim, tmp_path, capfd)
    assert keep and len(gone) > 2


@pytest.mark.parametrize("sim", [COS, JAC])
@pytest.mark.parametrize("k", (5, 57))
def test_two_leavers_in_one_call(kn, synth, oracle, tmp_path, capfd, monkeypatch, k, sim):
    """given in descending order; at k = 57 every list holds one of them: 0 carried, and still no plain refit"""
    monkeypatch.setenv(TRACE, "1")
    keep, gone = _remove_and_check(kn, oracle, ru.two(synth, k), sim, tmp_path, capfd, plain=False)
    assert {23, 41} <= set(gone) and ((len(keep) > 10) if k == 5 else keep == [])


# ---- 2. against knncf_amend given every row of the leaver ----------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_amend_answers_the_same_and_carries_nothing(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    """the assertion that separates the call from a refit behind a new name: carried > 0 here, 0 through knncf_amend"""
    monkeypatch.setenv(TRACE, "1")
    case = ru.two(synth, 5)
    keep, _ = ru.split(oracle, case, sim, _users(case.train))
    assert len(keep) > 10
    a, b = _engine(kn, case.train, case.k, sim), _engine(kn, case.train, case.k, sim)
    carried, gone = ru.remove_users(a, case.note["leavers"])
    assert (carried, gone) == (len(keep), 60 - len(keep)) and carried > 0
    assert am.amend(b, *case.call) == (0, 60)
    assert (a.num_users, a.num_items) == (b.num_users, b.num_items) == (58, len(np.unique(case.aug[1])))
    users = np.asarray(_users(case.aug), dtype=np.int32)
    uu, ii = _grid(case)
    got, ref = a.neighbors_batch(users), b.neighbors_batch(users)
    assert got[0].tolist() == ref[0].tolist() and _bits(got[1]) == _bits(ref[1]) and got[2].tolist() == ref[2].tolist()
    assert _bits(a.predict_batch(kn.PRED_KNN, uu, ii)) == _bits(b.predict_batch(kn.PRED_KNN, uu, ii))
    assert _bits(a.predict_batch(kn.PRED_BASELINE, uu, ii)) == _bits(b.predict_batch(kn.PRED_BASELINE, uu, ii))
    assert _bits([a.global_avg()]) == _bits([b.global_avg()])
    a.close(); b.close()


# ---- 3. word and tile edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_users", ru.EDGE_NS)
def test_mask_word_edges(kn, synth, oracle, tmp_path, capfd, monkeypatch, n_users):
    """fits of 63, 64, 65 and 129 users: leavers at dense 0, 63, 64 and last (63 and 64 adjacent), every user behind one moves up"""
    monkeypatch.setenv(TRACE, "1")
    case = ru.edge(synth, oracle, n_users)
    keep, gone = _remove_and_check(kn, oracle, case, COS, tmp_path, capfd)
    assert set(case.note["leavers"]) <= set(gone) and keep


def test_adjacent_pair(kn, synth, oracle, tmp_path, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    case = ru.adjacent(synth, oracle)
    keep, gone = _remove_and_check(kn, oracle, case, JAC, tmp_path, capfd)
    assert set(case.note["leavers"]) <= set(gone) and keep


TILE_LEAVER = 5000


def _straddling_file(kn, synth):
    """uc.scaled(129) (more than T + 10 file rows) with 74 rows of a new user at file rows [T - 64, T + 10): they fill bitmap word T / 64 - 1
    completely and go on across the boundary between tile 0 and tile 1"""
    T = kn.AMEND_TILE
    u, i, r = uc.scaled(synth, 129)
    items = np.unique(i)[:74].astype(np.int32)
    vals = (1.0 + (np.arange(74) * 7 % 9) / 2).astype(np.float64)
    at = T - 64
    assert len(items) == 74 and len(u) > T + 10 and at % 64 == 0
    train = (np.concatenate([u[:at], np.full(74, TILE_LEAVER, dtype=np.int32), u[at:]]).astype(np.int32),
             np.concatenate([i[:at], items, i[at:]]).astype(np.int32), np.concatenate([r[:at], vals, r[at:]]))
    rows = np.flatnonzero(train[0] == TILE_LEAVER)
    assert rows.tolist() == list(range(T - 64, T + 10))
    return train


@pytest.mark.parametrize("who", ["the-run", "the-run-and-two"])
def test_rows_across_a_tile_boundary(kn, synth, oracle, tmp_path, capfd, monkeypatch, who):
    """the leaver's rows are one run that fills a 64-row bitmap word and crosses KNNCF_AMEND_TILE; with two more leavers whose rows
    lie scattered on both sides of it"""
    monkeypatch.setenv(TRACE, "1")
    train = _straddling_file(kn, synth)
    order = uc.dense_order(oracle, train)
    leavers = [TILE_LEAVER] + ([order[1], order[-2]] if who == "the-run-and-two" else [])
    case = ru.leaving(f"tile-{who}", train, leavers, 5)
    keep, gone = _remove_and_check(kn, oracle, case, COS, tmp_path, capfd)
    assert keep and TILE_LEAVER in gone
    # the order of the surviving rows shows in the bits of every sum over them
    e = _engine(kn, case.train, case.k, COS, built=[])
    assert ru.remove_users(e, leavers) == (0, 0)
    m = oracle.Model(*case.aug)
    uu, ii = _grid(case)
    assert _bits([e.global_avg()]) == _bits([m.average()])
    assert _bits(e.predict_batch(kn.PRED_BASELINE, uu, ii)) == _bits([m.predict(oracle.KIND_BASELINE, int(u), int(i)) for u, i in zip(uu, ii)])
    e.close()


# ---- 4. long lists -------------------------------------------------------------------------------------------------------------------
def test_long_lists(kn, synth, oracle, tmp_path, capfd, monkeypatch):
    """140 users at k = 100: a wave takes two steps over a stored list, and some holders have the leaver only in the second"""
    monkeypatch.setenv(TRACE, "1")
    case = ru.long_lists(synth, oracle)
    keep, gone = _remove_and_check(kn, oracle, case, COS, tmp_path, capfd)
    held = ru.holders(oracle, case, COS)
    late = [v for v, at in held.items() if at[0] >= 64]
    assert late and set(late) <= set(gone) and keep


# ---- 5. partial B --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_partial_b(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    """every other list built: a leaver without a list is not in dropped, a holder without a list is in neither count; then with the
    leaver's list built; and B empty: the state of a fit"""
    monkeypatch.setenv(TRACE, "1")
    case = ru.two(synth, 20)
    fitted = _users(case.train)
    for built in (fitted[::2], fitted[1::2]):
        held = set(ru.holders(oracle, case, sim))
        keep, gone = _remove_and_check(kn, oracle, case, sim, tmp_path, capfd, built=built)
        assert set(keep) < set(built) and set(gone) < set(built) and len(keep) + len(gone) == len(built) and keep and gone
        assert held - set(built) and not (held - set(built)) & (set(keep) | set(gone))
        assert {c for c in (23, 41) if c in built} == {23, 41} & set(gone)
    assert (23 in fitted[::2]) != (23 in fitted[1::2])
    _remove_and_check(kn, oracle, case, sim, tmp_path, capfd, built=[])


# ---- 6. the lone item ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_lone_item(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    """the leaver is the only rater of an item: num_items drops by one, and the item predicts as an unknown one (it is in the grid)"""
    monkeypatch.setenv(TRACE, "1")
    case = ru.lone_rater(synth)
    assert ru.LONE_ITEM in _grid(case)[1].tolist() and len(np.unique(case.aug[1])) == len(np.unique(case.train[1])) - 1
    keep, _ = _remove_and_check(kn, oracle, case, sim, tmp_path, capfd)
    assert keep


# ---- 7. a life on one handle ---------------------------------------------------------------------------------------------------------
def test_a_life_on_one_handle(kn, synth, oracle, tmp_path, capfd, monkeypatch):
    """append -> remove_users -> amend -> neighbors_save / neighbors_load -> remove_users on the shrunk handle; after every step the
    lists the handle holds are the oracle's K of that step, and the state and the answers those of a fresh fit with K built"""
    monkeypatch.setenv(TRACE, "1")
    first = ac.joint(synth)
    e = _engine(kn, first.train, 5)
    built = _users(first.train)

    def check(case, keep):
        assert _table(e, tmp_path, "life") == _twin_table(kn, case, COS, keep, tmp_path), case.name
        assert e.num_users == len(_users(case.aug)) and e.num_items == len(np.unique(case.aug[1]))
        _check_answers(kn, oracle, e, case, COS, first=keep)
        return _users(case.aug)  # (_check_answers asked for every list)

    # append: two fitted changers and a newcomer
    step = am._amend("life-append", first.train, ([], []), first.rows, 5)
    keep, gone = ac.split(oracle, first, COS, built)
    assert kn.Appends(e).append(*first.rows) == (len(keep), len(gone)) and keep
    built = check(step, keep)
    # the newcomer and a fitted user leave again
    case = ru.leaving("life-remove", step.aug, [first.note["newcomer"], 41], 5)
    keep, gone = _remove_on(kn, oracle, e, case, COS, built, tmp_path, capfd)
    assert keep and len(gone) > 2
    built = _users(case.aug)
    # amend: user 5 removes two rows and rates one of them again
    mine = _rows(case.aug, 5)[0]
    step = am._amend("life-amend", case.aug, ([5, 5], [int(mine[0]), int(mine[2])]), ([5], [int(mine[0])], [1.5]), 5)
    keep, gone = am.split(oracle, step, COS, built)
    assert am.amend(e, *step.call) == (len(keep), len(gone)) and keep
    built = check(step, keep)
    # the checkpoint goes through a fresh handle's load and comes back
    path = str(tmp_path / "life.ckpt")
    e.neighbors_save(path)
    e.close()
    e = kn.Engine(k=5).fit(*step.aug)
    e.neighbors_load(path)
    # and two more users leave the shrunk fit
    case = ru.leaving("life-remove-2", step.aug, [23, 7], 5)
    keep, gone = _remove_on(kn, oracle, e, case, COS, built, tmp_path, capfd)
    assert keep and {23, 7} <= set(gone) and e.num_users == 57
    e.close()


# ---- 8. the leaver bitmap in global memory -------------------------------------------------------------------------------------------
def test_bitmap_in_global_memory(kn, synth, oracle, tmp_path, capfd, monkeypatch):
    """the 129-user edge case again with KNNCF_DEBUG_NO_LDS_BITMAPS: the trace says bitmap=global (test_mask_word_edges: bitmap=lds)"""
    monkeypatch.setenv(TRACE, "1")
    monkeypatch.setenv(NO_LDS, "1")
    case = ru.edge(synth, oracle, 129)
    keep, gone = _remove_and_check(kn, oracle, case, COS, tmp_path, capfd, bitmap="global")
    assert keep and set(case.note["leavers"]) <= set(gone)
    monkeypatch.delenv(NO_LDS)
    _remove_and_check(kn, oracle, ru.long_lists(synth, oracle), COS, tmp_path, capfd, bitmap="lds")


# ---- 9. plain refits -----------------------------------------------------------------------------------------------------------------
def test_plain_refits(kn, synth, oracle, tmp_path, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    full = ru.one(synth, 23, 59)                                                    # k = U - 1: the lists lose a cell
    assert ru.is_plain(full, JAC)
    _remove_and_check(kn, oracle, full, JAC, tmp_path, capfd, plain=True)
    short = ru.short_row_fit(synth)                                                 # a user of 4 ratings in train
    assert ru.is_plain(short, COS) and not ru.is_plain(short, JAC)
    _remove_and_check(kn, oracle, short, COS, tmp_path, capfd, plain=True)
    keep, _ = _remove_and_check(kn, oracle, short, JAC, tmp_path, capfd, plain=False)  # Jaccard carries
    assert keep
    crowd = ru.crowd(synth)                                                         # one leaver too many
    assert len(crowd.note["leavers"]) == kn.APPEND_MAX_CHANGERS + 1 == ru.MAX_LEAVERS + 1
    _remove_and_check(kn, oracle, crowd, JAC, tmp_path, capfd, plain=True)
    monkeypatch.setenv(MAX_CHANGERS, "0")                                           # the hook: every call is a plain refit
    _remove_and_check(kn, oracle, ru.one(synth, 23, 5), COS, tmp_path, capfd, plain=True)
    monkeypatch.delenv(MAX_CHANGERS)
    # KNNCF_SIM_ONE has no lists: 0 / 0, and the fit is the new one
    case = ru.one(synth, 23, 5)
    e = kn.Engine(k=5, similarity=kn.SIM_ONE).fit(*case.train)
    capfd.readouterr()
    assert ru.remove_users(e, [23], return_dropped=True)[:2] == (0, 0) and e.num_users == 59
    line = _trace(capfd)
    assert line["append"][0]["plain"] == 1 and line["remove"][0]["holders"] == 0
    e.close()


def test_a_fit_that_shrinks_below_five_users(kn, oracle, tmp_path, capfd, monkeypatch):
    """five users, one leaves: the four that stay iterate in the order of their first row — dropped lists them in that order and the
    leaver behind them, as knncf_amend does"""
    monkeypatch.setenv(TRACE, "1")
    case = ru.to_four_users()
    order = oracle.Model(*case.aug).user_iteration_order().tolist()
    assert sorted(order) == [3, 12, 40, 58] and bc.trie_sorted(oracle, order) != order
    for sim in (COS, JAC):
        keep, gone = _remove_and_check(kn, oracle, case, sim, tmp_path, capfd, plain=True)
        assert keep == [] and gone == order + [77]


# ---- 10. refusals leave the handle alone -----------------------------------------------------------------------------------------------
def test_refusals(kn, synth, tmp_path):
    case = ru.one(synth, 23, 5)
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
        assert (e.num_users, e.num_items) == (60, len(np.unique(train[1]))), name
        return out

    everyone = _users(train)
    bad = [[bc.UNKNOWN_USER],                      # no user of train
           [23, bc.UNKNOWN_USER],
           [23, 41, 23],                           # listed twice
           everyone,                               # no row is left
           [bc.UNKNOWN_USER] + everyone,           # precedence: the ids before the empty aug
           everyone + [23]]
    for n, users in enumerate(bad):
        rc, a, b, ids = untouched(lambda: _raw(e, users, 8), f"bad{n}")
        assert (rc, a, b) == (kn.E_INVALID, FILL, FILL) and (ids == FILL).all(), (n, rc)
    # argument checks
    u = np.asarray([23], dtype=np.int32)
    p = e._ptr
    a, b = C.c_int64(FILL), C.c_int64(FILL)
    for n, call in enumerate((lambda: e._lib.knncf_remove_users(e._h, None, 1, C.byref(a), C.byref(b), None, 0),
                              lambda: e._lib.knncf_remove_users(e._h, p(u, i32p), -1, C.byref(a), C.byref(b), None, 0),
                              lambda: e._lib.knncf_remove_users(e._h, p(u, i32p), 1, None, C.byref(b), None, 0),
                              lambda: e._lib.knncf_remove_users(e._h, p(u, i32p), 1, C.byref(a), None, None, 0),
                              lambda: e._lib.knncf_remove_users(e._h, p(u, i32p), 1, C.byref(a), C.byref(b), None, -1),
                              lambda: e._lib.knncf_remove_users(e._h, p(u, i32p), 1, C.byref(a), C.byref(b), None, 4),
                              # precedence: the arguments before the ids
                              lambda: e._lib.knncf_remove_users(e._h, p(np.asarray([bc.UNKNOWN_USER], dtype=np.int32), i32p), 1, None, C.byref(b), None, 0))):
        assert untouched(call, f"invalid{n}") == kn.E_INVALID, n
        assert (a.value, b.value) == (FILL, FILL)
    # the handle still takes the call; cells past the count keep their fill
    rc, a, b, ids = _raw(e, [23], 64)
    assert rc == kn.OK and a + b == 60 and a > 0 and (ids[:b] != FILL).all() and (ids[b:] == FILL).all() and e.num_users == 59
    e.close()
    # without a built list no marking runs: the ids are checked all the same
    e = _engine(kn, train, 5, built=[])
    for users in bad:
        assert _raw(e, users, 0)[0] == kn.E_INVALID and e.num_users == 60
    e.close()
    # before a fit
    e = kn.Engine(k=5)
    assert _raw(e, [23], 0)[0] == kn.E_STATE
    e.close()
    # a shard handle
    e = kn.Engine(k=5, shard_rank=0, shard_count=2)
    e.fit(*train)
    assert _raw(e, [23], 0)[0] == kn.E_UNSUPPORTED
    e.close()


# ---- 11. no leaver ---------------------------------------------------------------------------------------------------------------------
def test_no_leaver_touches_nothing(kn, synth, tmp_path, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    train = ru.base_train(synth)
    built = _users(train)[::3]
    e = _engine(kn, train, 5, built=built)
    t0 = _table(e, tmp_path, "before")
    capfd.readouterr()
    rc, a, b, ids = _raw(e, [], 8)
    assert (rc, a, b) == (kn.OK, len(built), 0) and (ids == FILL).all()
    assert e._lib.knncf_remove_users(e._h, None, 0, C.byref(C.c_int64()), C.byref(C.c_int64()), None, 0) == kn.OK
    assert ru.remove_users(e, []) == (len(built), 0) and ru.remove_users(e, [], return_dropped=True)[2].tolist() == []
    assert _trace(capfd) == {"append": [], "amend": [], "remove": []}
    assert _table(e, tmp_path, "after") == t0 and e.num_users == 60
    e.close()
