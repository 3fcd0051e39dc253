"""knncf_amend on the GPU (csrc/append.hip, k_am_*): removed rows leave the fit, re-rated ones move behind every train row, and
the kNN lists the change cannot touch are kept.  The comparison is test_gpu_append.py's: every answer bit for bit with the oracle
on aug = train without the removed rows ++ the rows; the handle's state (the parsed knncf_neighbors_save file) with a twin engine
that ran fit(aug) and neighbors_batch over the oracle's K in ascending raw id — existing code paths only.  The inputs are those
of tests/amend_cases.py (tests/test_amend_premises.py shows what they reach and that the S-rule holds), but for the compaction
edges, whose train sets are built here so that the file rows are under the test's control.  KNNCF_DEBUG_TRACE_DISPATCH: the
`append` line says what a call carried, the `amend` line what the removal stage took out."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import amend_cases as am
from tests import append_cases as ac
from tests import bystander_cases as bc
from tests import rating_scales as rs
from tests import update_entered_cases as uc
from tests.bystander_cases import NEW_ITEM, _rows, _users
from tests.query_helpers import UNKNOWN_ITEM, _bits
from tests.revise_bystander_cases import LONE_ITEM
from tests.test_gpu_similarity_batch import _table

pytestmark = pytest.mark.gpu

i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
FILL = -7
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
MAX_CHANGERS = "KNNCF_DEBUG_APPEND_MAX_CHANGERS"
COS, JAC = am.COS, am.JAC


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _engine(kn, train, k, sim=COS, built=None, **kw):
    """a fitted engine with the lists of `built` (raw ids; None: every user) built in one neighbors_batch"""
    e = kn.Engine(k=k, similarity=am.sim_kind(kn, sim), **kw)
    e.fit(*train)
    built = _users(train) if built is None else built
    if len(built):
        e.neighbors_batch(np.asarray(built, dtype=np.int32))
    return e


def _trace(capfd):
    """the fields of every `append` and every `amend` line since the last read"""
    out = {"append": [], "amend": []}
    for ln in capfd.readouterr().err.splitlines():
        m = re.match(r"knncf-dispatch (append|amend) ", ln)
        if m:
            out[m.group(1)].append({k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", ln)})
    return out


def _raw(kn, e, removals, rows, cap):
    """knncf_amend on a FILL-filled dropped array: (status, carried, dropped count, the array)"""
    ru, ri = (np.ascontiguousarray(a, dtype=np.int32) for a in removals)
    u, i, r = (np.ascontiguousarray(a, dtype=t) for a, t in zip(rows, (np.int32, np.int32, np.float64)))
    a, b = C.c_int64(FILL), C.c_int64(FILL)
    ids = np.full(max(cap, 1), FILL, dtype=np.int32)
    p = e._ptr
    rc = e._lib.knncf_amend(e._h, p(ru, i32p), p(ri, i32p), len(ru), p(u, i32p), p(i, i32p), p(r, f64p), len(u), C.byref(a), C.byref(b),
                            p(ids, i32p) if cap else None, cap)
    return rc, a.value, b.value, ids


def _grid(case):
    """(users, items) of a prediction grid on aug: every fourth user, the changers (a user that left among them), one unknown
    user x a few train items, the removed items (the item that left among them), the lone item where train has it, the rows'
    items, an item unknown to aug"""
    users = sorted(set(_users(case.aug)[::4]) | {c for c, _, _, _ in case.changers} | {bc.UNKNOWN_USER})
    mine = np.unique(case.train[1])
    items = sorted(set(mine[::9].tolist()) | ({LONE_ITEM} & set(mine.tolist())) | set(case.removed_items.tolist()) | set(case.items.tolist()) | {UNKNOWN_ITEM})
    uu, ii = np.meshgrid(np.asarray(users, dtype=np.int32), np.asarray(items, dtype=np.int32), indexing="ij")
    return uu.reshape(-1), ii.reshape(-1)


def _check_answers(kn, oracle, e, case, sim, first=()):
    """neighbors_batch over every user of aug and a PRED_KNN grid against ONE oracle pipeline on aug whose lists are asked for in
    the order the handle built them: `first` (the carried ones, ascending raw id), then the others in ascending raw id"""
    m = oracle.Model(*case.aug)
    p = m.pipeline(am.sim_kind(oracle, sim), case.k)
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
    return m


def _twin_table(kn, case, sim, keep, tmp_path, **kw):
    twin = _engine(kn, case.aug, case.k, sim, built=keep, **kw)
    t = _table(twin, tmp_path, "twin")
    twin.close()
    return t


def _expected_split(oracle, case, sim, built, plain):
    """(K, B ∩ S in the new fit's set order — a user that left where its id would stand)"""
    if not plain:
        return am.split(oracle, case, sim, built)
    assert len(_users(case.aug)) >= 5
    return [], bc.trie_sorted(oracle, built)


def _amend_and_check(kn, oracle, case, sim, tmp_path, capfd, built=None, moved=None, plain=0):
    """the whole comparison of one amend on a fresh engine; returns (K, B ∩ S)"""
    fitted = _users(case.train)
    built = fitted if built is None else built
    keep, gone = _expected_split(oracle, case, sim, built, plain)
    e = _engine(kn, case.train, case.k, sim, built=built)
    capfd.readouterr()
    carried, n_gone, ids = am.amend(e, *case.call, return_dropped=True)
    lines = _trace(capfd)
    assert (carried, n_gone, ids.tolist()) == (len(keep), len(gone), gone), (case.name, sim)
    assert len(lines["append"]) == 1 and lines["append"][0] == {"changers": len(case.changers), "built": len(built), "carried": len(keep),
                                                                "dropped": len(gone), "moved": lines["append"][0]["moved"], "plain": plain}
    if moved is not None:
        assert lines["append"][0]["moved"] == moved
    n_removed = len(case.removed_users)
    assert lines["amend"] == ([{"removers": len(case.removers), "removed": n_removed, "kept_rows": len(case.train[0]) - n_removed}] if n_removed else [])
    assert _table(e, tmp_path, "got") == _twin_table(kn, case, sim, keep, tmp_path), (case.name, sim)
    assert e.num_users == len(_users(case.aug)) and e.num_items == len(np.unique(case.aug[1]))
    _check_answers(kn, oracle, e, case, sim, first=keep)
    e.close()
    return keep, gone


# ---- 1. a single changer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
@pytest.mark.parametrize("k", (5, 20, 59))
@pytest.mark.parametrize("build", [am.removes_3, am.re_rates, am.same_value])
def test_single_changer(kn, synth, oracle, tmp_path, capfd, monkeypatch, build, k, sim):
    """removes-3, re-rates with another value, re-rates with the same value (an ordinary change: the lists of S are dropped)"""
    monkeypatch.setenv(TRACE, "1")
    keep, gone = _amend_and_check(kn, oracle, build(synth, k), sim, tmp_path, capfd, moved=0)
    assert len(gone) > 5 and (len(keep) > 10 if k < 59 else keep == [])  # (k = 59: every list holds the changer)


@pytest.mark.parametrize("sim", [COS, JAC])
def test_zero_weight_removal(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    """k >= U - 1: the planted user shares no item with the changer and keeps it at the same place with +0.0 — carried"""
    monkeypatch.setenv(TRACE, "1")
    case = am.zero_weight(synth)
    keep, gone = _amend_and_check(kn, oracle, case, sim, tmp_path, capfd, moved=0)
    assert keep == [case.note["planted"]]


# ---- 2. the lone item ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_lone_item(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    """removed / re-rated / kept: num_items drops by one only in the first, where the item predicts as an unknown one"""
    monkeypatch.setenv(TRACE, "1")
    n_items = len(np.unique(am.lone_item(synth, 5)[0].train[1]))
    for case, want in zip(am.lone_item(synth, 5), (n_items - 1, n_items, n_items)):
        assert LONE_ITEM in _grid(case)[1].tolist() and len(np.unique(case.aug[1])) == want
        keep, _ = _amend_and_check(kn, oracle, case, sim, tmp_path, capfd, moved=0)
        assert keep


# ---- 3. the joint call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_joint(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    """a fitted changer that removes and re-rates, one that only removes, one that only adds and a newcomer; the rows interleave,
    the removals are shuffled, the table moves"""
    monkeypatch.setenv(TRACE, "1")
    case = am.joint(synth)
    keep, gone = _amend_and_check(kn, oracle, case, sim, tmp_path, capfd, moved=1)
    assert len(keep) > 5 and NEW_ITEM in _grid(case)[1].tolist() and set(case.note["fitted"]) <= set(gone)


# ---- 4. partial B ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_partial_b(kn, synth, oracle, tmp_path, capfd, monkeypatch, sim):
    """every third user built: the amend builds nothing, K is a subset of B; and B empty: the state of a fit"""
    monkeypatch.setenv(TRACE, "1")
    case = am.re_rates(synth, 5)
    built = _users(case.train)[::3]
    keep, gone = _amend_and_check(kn, oracle, case, sim, tmp_path, capfd, built=built, moved=0)
    assert set(keep) < set(built) and set(gone) < set(built) and len(keep) + len(gone) == len(built) and keep and gone
    _amend_and_check(kn, oracle, case, sim, tmp_path, capfd, built=[], moved=0)


# ---- 5. mask-word edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_users", uc.EDGE_FITS)
def test_mask_word_edges(kn, synth, oracle, tmp_path, capfd, monkeypatch, n_users):
    """fits of 64, 65, 128 and 129 users: removers (hence dropped users) at dense 63, 64 and last; the newcomer moves the last
    user's row into a new 64-user word where the fit has 64 or 128"""
    monkeypatch.setenv(TRACE, "1")
    case = am.edge_fit(synth, oracle, n_users, 7)
    keep, gone = _amend_and_check(kn, oracle, case, COS, tmp_path, capfd, moved=1)
    assert set(case.note["at"]) <= set(gone) and keep


# ---- 6. plain refits -----------------------------------------------------------------------------------------------------------
def test_plain_refits(kn, synth, oracle, tmp_path, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    four = am.keeps_4(synth, 5)
    assert am.is_plain(four, COS) and not am.is_plain(four, JAC)
    _amend_and_check(kn, oracle, four, COS, tmp_path, capfd, plain=1)              # the adjusted cosine with a changer brought down to 4 rows
    keep, _ = _amend_and_check(kn, oracle, four, JAC, tmp_path, capfd, moved=0)   # Jaccard carries
    assert keep
    gone = am.leaver(synth, 5)                                                    # a user leaves: num_users one less
    for sim in (COS, JAC):
        _amend_and_check(kn, oracle, gone, sim, tmp_path, capfd, plain=1)
    assert len(_users(gone.aug)) == 59
    joins = am.with_newcomer(synth, am.base_train(synth), 60)                     # a newcomer at k >= U - 1: the lists grow by a cell
    assert am.is_plain(joins, JAC)
    _amend_and_check(kn, oracle, joins, JAC, tmp_path, capfd, plain=1)
    crowd = am.crowd(synth, kn.APPEND_MAX_CHANGERS + 1)                            # one remover too many
    _amend_and_check(kn, oracle, crowd, COS, tmp_path, capfd, plain=1)


def test_a_fit_that_shrinks_below_five_users(kn, oracle, tmp_path, capfd, monkeypatch):
    """five users, one leaves: the four that stay iterate in the order of their first row (a Set4), not by hash — dropped lists
    them in that order and the user that left behind them"""
    monkeypatch.setenv(TRACE, "1")
    users = [40, 12, 77, 3, 58]
    rows = [(u, 10 * i + 1, float(1 + (3 * x + 2 * i) % 9) / 2) for i in range(6) for x, u in enumerate(users) if (x + i) % 5]
    train = tuple(np.asarray(a, dtype=t) for a, t in zip(zip(*rows), (np.int32, np.int32, np.float64)))
    who = 77
    mine = _rows(train, who)[0]
    case = am._amend("shrinks-to-4", train, (np.full(len(mine), who), mine), ([], [], []), 2)
    order = oracle.Model(*case.aug).user_iteration_order().tolist()
    assert sorted(order) == [3, 12, 40, 58] and bc.trie_sorted(oracle, order) != order and len(np.unique(train[1])) >= 5
    for sim in (COS, JAC):
        e = _engine(kn, train, 2, sim)
        capfd.readouterr()
        carried, n_gone, ids = am.amend(e, *case.call, return_dropped=True)
        line = _trace(capfd)["append"]
        assert (carried, n_gone, ids.tolist()) == (0, 5, order + [who]) and len(line) == 1 and line[0]["plain"] == 1
        assert _table(e, tmp_path, "got") == _twin_table(kn, case, sim, [], tmp_path)
        assert e.num_users == 4
        _check_answers(kn, oracle, e, case, sim)
        e.close()


# ---- 7. compaction edges -------------------------------------------------------------------------------------------------------
EDGE_USERS, EDGE_ITEMS = 70, 60   # 4 200 pairs: enough for 2 T + 1 = 4 097 file rows
RUN_USER = 3 * 7 + 3              # the user whose consecutive rows lie across the T - 1 | T boundary


def _file(n, T, domain, seed=5):
    """a train set of n file rows over 70 users x 60 items in a shuffled order, every user with more than 8 rows; where the file has
    them, rows T - 3 .. T + 2 are six consecutive rows of RUN_USER.  domain: "sixteenths" (dyadic) or "tenths" (non-dyadic: every
    sum shows its order in its bits)"""
    rng = np.random.default_rng(seed)
    pairs = [(u * 7 + 3, i * 13 + 1) for u in range(1, EDGE_USERS + 1) for i in range(1, EDGE_ITEMS + 1)]
    order = rng.permutation(len(pairs))
    # the first 9 rows of every user first, so that a short file still holds every user with more than 8 rows
    head = [p for u in range(EDGE_USERS) for p in order[order // EDGE_ITEMS == u][:9]]
    taken = set(head)
    rows = [pairs[p] for p in (head + [p for p in order if p not in taken])[:n]]
    rows = [rows[p] for p in rng.permutation(n)]
    if n >= T + 3:
        for to in range(T - 3, T + 3):  # one more row of RUN_USER from outside the rows placed so far
            y = next(x for x, (u, _) in enumerate(rows) if u == RUN_USER and not T - 3 <= x < to)
            rows[y], rows[to] = rows[to], rows[y]
        assert all(rows[x][0] == RUN_USER for x in range(T - 3, T + 3))
    u, i = (np.asarray(a, dtype=np.int32) for a in zip(*rows))
    assert len(set(rows)) == n and np.unique(u, return_counts=True)[1].min() > 8
    return u, i, rs.rating_values(rng, domain, n).astype(np.float64)


def _removing(name, train, at, k=5):
    at = sorted(set(int(x) for x in at))
    return am._amend(name, train, (train[0][at], train[1][at]), ([], [], []), k, file_rows=at)


def _compaction_leg(kn, oracle, case, tmp_path, capfd, plain, values=False):
    keep, gone = _amend_and_check(kn, oracle, case, COS, tmp_path, capfd, moved=0, plain=plain)
    if values:  # the order of the surviving rows shows in the bits of every sum over them
        e = _engine(kn, case.train, case.k, COS, built=[])
        am.amend(e, *case.call)
        m = oracle.Model(*case.aug)
        uu, ii = _grid(case)
        assert _bits([e.global_avg()]) == _bits([m.average()]), case.name
        assert _bits(e.predict_batch(kn.PRED_BASELINE, uu, ii)) == _bits([m.predict(oracle.KIND_BASELINE, int(u), int(i)) for u, i in zip(uu, ii)])
        e.close()
    return keep, gone


def _edge_rows(n, T):
    at = [x for x in (0, 63, 64, T - 1, T, n - 1) if x < n]
    return at + (list(range(T - 3, T + 3)) if n >= T + 3 else [])


@pytest.mark.parametrize("which", ["T-1", "T", "T+1", "2T", "2T+1"])
def test_compaction_edges(kn, oracle, tmp_path, capfd, monkeypatch, which):
    """file rows 0, 63, 64, T - 1, T and n - 1 removed, and a run of one user's consecutive rows across the T - 1 | T boundary, at
    n = T - 1, T, T + 1, 2 T and 2 T + 1 rows: the first, the last and the only row of a tile, both sides of a bitmap word"""
    monkeypatch.setenv(TRACE, "1")
    T = kn.AMEND_TILE
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "2T": 2 * T, "2T+1": 2 * T + 1}[which]
    train = _file(n, T, "sixteenths")
    assert rs.is_dyadic(train[2])
    case = _removing(f"edges-{which}", train, _edge_rows(n, T))
    assert not am.is_plain(case, COS)
    keep, gone = _compaction_leg(kn, oracle, case, tmp_path, capfd, plain=0)
    assert keep and set(case.removers) <= set(gone)


def test_compaction_is_stable(kn, oracle, tmp_path, capfd, monkeypatch):
    """the same removals on non-dyadic ratings at n = 2 T + 1: global_avg, PRED_BASELINE and PRED_KNN equal the oracle's on aug in
    their bits, which a compaction that reorders rows would not give"""
    monkeypatch.setenv(TRACE, "1")
    T = kn.AMEND_TILE
    train = _file(2 * T + 1, T, "tenths")
    assert not rs.is_dyadic(train[2])
    _compaction_leg(kn, oracle, _removing("edges-non-dyadic", train, _edge_rows(2 * T + 1, T)), tmp_path, capfd, plain=0, values=True)


@pytest.mark.parametrize("which", ["first-of-two", "middle-of-three"])
def test_compaction_whole_tiles(kn, oracle, tmp_path, capfd, monkeypatch, which):
    """a tile that loses every row beside tiles that lose none (n = 2 T: tile 0 goes; n = 2 T + 1: tile 1 goes, tiles 0 and 2 stay
    whole).  Every user is a remover here; the changer limit is set to 0 so that the oracle need not mark for 70 changers: the
    removal stage runs in front of a plain refit all the same"""
    monkeypatch.setenv(TRACE, "1")
    monkeypatch.setenv(MAX_CHANGERS, "0")
    T = kn.AMEND_TILE
    n, at = (2 * T, range(0, T)) if which == "first-of-two" else (2 * T + 1, range(T, 2 * T))
    train = _file(n, T, "tenths")
    case = _removing(f"tile-{which}", train, at)
    assert len(case.removers) == EDGE_USERS
    _compaction_leg(kn, oracle, case, tmp_path, capfd, plain=1, values=True)


# ---- 8. no removals: knncf_append ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_without_removals_it_is_append(kn, synth, tmp_path, capfd, monkeypatch, sim):
    monkeypatch.setenv(TRACE, "1")
    case = ac.joint(synth)
    a, b = _engine(kn, case.train, case.k, sim), _engine(kn, case.train, case.k, sim)
    capfd.readouterr()
    got = am.amend(a, [], [], *case.rows, return_dropped=True)
    la = _trace(capfd)
    want = kn.Appends(b).append(*case.rows, return_dropped=True)
    lb = _trace(capfd)
    assert got[:2] == want[:2] and got[2].tolist() == want[2].tolist() and got[0] > 0 and got[1] > 0
    assert la == lb and len(la["append"]) == 1 and la["amend"] == []
    assert _table(a, tmp_path, "amend") == _table(b, tmp_path, "append")
    # both sizes 0: |B| and 0, nothing touched
    t0 = _table(a, tmp_path, "before")
    rc, x, y, ids = _raw(kn, a, ([], []), ([], [], []), 8)
    assert (rc, x, y) == (kn.OK, got[0], 0) and (ids == FILL).all() and _table(a, tmp_path, "after") == t0
    assert am.amend(a, [], [], [], [], []) == (got[0], 0) and _trace(capfd) == {"append": [], "amend": []}
    a.close(); b.close()


# ---- 9. refusals leave the handle alone ------------------------------------------------------------------------------------------
def test_refusals(kn, synth, tmp_path, capfd):
    case = am.re_rates(synth, 5)
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

    mine = _rows(train, 5)[0]
    free = uc.added_rows(train, 5, n=2)[0]
    none = ([], [], [])
    joins = (np.full(6, 1000), np.unique(train[1])[:6], np.asarray([4.0, 2.5, 3.0, 5.0, 1.5, 3.5]))
    bad = [(([5], [free[0]]), none, kn.E_INVALID),                                             # not a train row of the user
           (([5], [UNKNOWN_ITEM]), none, kn.E_INVALID),                                        # an item unknown to train
           (([bc.UNKNOWN_USER], [mine[0]]), none, kn.E_INVALID),                               # a user unknown to train
           (([1000], [joins[1][0]]), joins, kn.E_INVALID),                                     # a newcomer of the same call
           (([5, 7, 5], [mine[0], _rows(train, 7)[0][0], mine[0]]), none, kn.E_INVALID),       # listed twice
           (([5], [mine[0]]), ([5], [mine[1]], [3.0]), kn.E_DUPLICATE),                        # a row on an unremoved train item
           (([5], [mine[0]]), ([5, 5], [mine[0], mine[0]], [3.0, 4.0]), kn.E_DUPLICATE),       # the re-rating given twice
           (([5], [mine[0]]), ([5], [mine[0]], [float("nan")]), kn.E_NONFINITE),
           (([5], [mine[0]]), ([1000, 1000], [1, 2], [0.0, 2.0]), kn.E_NONFINITE),             # mean 1, a rating below: scale() == 0
           ((train[0], train[1]), none, kn.E_INVALID),                                         # everything removed: aug without a row
           (([5], [free[0]]), ([5], [mine[1]], [3.0]), kn.E_INVALID),                          # precedence: the bad removal before the duplicate
           (([5, 5], [mine[0], mine[0]]), ([5], [mine[1]], [float("nan")]), kn.E_INVALID)]
    for n, (removals, rows, status) in enumerate(bad):
        rc, a, b, ids = untouched(lambda: _raw(kn, e, removals, rows, 8), f"bad{n}")
        assert (rc, a, b) == (status, FILL, FILL) and (ids == FILL).all(), (n, status, rc)
    # argument checks
    ru, ri = np.asarray([5], dtype=np.int32), np.asarray([mine[0]], dtype=np.int32)
    u, i, r = np.asarray([5], dtype=np.int32), np.asarray([free[0]], dtype=np.int32), np.asarray([3.0])
    p = e._ptr
    a, b = C.c_int64(FILL), C.c_int64(FILL)
    rm, rows = (p(ru, i32p), p(ri, i32p), 1), (p(u, i32p), p(i, i32p), p(r, f64p), 1)
    out = (C.byref(a), C.byref(b), None, 0)
    for n, call in enumerate((lambda: e._lib.knncf_amend(e._h, None, rm[1], 1, *rows, *out),
                              lambda: e._lib.knncf_amend(e._h, rm[0], None, 1, *rows, *out),
                              lambda: e._lib.knncf_amend(e._h, rm[0], rm[1], -1, *rows, *out),
                              lambda: e._lib.knncf_amend(e._h, *rm, None, *rows[1:], *out),
                              lambda: e._lib.knncf_amend(e._h, *rm, *rows[:3], -1, *out),
                              lambda: e._lib.knncf_amend(e._h, *rm, *rows, None, C.byref(b), None, 0),
                              lambda: e._lib.knncf_amend(e._h, *rm, *rows, C.byref(a), None, None, 0),
                              lambda: e._lib.knncf_amend(e._h, *rm, *rows, C.byref(a), C.byref(b), None, -1),
                              lambda: e._lib.knncf_amend(e._h, *rm, *rows, C.byref(a), C.byref(b), None, 4))):
        assert untouched(call, f"invalid{n}") == kn.E_INVALID, n
        assert (a.value, b.value) == (FILL, FILL)
    # the handle still takes the call; cells past the count keep their fill
    rc, a, b, ids = _raw(kn, e, case.removals, case.rows, 64)
    assert rc == kn.OK and a + b == 60 and (ids[:b] != FILL).all() and (ids[b:] == FILL).all()
    e.close()
    # without a built list no marking runs: the removal stage refuses all the same, and the refit throws the duplicate
    e = _engine(kn, train, 5, built=[])
    before = (e.num_users, e.num_items, _bits([e.global_avg(), e.user_avg(5)]))
    for removals, rows, status in (bad[0], bad[3], bad[4], bad[5], bad[8], bad[10]):
        assert _raw(kn, e, removals, rows, 0)[0] == status
        assert (e.num_users, e.num_items, _bits([e.global_avg(), e.user_avg(5)])) == before
    e.close()
    # before a fit
    e = kn.Engine(k=5)
    assert _raw(kn, e, case.removals, case.rows, 0)[0] == kn.E_STATE
    e.close()
    # KNNCF_SIM_ONE has no lists: 0 / 0, and the fit is the new one
    e = kn.Engine(k=5, similarity=kn.SIM_ONE).fit(*train)
    gone = am.leaver(synth, 5)
    assert am.amend(e, *gone.call) == (0, 0) and e.num_users == 59
    e.close()


# ---- 10. a sequence on one handle ------------------------------------------------------------------------------------------------
def test_a_sequence_on_one_handle(kn, synth, tmp_path):
    """append -> amend (re-rate) -> mae -> amend (only removes) -> recommend_batch -> amend back to the original multiset of rows,
    whose file order differs; after every step the handle answers as a fresh fit of the data so far"""
    first = ac.adds_3(synth, 5)
    t = synth.syn_scaled(60, 80, 1500, 3).test
    e = _engine(kn, first.train, 5)
    data = first.train

    def same_as_a_fresh_fit(step):
        twin = kn.Engine(k=5).fit(*data)
        users = np.asarray(_users(data), dtype=np.int32)
        assert (e.num_users, e.num_items) == (twin.num_users, twin.num_items), step
        assert _bits([e.global_avg()]) == _bits([twin.global_avg()]), step
        assert _bits([e.mae(kn.PRED_KNN, t.users, t.items, t.ratings)]) == _bits([twin.mae(kn.PRED_KNN, t.users, t.items, t.ratings)]), step
        got, ref = e.neighbors_batch(users), twin.neighbors_batch(users)
        assert got[0].tolist() == ref[0].tolist() and _bits(got[1]) == _bits(ref[1]), step
        got, ref = e.recommend_batch(kn.PRED_KNN, users[::5], 7), twin.recommend_batch(kn.PRED_KNN, users[::5], 7)
        assert got[0].tolist() == ref[0].tolist() and _bits(got[1]) == _bits(ref[1]) and got[2].tolist() == ref[2].tolist(), step
        assert _bits(e.predict_batch(kn.PRED_PERSONALIZED, t.users[:50], t.items[:50])) == _bits(twin.predict_batch(kn.PRED_PERSONALIZED, t.users[:50], t.items[:50])), step
        twin.close()

    def amend(removals, rows):
        nonlocal data
        case = am._amend("step", data, removals, rows, 5)
        out = am.amend(e, *case.call)
        data = case.aug
        return out

    kn.Appends(e).append(*first.rows)
    data = first.aug
    same_as_a_fresh_fit("append")
    c = int(first.users[0])
    added = first.items.tolist()
    carried, gone = amend(([c], [added[0]]), ([c], [added[0]], [1.5]))            # re-rate one of the appended rows
    assert carried > 0 and carried + gone == 60
    same_as_a_fresh_fit("re-rate")
    carried, gone = amend(([c, c], [added[1], added[2]]), ([], [], []))           # only removes
    assert carried > 0
    same_as_a_fresh_fit("removes")
    # back to the original multiset of rows: the re-rated row goes too, and a train row of another user moves to the end
    other = 23
    it, rt = _rows(first.train, other)
    amend(([c, other], [added[0], int(it[0])]), ([other], [int(it[0])], [float(rt[0])]))
    original = sorted(zip(*(a.tolist() for a in first.train)))
    assert sorted(zip(*(a.tolist() for a in data))) == original and data[0].tolist() != first.train[0].tolist()
    same_as_a_fresh_fit("back")
    e.close()
