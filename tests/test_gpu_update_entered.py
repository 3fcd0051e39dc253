"""Entered queries of update queries (knncf_update_entered / _batch, csrc/entered.hip): the fitted users whose kNN list holds the
changer c on train or on aug = train ++ c's additional rows, with S(v, c) on aug, c's position in both lists and the user that
left or came in, without a refit.  Every answer is compared, ids, positions and similarity bits, with the oracle: a fresh pipeline
per fitted user on train and on aug under the report rule of include/knncf.h.  The inputs are those of
tests/update_entered_cases.py (tests/test_update_entered_premises.py shows what they reach).  The `knncf-dispatch entered_update`
lines of KNNCF_DEBUG_TRACE_DISPATCH say what a chunk held and how many tail rows went through the bystander path."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import bystander_cases as bc
from tests import entered_cases as ec
from tests import update_bystander_cases as ub
from tests import update_entered_cases as uc
from tests.query_helpers import _bits, _workspace_for
from tests.test_gpu_personalized_explain import _free_device_bytes

pytestmark = pytest.mark.gpu

i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
FILL = -7
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
COS, JAC = uc.COS, uc.JAC


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _engine(kn, train, k, sim=COS, **kw):
    e = kn.Engine(k=k, similarity=ec.sim_kind(kn, sim), **kw)
    e.fit(*train)
    return e


def _raw_batch(kn, e, queries, cap, null=False):
    """knncf_update_entered_batch on FILL-filled arrays: (status of the call, (users, sims, pos, prev, other) [B, cap], counts,
    statuses)"""
    us, off, it, rt = e._query_batch(queries)
    B, p = len(us), e._ptr
    out = (np.full((B, cap), FILL, dtype=np.int32), np.full((B, cap), float(FILL)), np.full((B, cap), FILL, dtype=np.int32),
           np.full((B, cap), FILL, dtype=np.int32), np.full((B, cap), FILL, dtype=np.int32))
    counts = np.full(B, FILL, dtype=np.int32)
    st = np.full(B, FILL, dtype=np.int32)
    ptrs = [None] * 5 if null else [p(a.reshape(-1), f64p if a.dtype == np.float64 else i32p) for a in out]
    rc = e._lib.knncf_update_entered_batch(e._h, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), B, cap, *ptrs, p(counts, i32p),
                                           p(st, i32p))
    return rc, out, counts, st


def _trace(capfd):
    """((slots, fitted, pair, width) of every chunk, (queries, rows) of every tail pass) since the last read"""
    err = capfd.readouterr().err
    chunks = [tuple(int(x) for x in m.groups())
              for m in re.finditer(r"knncf-dispatch entered_update slots=(\d+) fitted=(\d+) pair=(\d+) width=(\d+)", err)]
    tails = [tuple(int(x) for x in m.groups()) for m in re.finditer(r"knncf-dispatch entered_update tails queries=(\d+) rows=(\d+)", err)]
    return chunks, tails


# ---- adds-3: every kind of reported row ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adds(synth, oracle):
    """the oracle's answers of the adds-3 cases, computed once: {(k, sim): (case, want)}"""
    return {(k, sim): (uc.adds_3(synth, k), uc.expected(oracle, uc.adds_3(synth, k), sim)) for k in uc.ADDS_KS for sim in (COS, JAC)}


@pytest.mark.parametrize("sim", [COS, JAC])
@pytest.mark.parametrize("k", uc.ADDS_KS)
def test_adds_3(kn, adds, capfd, monkeypatch, k, sim):
    monkeypatch.setenv(TRACE, "1")
    c, want = adds[k, sim]
    e = _engine(kn, c.train, k, sim)
    capfd.readouterr()
    got = kn.EnteredQueries(e).entered_with(c.q, c.items, c.ratings)
    uc.same_answer(got, want, (k, sim))
    chunks, tails = _trace(capfd)
    assert chunks == [(1, 1, 0, 0), (1, 1, 0, len(want[0]))]  # the count-only call, then the full one
    # the tail rows that travel: every row c left, and those it may have left (a superset of the premise's "stay" rows is not
    # required: a c that held the last cell with a key that did not get worse is decided from the stored list)
    left = int((want[2] == -1).sum())
    if k < 59:
        assert len(tails) == 1 and tails[0][0] == 1 and tails[0][1] >= left
    else:
        assert tails == []  # nobody is outside a list
    e.close()


@pytest.mark.parametrize("sim", [COS, JAC])
def test_zero_weight_and_no_rows(kn, synth, oracle, sim):
    c = uc.zero_weight(synth)
    want = uc.expected(oracle, c, sim)
    assert c.note["planted"] not in want[0].tolist()
    e = _engine(kn, c.train, c.k, sim)
    uc.same_answer(kn.EnteredQueries(e).entered_with(c.q, c.items, c.ratings), want, sim)
    # exception (a): a fitted c without additional rows is a valid query that reports nothing
    rc, out, counts, st = _raw_batch(kn, e, [(c.q, [], [])], 4)
    assert (rc, counts.tolist(), st.tolist()) == (kn.OK, [0], [kn.OK]) and all((a == FILL).all() for a in out)
    assert len(kn.EnteredQueries(e).entered_with(c.q, [], [])[0]) == 0
    # ... and of an absent user it stays invalid
    rc, out, counts, st = _raw_batch(kn, e, [(4321, [], [])], 4)
    assert (rc, counts.tolist(), st.tolist()) == (kn.OK, [0], [kn.E_INVALID])
    e.close()


def test_tie_at_the_cut(kn, synth, oracle):
    for c in uc.tie(synth, oracle):
        want = uc.expected(oracle, c, COS)
        e = _engine(kn, c.train, c.k)
        got = kn.EnteredQueries(e).entered_with(c.q, c.items, c.ratings)
        uc.same_answer(got, want, c.name)
        v = c.note["bystander"]
        at = got[0].tolist().index(v) if v in got[0].tolist() else -1
        if c.note["side"] == "before":
            assert got[2][at] == c.k - 1
        else:
            assert at < 0 or got[2][at] == -1
        e.close()


# ---- cap ---------------------------------------------------------------------------------------------------------------------
def test_cap(kn, adds, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    c, want = adds[20, COS]
    n = len(want[0])
    e = _engine(kn, c.train, c.k)
    q = [(c.q, c.items, c.ratings)]
    capfd.readouterr()
    rc, _, counts, st = _raw_batch(kn, e, q, 0, null=True)  # count only: no tail row is resolved
    assert (rc, counts.tolist(), st.tolist()) == (kn.OK, [n], [kn.OK])
    assert _trace(capfd)[1] == []
    cnt = C.c_int32(FILL)
    p = e._ptr
    it, rt = np.asarray(c.items, dtype=np.int32), np.asarray(c.ratings, dtype=np.float64)
    assert e._lib.knncf_update_entered(e._h, c.q, p(it, i32p), p(rt, f64p), len(it), 0, None, None, None, None, None, C.byref(cnt)) == kn.OK
    assert cnt.value == n
    # a cap between two rows that c left (tail rows): the later ones are counted and never resolved
    left = np.flatnonzero(want[2] == -1)
    assert len(left) >= 3
    cap = int(left[1]) + 1
    capfd.readouterr()
    rc, out, counts, st = _raw_batch(kn, e, q, cap)
    assert (rc, counts.tolist()) == (kn.OK, [n]) and cap < n
    uc.same_answer([a[0] for a in out], [w[:cap] for w in want], "cap between tail rows")
    tails = _trace(capfd)[1]
    assert len(tails) == 1 and 2 <= tails[0][1] < int((want[2] == -1).sum())
    rc, out, counts, st = _raw_batch(kn, e, q, n + 5)  # the cells past counts keep the marker
    uc.same_answer([a[0, :n] for a in out], want, "cap n + 5")
    assert all((a[0, n:] == FILL).all() for a in out)
    assert e._lib.knncf_update_entered_batch(e._h, None, None, None, None, 0, 5, None, None, None, None, None, None, None) == kn.OK
    assert e._lib.knncf_update_entered_batch(e._h, None, None, None, None, -1, 5, None, None, None, None, None, None, None) == kn.E_INVALID
    assert _raw_batch(kn, e, q, 3, null=True)[0] == kn.E_INVALID
    # the single form: *count = 0 once the argument checks pass, whatever the query's status
    ids, pos, prev, oth = (np.full(4, FILL, dtype=np.int32) for _ in range(4))
    sims = np.full(4, float(FILL))
    dup = np.asarray([it[0], it[0]], dtype=np.int32)
    cnt = C.c_int32(FILL)
    assert e._lib.knncf_update_entered(e._h, c.q, p(dup, i32p), p(rt, f64p), 2, 4, p(ids, i32p), p(sims, f64p), p(pos, i32p),
                                       p(prev, i32p), p(oth, i32p), C.byref(cnt)) == kn.E_DUPLICATE
    assert cnt.value == 0 and (ids == FILL).all()
    e.close()


# ---- batches -----------------------------------------------------------------------------------------------------------------
def _mixed_queries(synth, n_good=33):
    """fitted changers and newcomers on the base fit, the same changer twice with different rows, and three failed queries in
    the middle: a duplicate against a train item, a negative mean, an empty query of an absent user.  n_good answerable ones"""
    train = bc.base_train(synth)
    users = bc._users(train)
    good = []
    for j in range(n_good):
        if j % 3 == 2:  # a newcomer: the rows of a fitted user rotated, one rating changed; every other one with <= 4 rows
            it, rt = bc._rows(train, users[(7 * j) % 60])
            it, rt = np.roll(it, j), np.roll(rt, j)
            rt[0] = 1.5 if rt[0] != 1.5 else 2.5
            if j % 2 == 0:
                it, rt = it[:1 + j % 4][::-1], rt[:1 + j % 4][::-1]
            good.append((2000 + j, it.astype(np.int32), rt.copy()))
        else:
            c = users[(5 * j) % 60]
            it, rt = uc.added_rows(train, c, n=1 + j % 4, rating=[5.0, 1.0, 3.5][j % 3], skip=j % 5)
            good.append((c, it, rt))
    c = ub.CHANGER
    good[1] = (c, *uc.added_rows(train, c, n=3))
    good[4] = (c, *uc.added_rows(train, c, n=2, rating=1.0, skip=4))
    mine = bc._rows(train, c)[0]
    bad = [((c, np.asarray([mine[0]], dtype=np.int32), np.asarray([3.0])), "E_DUPLICATE"),
           ((c, uc.added_rows(train, c, n=2)[0], np.asarray([-900.0, -900.0])), "E_UNSUPPORTED"),
           ((4321, np.empty(0, dtype=np.int32), np.empty(0)), "E_INVALID")]
    queries = good[:10] + [b[0] for b in bad] + good[10:]
    statuses = ["OK"] * 10 + [b[1] for b in bad] + ["OK"] * (n_good - 10)
    return train, queries, statuses


@pytest.fixture(scope="module")
def mixed(kn, synth, oracle):
    """the mixed batch with every answerable query's single-form answer, four of them checked against the oracle"""
    train, queries, statuses = _mixed_queries(synth)
    e = _engine(kn, train, 5)
    singles = [kn.EnteredQueries(e).entered_with(*q) if s == "OK" else None for q, s in zip(queries, statuses)]
    e.close()
    for j in (1, 2, 4, 13):  # the changer named twice, a newcomer, a query behind the failed ones
        uc.same_answer(singles[j], uc.expected_for(oracle, train, *queries[j], 5, COS), j)
    assert bc._users(train).count(queries[2][0]) == 0 and len(queries[2][1]) <= 4
    return train, queries, statuses, singles


@pytest.mark.parametrize("chunk", [64, 1, 2])
def test_batch_chunks_and_statuses(kn, mixed, capfd, monkeypatch, chunk):
    """36 queries of which 33 are answerable: one chunk of 33 slots (the dual similarity kernel), and workspaces that give C = 1
    and C = 2; the rows are the single calls', failed queries leave their rows untouched"""
    monkeypatch.setenv(TRACE, "1")
    train, queries, statuses, singles = mixed
    kw = {} if chunk == 64 else {"workspace_bytes": _workspace_for(chunk, 60, 80)}
    e = _engine(kn, train, 5, **kw)
    capfd.readouterr()
    rc, out, counts, st = _raw_batch(kn, e, queries, 40)
    assert rc == kn.OK and st.tolist() == [getattr(kn, s) for s in statuses]
    chunks, _ = _trace(capfd)
    if chunk == 64:
        assert [x[0] for x in chunks] == [35] and chunks[0][2] == 1  # (the empty query is refused on the host, two on the device)
    else:
        assert max(x[0] for x in chunks) == chunk
    assert "query 10" in e._lib.knncf_last_error(e._h).decode()
    for b, s in enumerate(statuses):
        if s != "OK":
            assert counts[b] == 0 and all((a[b] == FILL).all() for a in out), b
            continue
        uc.same_answer([a[b, :counts[b]] for a in out], singles[b], (chunk, b))
        assert all((a[b, counts[b]:] == FILL).all() for a in out), b
    rows, st2 = kn.EnteredQueries(e).entered_with_batch(queries)
    assert st2.tolist() == st.tolist() and [len(r[0]) for r in rows] == counts.tolist()
    free = _free_device_bytes()
    _raw_batch(kn, e, queries, 40)  # a repeated call of the same shape allocates no device memory
    assert _free_device_bytes() >= free
    assert kn.EnteredQueries(e).entered_with_batch([])[0] == []
    e.close()


def test_jaccard_batch(kn, oracle, mixed):
    train, queries, statuses, _ = mixed
    e = _engine(kn, train, 5, JAC)
    rows, st = kn.EnteredQueries(e).entered_with_batch(queries)
    assert st.tolist() == [getattr(kn, s) for s in statuses]
    for j in (1, 2, 4, 13, 35):
        uc.same_answer(rows[j], uc.expected_for(oracle, train, *queries[j], 5, JAC), j)
    e.close()


# ---- fixed-size edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", uc.EDGE_KS)
def test_list_block_edges(kn, synth, oracle, k):
    """full lists of 63, 64, 65, 128 and 129 cells on a fit of 140 users, the changer stored at positions 0, 63, 64 and last
    (tests/test_update_entered_premises.py): the 64-cell steps of k_enu_locate and k_enu_place.  Ratings of 5.0 and of 1.0: the
    changer moves up in some lists and down, or out, in others"""
    train = uc.scaled(synth, uc.EDGE_USERS)
    c = uc.edge_changer(oracle, train, k)
    e = _engine(kn, train, k)
    for rating in (5.0, 1.0):
        items, ratings = uc.added_rows(train, c, n=4, rating=rating)
        want = uc.expected_for(oracle, train, c, items, ratings, k, COS)
        assert uc.edge_positions(k) <= set(want[3].tolist())
        uc.same_answer(kn.EnteredQueries(e).entered_with(c, items, ratings), want, (k, rating))
    e.close()


@pytest.mark.parametrize("n_users", uc.EDGE_FITS)
def test_bitmap_word_edges(kn, synth, oracle, n_users):
    """fits of 64, 65, 128 and 129 users with the changer at dense index 63, 64 and U - 1: one and two words of the report bitmap,
    the filter and the ballots at their edges; k = U - 1 reports the users at those indices, k = 7 is selective"""
    train = uc.scaled(synth, n_users)
    order = uc.dense_order(oracle, train)
    for k in (n_users - 1, 7):
        e = _engine(kn, train, k)
        queries = [(order[at], *uc.added_rows(train, order[at])) for at in uc.edge_indices(n_users)]
        rows, st = kn.EnteredQueries(e).entered_with_batch(queries)
        assert st.tolist() == [kn.OK] * len(queries)
        for q, got in zip(queries, rows):
            want = uc.expected_for(oracle, train, *q, k, COS)
            uc.same_answer(got, want, (n_users, k, q[0]))
            if k == 7:
                assert 0 < len(want[0]) < n_users - 1
        e.close()


# ---- the other calls ---------------------------------------------------------------------------------------------------------
def test_an_absent_changer_is_the_fold_in_case(kn, synth, oracle):
    """a newcomer's answer is knncf_query_entered's bit for bit, out_prev = -1: more than 4 rows, and 3-4 rows in reverse trie
    order (k_en_pair)"""
    for c in (bc.near_clone(synth), ec.tiny_newcomer(synth, oracle), bc.new_item(synth)):
        e = _engine(kn, c.train, c.k)
        q = kn.EnteredQueries(e)
        users, sims, pos, prev, other = q.entered_with(c.q, c.items, c.ratings)
        ec.same_answer((users, sims, pos, other), q.entered(c.q, c.items, c.ratings), c.name)
        assert len(users) > 0 and (prev == -1).all()
        e.close()


@pytest.mark.parametrize("sim", [COS, JAC])
def test_consistent_with_the_bystander_and_neighbour_calls(kn, adds, sim):
    """for every fitted v: c is in knncf_update_bystander_neighbors' row at out_pos and in knncf_neighbors_batch's at out_prev,
    with the same bits, and v is reported iff the rule says so"""
    c, _ = adds[20, sim]
    e = _engine(kn, c.train, c.k, sim)
    users, sims, pos, prev, other = kn.EnteredQueries(e).entered_with(c.q, c.items, c.ratings)
    fitted = [v for v in c.others if v != bc.UNKNOWN_USER]
    after = kn.BystanderQueries(e).neighbors_with(c.q, c.items, c.ratings, fitted, cap=c.k)
    before = e.neighbors_batch(np.asarray(fitted, dtype=np.int32))
    seen = 0
    for v, (ids1, s1), ids0, s0 in zip(fitted, after, before[0], before[1]):
        ids0, ids1 = ids0.tolist(), ids1.tolist()
        p0 = ids0.index(c.q) if c.q in ids0 else -1
        p1 = ids1.index(c.q) if c.q in ids1 else -1
        quiet = (p0 < 0 and p1 < 0) or (p0 >= 0 and p0 == p1 and s1[p1] == 0.0 and _bits([s0[p0]]) == _bits([s1[p1]]))
        assert (v in users.tolist()) == (not quiet), v
        if quiet:
            continue
        at = users.tolist().index(v)
        assert (pos[at], prev[at]) == (p1, p0), v
        if p1 >= 0:
            assert _bits([sims[at]]) == _bits([s1[p1]]), v
        if p0 < 0:
            assert [x for x in ids0 if x not in ids1] == [other[at]], v
        elif p1 < 0:
            assert other[at] == ids1[-1], v
        else:
            assert other[at] == -1, v
        seen += 1
    assert seen == len(users) > 20
    e.close()


# ---- handle state, refusals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", [False, True])
def test_handle_state(kn, synth, adds, tmp_path, history):
    """the call leaves the handle as knncf_neighbors_batch over the missing users in ascending raw id does — also after its tail
    rows went through the bystander path: the checkpoint bytes, the answers and a later mae are those of a twin handle"""
    c, want = adds[5, COS]
    t = synth.syn_scaled(60, 80, 1500, 3).test
    users = np.sort(np.asarray(bc._users(c.train), dtype=np.int32))
    few = np.isin(t.users, users[[2, 11, 30]])
    asked = users[[5, 44]]

    def session(tag, entered_first):
        e = _engine(kn, c.train, c.k)
        done = set()
        if history:
            e.mae(kn.PRED_KNN, t.users[few], t.items[few], t.ratings[few])
            for v in asked:
                e.neighbors(int(v))
            done = set(np.unique(t.users[few]).tolist()) | set(asked.tolist())
        got = None
        if entered_first:
            got = kn.EnteredQueries(e).entered_with(c.q, c.items, c.ratings)
        else:
            e.neighbors_batch(np.asarray([v for v in users.tolist() if v not in done], dtype=np.int32))
        e.neighbors_save(str(tmp_path / f"{tag}.1"))
        again = kn.EnteredQueries(e).entered_with(c.q, c.items, c.ratings)
        e.neighbors_save(str(tmp_path / f"{tag}.2"))
        mae = e.mae(kn.PRED_KNN, t.users, t.items, t.ratings)
        e.close()
        return got, again, mae

    got, again, mae = session("a", True)
    _, twin, twin_mae = session("b", False)
    uc.same_answer(got, want, "first call")
    uc.same_answer(again, got, "second call")
    uc.same_answer(twin, got, "twin")
    a1, a2, b1, b2 = ((tmp_path / n).read_bytes() for n in ("a.1", "a.2", "b.1", "b.2"))
    assert a1 == b1, "the state knncf_neighbors_batch over M leaves"
    assert a1 == a2 and b1 == b2, "a second call changes no byte"
    assert _bits([mae]) == _bits([twin_mae])


def test_refusals_of_the_handle(kn, synth, oracle):
    c = uc.adds_3(synth, 5)
    tiny = bc.tiny_rows(synth, oracle)[1]
    e = _engine(kn, tiny.train, tiny.k, COS)  # the adjusted cosine with train users of <= 4 ratings
    for call in (lambda: kn.EnteredQueries(e).entered_with(tiny.q, tiny.items, tiny.ratings),
                 lambda: kn.EnteredQueries(e).entered_with_batch([(tiny.q, tiny.items, tiny.ratings)]),
                 lambda: kn.EnteredQueries(e).entered_with_batch([])):
        with pytest.raises(kn.KnncfError) as err:
            call()
        assert err.value.status == kn.E_UNSUPPORTED and "<= 4 ratings" in str(err.value)
    e.close()
    e = _engine(kn, tiny.train, tiny.k, JAC)  # Jaccard is accepted: a fitted changer of one train rating
    u1 = next(u for u, n in tiny.note["tiny"].items() if n == 1)
    items, ratings = uc.added_rows(tiny.train, u1, n=2, rating=4.5)
    uc.same_answer(kn.EnteredQueries(e).entered_with(u1, items, ratings),
                   uc.expected_for(oracle, tiny.train, u1, items, ratings, tiny.k, JAC), "tiny changer")
    e.close()
    e = kn.Engine(k=5, similarity=kn.SIM_ONE)
    e.fit(*c.train)
    with pytest.raises(kn.KnncfError) as err:
        kn.EnteredQueries(e).entered_with(c.q, c.items, c.ratings)
    assert err.value.status == kn.E_UNSUPPORTED
    e.close()
    e = kn.Engine(k=5)
    with pytest.raises(kn.KnncfError) as err:
        kn.EnteredQueries(e).entered_with_batch([(c.q, c.items, c.ratings)], cap=3)
    assert err.value.status == kn.E_STATE
    e.close()
