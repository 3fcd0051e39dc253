"""Entered queries of revise queries (knncf_revise_entered / _batch, csrc/entered.hip): the fitted users whose kNN list holds the
changer c on train or on aug = train without c's removed rows ++ c's additional rows, with S(v, c) on aug, c's position in both
lists and the user that left or came in, without a refit.  Every answer is compared, ids, positions and similarity bits, with the
oracle: a fresh pipeline per fitted user on train and on aug under the report rule of include/knncf.h.  The inputs are those of
tests/revise_entered_cases.py (tests/test_revise_entered_premises.py shows what they reach).  The `knncf-dispatch entered_update`
and `entered_revise` lines of KNNCF_DEBUG_TRACE_DISPATCH say what a chunk held and how many tail rows went through the bystander
path."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import bystander_cases as bc
from tests import entered_cases as ec
from tests import revise_entered_cases as rc
from tests import update_entered_cases as uc
from tests.query_helpers import _bits, _workspace_for
from tests.test_gpu_personalized_explain import _free_device_bytes

pytestmark = pytest.mark.gpu

i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
FILL = -7
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
COS, JAC = rc.COS, rc.JAC
CHANGER = rc.CHANGER
NONE = np.empty(0, dtype=np.int32)
MAKERS = {"removes-3": rc.removes_3, "keeps-4": rc.keeps_4, "re-rates": rc.re_rates}


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _engine(kn, train, k, sim=COS, **kw):
    e = kn.Engine(k=k, similarity=ec.sim_kind(kn, sim), **kw)
    e.fit(*train)
    return e


def _outputs(B, cap):
    return (np.full((B, cap), FILL, dtype=np.int32), np.full((B, cap), float(FILL)), np.full((B, cap), FILL, dtype=np.int32),
            np.full((B, cap), FILL, dtype=np.int32), np.full((B, cap), FILL, dtype=np.int32))


def _raw_batch(kn, e, queries, cap, null=False):
    """knncf_revise_entered_batch over (user, removed, items, ratings) queries on FILL-filled arrays: (status of the call,
    (users, sims, pos, prev, other) [B, cap], counts, statuses)"""
    qargs, keep = e._batch_args("revise", queries)
    B, p = qargs[-1], e._ptr
    out = _outputs(B, cap)
    counts = np.full(B, FILL, dtype=np.int32)
    st = np.full(B, FILL, dtype=np.int32)
    ptrs = [None] * 5 if null else [p(a.reshape(-1), f64p if a.dtype == np.float64 else i32p) for a in out]
    rc_ = e._lib.knncf_revise_entered_batch(e._h, *qargs, cap, *ptrs, p(counts, i32p), p(st, i32p))
    return rc_, out, counts, st


def _trace(capfd):
    """((slots, fitted, pair, width) of every chunk, (slots, removed, small) of every chunk with removals, (queries, rows) of every
    tail pass) since the last read"""
    err = capfd.readouterr().err
    ints = lambda pattern: [tuple(int(x) for x in m.groups()) for m in re.finditer(pattern, err)]
    return (ints(r"knncf-dispatch entered_update slots=(\d+) fitted=(\d+) pair=(\d+) width=(\d+)"),
            ints(r"knncf-dispatch entered_revise slots=(\d+) removed=(\d+) small=(\d+)"),
            ints(r"knncf-dispatch entered_update tails queries=(\d+) rows=(\d+)"))


def _ask(kn, e, case, cap=None):
    return kn.EnteredQueries(e).entered_with(case.q, case.items, case.ratings, cap=cap, removed=case.removed)


# ---- the removal cases: every kind of reported row ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def answers(synth, oracle):
    """the oracle's answers of the removal cases, computed once: {(name, k, sim): (case, want)}"""
    out = {}
    for name, make in MAKERS.items():
        for k in rc.KS:
            for sim in (COS, JAC):
                case = make(synth, k)
                out[name, k, sim] = (case, rc.expected(oracle, case, sim))
    return out


@pytest.mark.parametrize("sim", [COS, JAC])
@pytest.mark.parametrize("k", rc.KS)
@pytest.mark.parametrize("name", sorted(MAKERS))
def test_removal_cases(kn, answers, capfd, monkeypatch, name, k, sim):
    monkeypatch.setenv(TRACE, "1")
    c, want = answers[name, k, sim]
    assert len(want[0]) > 0  # (a removal-only query is answered like any other: exception (a) needs n_removed == 0 as well)
    e = _engine(kn, c.train, k, sim)
    capfd.readouterr()
    uc.same_answer(_ask(kn, e, c), want, (name, k, sim))
    chunks, revised, tails = _trace(capfd)
    small = int(name == "keeps-4")
    pair = int(small and sim == COS)
    assert chunks == [(1, 1, pair, 0), (1, 1, pair, len(want[0]))]  # the count-only call, then the full one
    assert revised == [(1, len(c.removed), small)] * 2
    left = int((want[2] == -1).sum())
    if k < 59 and left > 0:
        assert len(tails) == 1 and tails[0][0] == 1 and tails[0][1] >= left
    elif k < 59:  # (nobody left: a c that keeps the last cell with a key that did not get worse is decided from the stored list)
        assert len(tails) <= 1
    else:
        assert tails == []  # nobody is outside a list
    e.close()


@pytest.mark.parametrize("k,changer", [(5, rc.KEEPS_4_K5_CHANGER), (20, CHANGER), (59, CHANGER), (300, CHANGER)])
def test_keeps_4_similarities_are_the_bystanders(kn, synth, oracle, capfd, monkeypatch, k, changer):
    """a cosine changer that falls to 4 rows on aug: pair=1 small=1, and the reported rows whose bits depend on who owns the pair
    carry S(v, c) as v folds it, not the S(c, v) that the changer's own revise query answers"""
    monkeypatch.setenv(TRACE, "1")
    c = rc.keeps_4(synth, k, changer)
    want = rc.expected(oracle, c, COS)
    rows = rc.pair_order_rows(oracle, c)
    assert rows
    e = _engine(kn, c.train, k)
    capfd.readouterr()
    got = _ask(kn, e, c, cap=60)
    uc.same_answer(got, want, (k, changer))
    chunks, revised, _ = _trace(capfd)
    assert chunks == [(1, 1, 1, 60)] and revised == [(1, len(c.removed), 1)]
    own_ids, own_sims = e.neighbors_revised(c.q, c.removed, c.items, c.ratings, cap=60)  # c owns these pairs
    for v, s in rows:
        at = got[0].tolist().index(v)
        assert _bits([got[1][at]]) == _bits([s])
        if v in own_ids.tolist():
            assert _bits([own_sims[own_ids.tolist().index(v)]]) != _bits([s]), v
    e.close()


@pytest.mark.parametrize("sim", [COS, JAC])
def test_lone_item_same_value_and_zero_weight(kn, synth, oracle, sim):
    for c in rc.lone_item(synth, 5) + [rc.same_value(synth, 5), rc.same_value(synth, 20)]:
        want = rc.expected(oracle, c, sim)
        assert len(want[0]) > 0
        eng = _engine(kn, c.train, c.k, sim)
        uc.same_answer(_ask(kn, eng, c), want, (c.name, sim))
        eng.close()
    z = rc.zero_weight(synth)
    want = rc.expected(oracle, z, sim)
    assert z.note["planted"] not in want[0].tolist()
    eng = _engine(kn, z.train, z.k, sim)
    uc.same_answer(_ask(kn, eng, z), want, ("zero-weight", sim))
    # exception (a): a fitted c without removals and without rows is a valid query that reports nothing
    rc_, out, counts, st = _raw_batch(kn, eng, [(z.q, [], [], [])], 4)
    assert (rc_, counts.tolist(), st.tolist()) == (kn.OK, [0], [kn.OK]) and all((a == FILL).all() for a in out)
    assert len(kn.EnteredQueries(eng).entered_with(z.q, [], [], removed=[])[0]) == 0
    # ... of an absent user it stays invalid, with or without a removal
    rc_, out, counts, st = _raw_batch(kn, eng, [(4321, [], [], []), (4321, [int(z.removed[0])], [], [])], 4)
    assert (rc_, counts.tolist(), st.tolist()) == (kn.OK, [0, 0], [kn.E_INVALID, kn.E_INVALID])
    eng.close()


def test_without_removals_it_is_the_update_call(kn, synth, capfd, monkeypatch):
    """n_removed == 0 in every query: knncf_update_entered_batch's arrays byte for byte on FILL-filled buffers, the same trace
    lines, no entered_revise line"""
    monkeypatch.setenv(TRACE, "1")
    train = bc.base_train(synth)
    users = bc._users(train)
    queries = [(users[3 * j], *uc.added_rows(train, users[3 * j], n=1 + j % 3, rating=[5.0, 1.0][j % 2])) for j in range(2, 8)]
    queries += [(CHANGER, *uc.added_rows(train, CHANGER, n=3)), (2000, *bc._rows(train, users[7])), (2001, bc._rows(train, users[9])[0][:3][::-1], np.asarray([1.0, 5.0, 2.5])),
                (users[4], NONE, np.empty(0))]
    e = _engine(kn, train, 5)
    us, off, it, rt = e._query_batch(queries)
    B, p, cap = len(us), e._ptr, 30
    want = _outputs(B, cap)
    w_counts, w_st = np.full(B, FILL, dtype=np.int32), np.full(B, FILL, dtype=np.int32)
    capfd.readouterr()
    assert e._lib.knncf_update_entered_batch(e._h, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), B, cap,
                                             *[p(a.reshape(-1), f64p if a.dtype == np.float64 else i32p) for a in want],
                                             p(w_counts, i32p), p(w_st, i32p)) == kn.OK
    w_chunks, w_revised, w_tails = _trace(capfd)
    rc_, got, counts, st = _raw_batch(kn, e, [(q[0], NONE, q[1], q[2]) for q in queries], cap)
    chunks, revised, tails = _trace(capfd)
    assert rc_ == kn.OK and counts.tolist() == w_counts.tolist() and st.tolist() == w_st.tolist() == [kn.OK] * B
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert (chunks, tails) == (w_chunks, w_tails) and revised == w_revised == [] and counts[-1] == 0 and counts[:8].min() > 0
    assert w_chunks[0][2] == 1 and len(w_tails) == 1  # (the batch has a newcomer of 3 rows and tail rows)
    e.close()


# ---- cap ---------------------------------------------------------------------------------------------------------------------
def test_cap(kn, answers, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    c, want = answers["removes-3", 20, COS]
    n = len(want[0])
    e = _engine(kn, c.train, c.k)
    q = [c.query]
    capfd.readouterr()
    rc_, _, counts, st = _raw_batch(kn, e, q, 0, null=True)  # count only: no tail row is resolved
    assert (rc_, counts.tolist(), st.tolist()) == (kn.OK, [n], [kn.OK])
    assert _trace(capfd)[2] == []
    cnt = C.c_int32(FILL)
    p = e._ptr
    rm = np.asarray(c.removed, dtype=np.int32)
    assert e._lib.knncf_revise_entered(e._h, c.q, p(rm, i32p), len(rm), None, None, 0, 0, None, None, None, None, None, C.byref(cnt)) == kn.OK
    assert cnt.value == n
    # a cap between two rows that c left (tail rows): the later ones are counted and never resolved
    left = np.flatnonzero(want[2] == -1)
    assert len(left) >= 3
    cap = int(left[1]) + 1
    capfd.readouterr()
    rc_, out, counts, st = _raw_batch(kn, e, q, cap)
    assert (rc_, counts.tolist()) == (kn.OK, [n]) and cap < n
    uc.same_answer([a[0] for a in out], [w[:cap] for w in want], "cap between tail rows")
    tails = _trace(capfd)[2]
    assert len(tails) == 1 and 2 <= tails[0][1] < int((want[2] == -1).sum())
    rc_, out, counts, st = _raw_batch(kn, e, q, n + 5)  # the cells past counts keep the marker
    uc.same_answer([a[0, :n] for a in out], want, "cap n + 5")
    assert all((a[0, n:] == FILL).all() for a in out)
    nulls = [None] * 7
    assert e._lib.knncf_revise_entered_batch(e._h, None, None, None, None, None, None, 0, 5, *nulls) == kn.OK
    assert e._lib.knncf_revise_entered_batch(e._h, None, None, None, None, None, None, -1, 5, *nulls) == kn.E_INVALID
    assert _raw_batch(kn, e, q, 3, null=True)[0] == kn.E_INVALID
    # the call-level refusals of the removed CSR
    us, off = np.asarray([c.q], dtype=np.int32), np.zeros(2, dtype=np.int64)
    out = _outputs(1, 4)
    ptrs = [p(a.reshape(-1), f64p if a.dtype == np.float64 else i32p) for a in out]
    counts, st = np.full(1, FILL, dtype=np.int32), np.full(1, FILL, dtype=np.int32)
    for roff, items in (([0, 3], None), ([1, 3], rm), ([0, -1], rm), (None, rm)):
        ro = None if roff is None else p(np.asarray(roff, dtype=np.int64), i64p)
        ri = None if items is None else p(items, i32p)
        assert e._lib.knncf_revise_entered_batch(e._h, p(us, i32p), ro, ri, p(off, i64p), None, None, 1, 4, *ptrs, p(counts, i32p),
                                                 p(st, i32p)) == kn.E_INVALID, roff
    assert all((a == FILL).all() for a in out)
    # the single form: *count = 0 once the argument checks pass, whatever the query's status
    ids, pos, prev, oth = (np.full(4, FILL, dtype=np.int32) for _ in range(4))
    sims = np.full(4, float(FILL))
    outs = (p(ids, i32p), p(sims, f64p), p(pos, i32p), p(prev, i32p), p(oth, i32p))
    twice = np.asarray([rm[0], rm[0]], dtype=np.int32)
    cnt = C.c_int32(FILL)
    assert e._lib.knncf_revise_entered(e._h, c.q, p(twice, i32p), 2, None, None, 0, 4, *outs, C.byref(cnt)) == kn.E_INVALID
    assert cnt.value == 0 and (ids == FILL).all()
    cnt = C.c_int32(FILL)  # ... and stays as it was when they do not
    assert e._lib.knncf_revise_entered(e._h, c.q, None, -1, None, None, 0, 4, *outs, C.byref(cnt)) == kn.E_INVALID
    assert e._lib.knncf_revise_entered(e._h, c.q, None, 2, None, None, 0, 4, *outs, C.byref(cnt)) == kn.E_INVALID
    assert cnt.value == FILL
    e.close()


# ---- batches -----------------------------------------------------------------------------------------------------------------
def rb_other(r):
    """another value on the same scale (revise_bystander_cases._other_value)"""
    return rc.rb._other_value(r, True)


def _mixed_queries(synth, n_good=33):
    """revise changers, plain update changers and newcomers on the base fit, the same changer twice with different removals, and
    in the middle one failed query of each kind.  n_good answerable ones"""
    train = bc.base_train(synth)
    users = bc._users(train)
    good = []
    for j in range(n_good):
        if j % 4 == 2:  # a newcomer: the rows of a fitted user rotated, one rating changed; every other one with <= 4 rows
            it, rt = bc._rows(train, users[(7 * j) % 60])
            it, rt = np.roll(it, j), np.roll(rt, j)
            rt[0] = 1.5 if rt[0] != 1.5 else 2.5
            if j % 8 == 2:
                it, rt = it[:1 + j % 4][::-1], rt[:1 + j % 4][::-1]
            good.append((2000 + j, NONE, it.astype(np.int32), rt.copy()))
        elif j % 4 == 3:  # a plain update changer
            c = users[(5 * j) % 60]
            good.append((c, NONE, *uc.added_rows(train, c, n=1 + j % 3, rating=[5.0, 1.0, 3.5][j % 3], skip=j % 5)))
        else:  # a revise changer: 1-3 removals, every other one with additional rows as well
            c = users[(5 * j) % 60]
            rm = rc.removed_rows(train, c, 1 + j % 3, skip=j % 4)
            it, rt = uc.added_rows(train, c, n=(j % 2) * (1 + j % 3), rating=[4.5, 1.0][j % 2 == 0], skip=j % 5)
            good.append((c, rm, it, rt))
    mine, vals = bc._rows(train, CHANGER)
    good[1] = (CHANGER, mine[[0, 8, 16]], NONE, np.empty(0))
    good[4] = (CHANGER, mine[[3, 4]], mine[[4]], np.asarray([rb_other(vals[4])]))  # one removal and one re-rating
    good[8] = (CHANGER, mine[4:], NONE, np.empty(0))  # keeps-4 in the middle of a chunk
    free = uc.added_rows(train, CHANGER, n=2)[0]
    bad = [((CHANGER, free[:1], NONE, np.empty(0)), "E_INVALID"),                                   # an unrated removed item
           ((CHANGER, mine[[2, 2]], NONE, np.empty(0)), "E_INVALID"),                               # a removed item twice
           ((4321, mine[:1], mine[:2], np.asarray([3.0, 4.0])), "E_INVALID"),                       # a removal for an absent user
           ((CHANGER, mine, NONE, np.empty(0)), "E_INVALID"),                                       # left without a row
           ((CHANGER, mine[:1], mine[1:2], np.asarray([3.0])), "E_DUPLICATE"),                      # against an unremoved train item
           ((CHANGER, mine[:2], free, np.asarray([-900.0, -900.0])), "E_UNSUPPORTED")]              # a negative mean on aug
    queries = good[:10] + [b[0] for b in bad] + good[10:]
    statuses = ["OK"] * 10 + [b[1] for b in bad] + ["OK"] * (n_good - 10)
    return train, queries, statuses


def _single(kn, e, q, cap=None):
    return kn.EnteredQueries(e).entered_with(q[0], q[2], q[3], cap=cap, removed=q[1])


@pytest.fixture(scope="module")
def mixed(kn, synth, oracle):
    """the mixed batch with every answerable query's single-form answer, some of them checked against the oracle"""
    train, queries, statuses = _mixed_queries(synth)
    e = _engine(kn, train, 5)
    singles = [_single(kn, e, q) if s == "OK" else None for q, s in zip(queries, statuses)]
    e.close()
    for j in (0, 1, 2, 3, 4, 8, 17):  # revise changers, the changer named three times, a newcomer, an update changer, one behind the failed ones
        uc.same_answer(singles[j], rc.expected_for(oracle, train, *queries[j], 5, COS), j)
    assert bc._users(train).count(queries[2][0]) == 0 and len(queries[2][2]) <= 4
    kinds = [("new" if q[0] >= 2000 else "revise" if len(q[1]) else "update") for q, s in zip(queries, statuses) if s == "OK"]
    assert min(kinds.count(x) for x in ("new", "revise", "update")) >= 8
    return train, queries, statuses, singles


@pytest.mark.parametrize("chunk", [64, 1, 2])
def test_batch_chunks_and_statuses(kn, mixed, capfd, monkeypatch, chunk):
    """39 queries of which 33 are answerable: one chunk (the dual similarity kernel), and workspaces that give C = 1 and C = 2;
    the rows are the single calls', failed queries leave their rows untouched"""
    monkeypatch.setenv(TRACE, "1")
    train, queries, statuses, singles = mixed
    kw = {} if chunk == 64 else {"workspace_bytes": _workspace_for(chunk, 60, 80)}
    e = _engine(kn, train, 5, **kw)
    capfd.readouterr()
    rc_, out, counts, st = _raw_batch(kn, e, queries, 40)
    assert rc_ == kn.OK and st.tolist() == [getattr(kn, s) for s in statuses]
    chunks, revised, _ = _trace(capfd)
    in_chunk = [q for q, s in zip(queries, statuses) if s == "OK" or q[0] == CHANGER and len(q[1]) < 17]  # (two are refused on the host)
    with_removals = [q for q in in_chunk if len(q[1])]
    if chunk == 64:
        assert [x[0] for x in chunks] == [37] and chunks[0][2] == 1
        assert revised == [(len(with_removals), sum(len(q[1]) for q in with_removals), 1)]
    else:  # (queries 10 .. 15 fill whole chunks of 1 and of 2: a chunk without an answerable query has no answer stage, no line)
        assert max(x[0] for x in chunks) == chunk
        answered = [q for q, s in zip(queries, statuses) if s == "OK" and len(q[1])]
        assert sum(x[0] for x in revised) == len(answered) and sum(x[1] for x in revised) == sum(len(q[1]) for q in answered)
        assert sum(x[2] for x in revised) == 1
    assert "query 10" in e._lib.knncf_last_error(e._h).decode()
    for b, s in enumerate(statuses):
        if s != "OK":
            assert counts[b] == 0 and all((a[b] == FILL).all() for a in out), b
            continue
        uc.same_answer([a[b, :counts[b]] for a in out], singles[b], (chunk, b))
        assert all((a[b, counts[b]:] == FILL).all() for a in out), b
    rows, st2 = kn.EnteredQueries(e).entered_with_batch([(q[0], q[2], q[3]) for q in queries], removed=[q[1] for q in queries])
    assert st2.tolist() == st.tolist() and [len(r[0]) for r in rows] == counts.tolist()
    free = _free_device_bytes()
    _raw_batch(kn, e, queries, 40)  # a repeated call of the same shape allocates no device memory
    assert _free_device_bytes() >= free
    assert kn.EnteredQueries(e).entered_with_batch([], removed=[])[0] == []
    e.close()


def test_jaccard_batch(kn, oracle, mixed):
    train, queries, statuses, _ = mixed
    e = _engine(kn, train, 5, JAC)
    rows, st = kn.EnteredQueries(e).entered_with_batch([(q[0], q[2], q[3]) for q in queries], removed=[q[1] for q in queries])
    assert st.tolist() == [getattr(kn, s) for s in statuses]
    for j in (0, 1, 2, 4, 8, 17, 38):
        uc.same_answer(rows[j], rc.expected_for(oracle, train, *queries[j], 5, JAC), j)
    e.close()


# ---- fixed-size edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", uc.EDGE_KS)
def test_list_block_edges(kn, synth, oracle, k):
    """full lists of 63, 64, 65, 128 and 129 cells on a fit of 140 users, the changer stored at positions 0, 63, 64 and last
    (tests/test_revise_entered_premises.py): the 64-cell steps of k_enu_locate and k_enu_place.  Half of its rows removed, and
    three: the changer moves up in some lists and out of others"""
    train = uc.scaled(synth, uc.EDGE_USERS)
    c = uc.edge_changer(oracle, train, k)
    e = _engine(kn, train, k)
    for n in rc.edge_removals(train, c):
        removed = rc.removed_rows(train, c, n)
        want = rc.expected_for(oracle, train, c, removed, [], [], k, COS)
        assert uc.edge_positions(k) <= set(want[3].tolist())
        uc.same_answer(kn.EnteredQueries(e).entered_with(c, [], [], removed=removed), want, (k, n))
    e.close()


@pytest.mark.parametrize("n_users", uc.EDGE_FITS)
def test_bitmap_word_edges(kn, synth, oracle, n_users):
    """fits of 64, 65, 128 and 129 users with the changer at dense index 63, 64 and U - 1: one and two words of the report bitmap,
    the filter and the ballots at their edges; k = U - 1 reports the users at those indices, k = 7 is selective"""
    train = uc.scaled(synth, n_users)
    order = uc.dense_order(oracle, train)
    for k in (n_users - 1, 7):
        e = _engine(kn, train, k)
        queries = [(order[at], rc.removed_rows(train, order[at], 3), NONE, np.empty(0)) for at in uc.edge_indices(n_users)]
        rows, st = kn.EnteredQueries(e).entered_with_batch([(q[0], q[2], q[3]) for q in queries], removed=[q[1] for q in queries])
        assert st.tolist() == [kn.OK] * len(queries)
        for q, got in zip(queries, rows):
            want = rc.expected_for(oracle, train, *q, k, COS)
            uc.same_answer(got, want, (n_users, k, q[0]))
            if k == 7:
                assert 0 < len(want[0]) < n_users - 1
        e.close()


# ---- the other calls ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", [COS, JAC])
def test_consistent_with_the_bystander_and_neighbour_calls(kn, answers, sim):
    """for every fitted v: c is in knncf_revise_bystander_neighbors' row at out_pos and in knncf_neighbors_batch's at out_prev,
    with the same bits, and v is reported iff the rule says so"""
    c, _ = answers["removes-3", 20, sim]
    e = _engine(kn, c.train, c.k, sim)
    users, sims, pos, prev, other = _ask(kn, e, c)
    fitted = [v for v in c.others if v != bc.UNKNOWN_USER]
    after = kn.BystanderQueries(e).neighbors_with(c.q, c.items, c.ratings, fitted, cap=c.k, removed=c.removed)
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
def test_handle_state(kn, synth, answers, tmp_path, history):
    """the call leaves the handle as knncf_neighbors_batch over the missing users in ascending raw id does — also after its tail
    rows went through the revise bystander path: the checkpoint bytes, the answers and a later mae are those of a twin handle"""
    c, want = answers["removes-3", 5, COS]
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
            got = _ask(kn, e, c)
        else:
            e.neighbors_batch(np.asarray([v for v in users.tolist() if v not in done], dtype=np.int32))
        e.neighbors_save(str(tmp_path / f"{tag}.1"))
        again = _ask(kn, e, c)
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
    c = rc.removes_3(synth, 5)
    tiny = rc.tiny_changer(synth, oracle)
    e = _engine(kn, tiny.train, tiny.k, COS)  # the adjusted cosine with TRAIN users of <= 4 ratings
    for call in (lambda: _ask(kn, e, tiny),
                 lambda: kn.EnteredQueries(e).entered_with_batch([(tiny.q, [], [])], removed=[tiny.removed]),
                 lambda: kn.EnteredQueries(e).entered_with_batch([], removed=[])):
        with pytest.raises(kn.KnncfError) as err:
            call()
        assert err.value.status == kn.E_UNSUPPORTED and "<= 4 ratings" in str(err.value)
    e.close()
    e = _engine(kn, tiny.train, tiny.k, JAC)  # Jaccard is accepted: a fitted changer of 4 train ratings that removes one
    want = rc.expected(oracle, tiny, JAC)
    assert len(want[0]) > 0
    uc.same_answer(_ask(kn, e, tiny), want, "tiny changer")
    e.close()
    e = kn.Engine(k=5, similarity=kn.SIM_ONE)
    e.fit(*c.train)
    with pytest.raises(kn.KnncfError) as err:
        _ask(kn, e, c)
    assert err.value.status == kn.E_UNSUPPORTED
    e.close()
    e = kn.Engine(k=5)
    with pytest.raises(kn.KnncfError) as err:
        kn.EnteredQueries(e).entered_with_batch([(c.q, c.items, c.ratings)], cap=3, removed=[c.removed])
    assert err.value.status == kn.E_STATE
    e.close()
    e = kn.Engine(k=5, shard_rank=0, shard_count=2)  # a shard handle
    e.fit(*c.train)
    with pytest.raises(kn.KnncfError) as err:
        _ask(kn, e, c)
    assert err.value.status == kn.E_UNSUPPORTED
    e.close()
