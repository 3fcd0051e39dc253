"""Entered queries (knncf_query_entered / _batch, csrc/entered.hip): the fitted users whose neighbour list a newcomer joins, with
the newcomer's similarity and position there and the user it displaces, without a refit.  Every answer is compared, ids and
bits, with the oracle on aug = train ++ the newcomer's rows: a fresh pipeline per fitted user.  The inputs are those of
tests/entered_cases.py (tests/test_entered_premises.py shows what they reach)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import bystander_cases as bc
from tests import entered_cases as ec
from tests.query_helpers import _bits, _workspace_for

pytestmark = pytest.mark.gpu

i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
FILL = -7


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def cases(synth, oracle):
    return {c.name: c for c in ec.all_cases(synth, oracle)}


@pytest.fixture(scope="module")
def answers(oracle, cases):
    return {(name, sim): ec.expected(oracle, c, sim) for name, c in cases.items() for sim in c.note["sims"]}


def _engine(kn, train, k, sim=ec.COS, **kw):
    e = kn.Engine(k=k, similarity=ec.sim_kind(kn, sim), **kw)
    e.fit(*train)
    return e


def _raw_batch(kn, e, queries, cap, null=False):
    """knncf_query_entered_batch on FILL-filled arrays: (status of the call, (users, sims, pos, displaced) [B, cap], counts,
    statuses)"""
    us, off, it, rt = e._query_batch(queries)
    B, p = len(us), e._ptr
    out = (np.full((B, cap), FILL, dtype=np.int32), np.full((B, cap), float(FILL)), np.full((B, cap), FILL, dtype=np.int32),
           np.full((B, cap), FILL, dtype=np.int32))
    counts = np.full(B, FILL, dtype=np.int32)
    st = np.full(B, FILL, dtype=np.int32)
    ptrs = [None] * 4 if null else [p(a.reshape(-1), t) for a, t in zip(out, (i32p, f64p, i32p, i32p))]
    rc = e._lib.knncf_query_entered_batch(e._h, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), B, cap, *ptrs, p(counts, i32p),
                                          p(st, i32p))
    return rc, out, counts, st


SINGLE = [(name, sim) for name in ec.NAMES for sim in (ec.COS, ec.JAC)
          if not (name.startswith("tiny-") and name != "tiny-newcomer" and sim == ec.COS)]


@pytest.mark.parametrize("name,sim", SINGLE)
def test_cases_single_form(kn, cases, answers, oracle, name, sim):
    c = cases[name]
    want = answers[name, sim] if (name, sim) in answers else ec.expected(oracle, c, sim)
    e = _engine(kn, c.train, c.k, sim)
    ec.same_answer(kn.EnteredQueries(e).entered(c.q, c.items, c.ratings), want, (name, sim))
    if sim in c.note["count"]:
        assert len(want[0]) == c.note["count"][sim]
    e.close()


BASE_K5 = ("near-clone", "anti-clone", "tiny-newcomer", "new-item")
BATCHES = [(BASE_K5, ec.COS), (BASE_K5, ec.JAC), (("short-59", "anti-clone-59"), ec.COS), (("tiny-1", "tiny-4", "tiny-5"), ec.JAC)]


@pytest.mark.parametrize("names,sim", BATCHES)
def test_cases_batch_form_per_train(kn, oracle, cases, answers, names, sim):
    """the cases of one train set (and one k, which belongs to the handle) in one call; a case that stands alone on its handle
    has nothing to share a call with: the single form is the batch of one"""
    group = [cases[n] for n in names]
    assert all(c.k == group[0].k and all(np.array_equal(x, y) for x, y in zip(c.train, group[0].train)) for c in group)
    e = _engine(kn, group[0].train, group[0].k, sim)
    rows, st = kn.EnteredQueries(e).entered_batch([(c.q, c.items, c.ratings) for c in group])
    assert st.tolist() == [kn.OK] * len(group)
    for c, got in zip(group, rows):
        want = answers[c.name, sim] if (c.name, sim) in answers else ec.expected(oracle, c, sim)
        ec.same_answer(got, want, (c.name, sim))
    e.close()


def test_consistent_with_bystander_rows(kn, cases):
    """row v of knncf_query_bystander_neighbors holds q iff v is reported, at out_pos, with the same similarity bits"""
    c = cases["near-clone"]
    e = _engine(kn, c.train, c.k)
    users, sims, pos, disp = kn.EnteredQueries(e).entered(c.q, c.items, c.ratings)
    rows = kn.BystanderQueries(e).neighbors_for(c.q, c.items, c.ratings, c.others, cap=c.k)
    before = e.neighbors_batch(np.asarray(c.others, dtype=np.int32))[0]
    seen = 0
    for v, (ids, ss), ids0 in zip(c.others, rows, before):
        ids = ids.tolist()
        if v not in users.tolist():
            assert c.q not in ids, v
            continue
        at = users.tolist().index(v)
        assert ids.index(c.q) == pos[at] and _bits([ss[pos[at]]]) == _bits([sims[at]]), v
        assert [x for x in ids0.tolist() if x not in ids] == [disp[at]], v
        seen += 1
    assert seen == len(users) == 11
    e.close()


def test_cap(kn, cases, answers):
    c = cases["near-clone"]
    want = answers["near-clone", ec.COS]
    e = _engine(kn, c.train, c.k)
    q = [(c.q, c.items, c.ratings)]
    rc, _, counts, st = _raw_batch(kn, e, q, 0, null=True)  # count only
    assert (rc, counts.tolist(), st.tolist()) == (kn.OK, [len(want[0])], [kn.OK])
    cnt = C.c_int32(FILL)
    p = e._ptr
    it, rt = np.asarray(c.items, dtype=np.int32), np.asarray(c.ratings, dtype=np.float64)
    assert e._lib.knncf_query_entered(e._h, c.q, p(it, i32p), p(rt, f64p), len(it), 0, None, None, None, None, C.byref(cnt)) == kn.OK
    assert cnt.value == len(want[0])
    rc, out, counts, st = _raw_batch(kn, e, q, 3)  # the first three in set order, the rest untouched
    assert (rc, counts.tolist()) == (kn.OK, [len(want[0])]) and len(want[0]) > 3
    ec.same_answer([a[0] for a in out], [w[:3] for w in want], "cap 3")
    rc, out, counts, st = _raw_batch(kn, e, q, 20)
    ec.same_answer([a[0, :counts[0]] for a in out], want, "cap 20")
    assert (out[0][0, counts[0]:] == FILL).all() and (out[1][0, counts[0]:] == FILL).all()
    assert (out[2][0, counts[0]:] == FILL).all() and (out[3][0, counts[0]:] == FILL).all()
    assert e._lib.knncf_query_entered_batch(e._h, None, None, None, None, 0, 5, None, None, None, None, None, None) == kn.OK
    assert e._lib.knncf_query_entered_batch(e._h, None, None, None, None, -1, 5, None, None, None, None, None, None) == kn.E_INVALID
    assert _raw_batch(kn, e, q, 3, null=True)[0] == kn.E_INVALID
    e.close()


def test_statuses(kn, cases, answers):
    """refused queries in the middle of a batch leave their rows untouched and the others alone; one raw id may be the
    newcomer of two queries"""
    c, t = cases["near-clone"], cases["tiny-newcomer"]
    dup = (1001, np.concatenate([c.items[:3], c.items[:1]]).astype(np.int32), np.array([4.0, 3.0, 2.0, 1.0]))
    queries = [(c.q, c.items, c.ratings), (c.others[3], c.items, c.ratings), (c.q, t.items, t.ratings), dup, (c.q, [], []),
               (t.q, t.items, t.ratings)]
    statuses = [kn.OK, kn.E_INVALID, kn.OK, kn.E_DUPLICATE, kn.E_INVALID, kn.OK]
    e = _engine(kn, c.train, c.k)
    rc, out, counts, st = _raw_batch(kn, e, queries, 20)
    assert rc == kn.OK and st.tolist() == statuses
    assert "query 1" in e._lib.knncf_last_error(e._h).decode()
    single = kn.EnteredQueries(e)
    for b, q in enumerate(queries):
        if statuses[b] != kn.OK:
            assert counts[b] == 0 and all((a[b] == FILL).all() for a in out), b
            if len(q[1]):
                with pytest.raises(kn.KnncfError) as err:
                    single.entered(*q)
                assert err.value.status == statuses[b] and "query: " in str(err.value)
            continue
        ec.same_answer([a[b, :counts[b]] for a in out], single.entered(*q), b)
    ec.same_answer([a[0, :counts[0]] for a in out], answers["near-clone", ec.COS], "first")
    # the same rows under another newcomer id: the set-order rank differs, the similarities need not (the norm's fold order)
    ec.same_answer([a[5, :counts[5]] for a in out], answers["tiny-newcomer", ec.COS], "last")
    rows, st2 = single.entered_batch(queries)
    assert st2.tolist() == statuses and [len(r[0]) for r in rows] == counts.tolist()
    assert single.entered_batch([])[0] == []
    # the single form: *count = 0 once the argument checks pass, whatever the query's status
    cnt = C.c_int32(FILL)
    p = e._ptr
    it, rt = np.asarray(c.items, dtype=np.int32), np.asarray(c.ratings, dtype=np.float64)
    ids, pos, disp = (np.full(4, FILL, dtype=np.int32) for _ in range(3))
    sims = np.full(4, float(FILL))
    assert e._lib.knncf_query_entered(e._h, int(c.others[3]), p(it, i32p), p(rt, f64p), len(it), 4, p(ids, i32p), p(sims, f64p),
                                      p(pos, i32p), p(disp, i32p), C.byref(cnt)) == kn.E_INVALID
    assert cnt.value == 0 and (ids == FILL).all()
    e.close()


def test_refusals_of_the_handle(kn, cases):
    c, tiny = cases["near-clone"], cases["tiny-4"]
    e = _engine(kn, tiny.train, tiny.k, ec.COS)  # the adjusted cosine with train users of <= 4 ratings
    for call in (lambda: kn.EnteredQueries(e).entered(tiny.q, tiny.items, tiny.ratings),
                 lambda: kn.EnteredQueries(e).entered_batch([(tiny.q, tiny.items, tiny.ratings)]),
                 lambda: kn.EnteredQueries(e).entered_batch([])):
        with pytest.raises(kn.KnncfError) as err:
            call()
        assert err.value.status == kn.E_UNSUPPORTED and "<= 4 ratings" in str(err.value)
    e.close()
    e = kn.Engine(k=5, similarity=kn.SIM_ONE)
    e.fit(*c.train)
    with pytest.raises(kn.KnncfError) as err:
        kn.EnteredQueries(e).entered(c.q, c.items, c.ratings)
    assert err.value.status == kn.E_UNSUPPORTED
    e.close()
    e = kn.Engine(k=5)
    with pytest.raises(kn.KnncfError) as err:
        kn.EnteredQueries(e).entered(c.q, c.items, c.ratings)
    assert err.value.status == kn.E_STATE
    with pytest.raises(kn.KnncfError) as err:
        kn.EnteredQueries(e).entered_batch([(c.q, c.items, c.ratings)], cap=3)
    assert err.value.status == kn.E_STATE
    e.close()


# ---- chunks and forms: the answers do not depend on how the queries travel ---------------------------------------------------
def _many_queries(synth, oracle, n=65):
    """n newcomers on the base fit: the rows of fitted user j % 60 rotated by j with one rating changed; every fifth has 4 or
    fewer rows in reverse trie order, so both similarity forms meet a newcomer whose pairs the fitted user folds differently"""
    train = bc.base_train(synth)
    users = bc._users(train)
    out = []
    for j in range(n):
        it, rt = bc._rows(train, users[j % 60])
        it, rt = np.roll(it, j), np.roll(rt, j)
        rt[0] = 1.5 if rt[0] != 1.5 else 2.5
        if j % 5 == 4:
            keep = 1 + j % 4
            order = [it.tolist().index(x) for x in bc.trie_sorted(oracle, it[:keep + 3])[::-1]][:keep]
            it, rt = it[order], rt[order]
        out.append((2000 + j, it.astype(np.int32), rt.copy()))
    return train, out


@pytest.fixture(scope="module")
def many(kn, synth, oracle):
    train, queries = _many_queries(synth, oracle)
    e = _engine(kn, train, 5)
    singles = [kn.EnteredQueries(e).entered(*q) for q in queries]
    e.close()
    assert sum(len(q[1]) <= 4 for q in queries) == 13 and min(len(s[0]) for s in singles) == 0 and max(len(s[0]) for s in singles) > 8
    return train, queries, singles


def test_single_calls_of_the_chunk_inputs_are_the_oracles(oracle, many):
    train, queries, singles = many
    for j in (0, 4, 9, 14, 19, 64):  # (9, 14, 19, 64: newcomers of 2, 3, 4 and 1 rows)
        ec.same_answer(singles[j], ec.expected_for(oracle, train, *queries[j], 5, ec.COS), j)


@pytest.mark.parametrize("n,chunk", [(65, 64), (31, 64), (32, 64), (33, 64), (7, 1), (7, 3)])
def test_chunks_and_similarity_forms(kn, many, n, chunk):
    """65 queries are two chunks at C = 64; 31 and 32 answerable queries are the two sides of QB_DUAL_MIN (with a refused query in
    front: 32 slots of which 31 are answered would be the other form); a workspace that forces C = 1, and C = 3"""
    train, queries, singles = many
    kw = {} if chunk == 64 else {"workspace_bytes": _workspace_for(chunk, 60, 80)}
    e = _engine(kn, train, 5, **kw)
    rows, st = kn.EnteredQueries(e).entered_batch(queries[:n])
    assert st.tolist() == [kn.OK] * n
    for j in range(n):
        ec.same_answer(rows[j], singles[j], (n, chunk, j))
    if n == 31:  # a query refused on the host takes no slot: still 31 slots
        rows, st = kn.EnteredQueries(e).entered_batch([(int(train[0][0]), queries[0][1], queries[0][2])] + queries[:n])
        assert st.tolist() == [kn.E_INVALID] + [kn.OK] * n
        for j in range(n):
            ec.same_answer(rows[j + 1], singles[j], (n, "refused in front", j))
    e.close()


def test_jaccard_chunk(kn, oracle, many):
    train, queries, _ = many
    e = _engine(kn, train, 5, ec.JAC)
    rows, st = kn.EnteredQueries(e).entered_batch(queries[:40])
    assert st.tolist() == [kn.OK] * 40
    for j in (0, 4, 9, 39):
        ec.same_answer(rows[j], ec.expected_for(oracle, train, *queries[j], 5, ec.JAC), j)
        ec.same_answer(rows[j], kn.EnteredQueries(e).entered(*queries[j]), j)
    e.close()


# ---- kernel edges ------------------------------------------------------------------------------------------------------------
def _scaled(synth, n_users):
    t = synth.syn_scaled(n_users, 90, 24 * n_users, 11).train
    train = (t.users.copy(), t.items.copy(), t.ratings.copy())
    assert len(np.unique(train[0])) == n_users and np.unique(train[0], return_counts=True)[1].min() > 4
    return train


@pytest.mark.parametrize("n_users,k", [(255, 7), (256, 7), (257, 7), (255, 300), (256, 300), (257, 300), (257, 256), (257, 100)])
def test_scan_block_edges(kn, synth, oracle, n_users, k):
    """fits of 255, 256 and 257 users: 4 | 5 words of the entered-user bitmap that k_en_compact scans (not the scan's
    per-thread edge: a thread owns more than one word only beyond 65 536 users; tests/test_gpu_query_edges.py covers that edge
    through the shared block_exclusive_scan); k >= U enters everybody (counts of 255 .. 257, across 64 and 256), k = U - 1 = 256
    has full lists, k = 100 a count in between"""
    train = _scaled(synth, n_users)
    c = bc.near_clone(synth, k=k, train=train)
    want = ec.expected_for(oracle, train, c.q, c.items, c.ratings, k, ec.COS)
    if k >= n_users:
        assert len(want[0]) == n_users and (want[3] == -1).all()
    if k == 100:
        assert 64 < len(want[0]) < 256
    e = _engine(kn, train, k)
    ec.same_answer(kn.EnteredQueries(e).entered(c.q, c.items, c.ratings), want, (n_users, k))
    e.close()


@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_list_block_edges(kn, synth, oracle, k):
    """k = 1, 63, 64 and 65 on a fit of 130 users: lists of one cell, and of one cell less than, exactly and one more than the
    64 cells a wave counts at a time"""
    train = _scaled(synth, 130)
    c = bc.near_clone(synth, k=k, train=train)
    want = ec.expected_for(oracle, train, c.q, c.items, c.ratings, k, ec.COS)
    assert 0 < len(want[0]) < 130
    # the same rows with every rating r as 6 - r: a newcomer near the end of the lists it enters
    anti = np.round(6.0 - c.ratings, 2)
    far = ec.expected_for(oracle, train, c.q, c.items, anti, k, ec.COS)
    assert len(far[0]) < 130 and (k < 64 or far[2].max() == k - 1)  # (k = 64, 65: positions 63 and 64, around the block edge)
    e = _engine(kn, train, k)
    ec.same_answer(kn.EnteredQueries(e).entered(c.q, c.items, c.ratings), want, k)
    ec.same_answer(kn.EnteredQueries(e).entered(c.q, c.items, anti), far, (k, "anti"))
    rows, st = kn.EnteredQueries(e).entered_batch([(c.q, c.items, anti), (c.q, c.items, c.ratings)], cap=len(want[0]) + 2)
    ec.same_answer(rows[1], want, (k, "batch"))
    ec.same_answer(rows[0], tuple(a[:len(want[0]) + 2] for a in far), (k, "batch, anti"))
    e.close()


# ---- handle state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", [False, True])
def test_handle_state(kn, synth, cases, answers, tmp_path, history):
    """the call leaves the handle as knncf_neighbors_batch over the missing users in ascending raw id does: the checkpoint bytes,
    the answers and a later mae are those of a twin handle that made that call instead"""
    c = cases["near-clone"]
    t = synth.syn_scaled(60, 80, 1500, 3).test
    users = np.sort(np.asarray(c.others, dtype=np.int32))
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
            got = kn.EnteredQueries(e).entered(c.q, c.items, c.ratings)
        else:
            e.neighbors_batch(np.asarray([v for v in users.tolist() if v not in done], dtype=np.int32))
        e.neighbors_save(str(tmp_path / f"{tag}.1"))
        again = kn.EnteredQueries(e).entered(c.q, c.items, c.ratings)
        e.neighbors_save(str(tmp_path / f"{tag}.2"))
        mae = e.mae(kn.PRED_KNN, t.users, t.items, t.ratings)
        e.close()
        return got, again, mae

    got, again, mae = session("a", True)
    _, twin, twin_mae = session("b", False)
    ec.same_answer(got, answers["near-clone", ec.COS], "first call")
    ec.same_answer(again, got, "second call")
    ec.same_answer(twin, got, "twin")
    a1, a2, b1, b2 = ((tmp_path / n).read_bytes() for n in ("a.1", "a.2", "b.1", "b.2"))
    assert a1 == b1, "the state knncf_neighbors_batch over M leaves"
    assert a1 == a2 and b1 == b2, "a second call changes no byte"
    assert _bits([mae]) == _bits([twin_mae])


def test_build_happens_when_no_query_is_answerable(kn, cases, tmp_path):
    """M is built once the handle-level checks pass, also when every query is refused"""
    c = cases["near-clone"]
    users = np.sort(np.asarray(c.others, dtype=np.int32))
    e = _engine(kn, c.train, c.k)
    rows, st = kn.EnteredQueries(e).entered_batch([(int(users[0]), c.items, c.ratings)], cap=4)
    assert st.tolist() == [kn.E_INVALID]
    e.neighbors_save(str(tmp_path / "a"))
    e.close()
    e = _engine(kn, c.train, c.k)
    e.neighbors_batch(users)
    e.neighbors_save(str(tmp_path / "b"))
    e.close()
    assert (tmp_path / "a").read_bytes() == (tmp_path / "b").read_bytes()
