"""Bystanders of update queries (knncf_update_bystander_neighbors / _predict and their batched forms, csrc/bystander.hip): the
neighbours and kNN predictions of a FITTED user once another user — of the fit or not — has added ratings, without a refit.
Every row is compared bit for bit, ids and values, with the oracle on aug = train ++ the additional rows, on a fresh pipeline
per row whose first evaluation is that row's.  The inputs are those of tests/update_bystander_cases.py
(tests/test_update_bystander_premises.py shows what they reach).  The `knncf-dispatch bystander` line of
KNNCF_DEBUG_TRACE_DISPATCH says which kinds of changer a chunk held."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import bystander_cases as bc
from tests import update_bystander_cases as uc
from tests.query_helpers import UNKNOWN_ITEM, _aug, _bits, _same_pair, _workspace_for
from tests.test_gpu_personalized_explain import _free_device_bytes
from tests.test_gpu_update import _hold_out, _syn100k

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
NAMES = ["adds-3", "leaves-short-59", "leaves-short-300", "new-item", "negative", "fold-place", "tiny-changer", "tiny-bystanders",
         "tie-before", "tie-after"]


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def cases(synth, oracle):
    return {c.name: c for c in uc.all_cases(synth, oracle)}


def _trace(capfd):
    """(slots, fitted, merge) of every bystander chunk since the last read"""
    err = capfd.readouterr().err
    return [tuple(int(x) for x in m.groups()) for m in re.finditer(r"knncf-dispatch bystander slots=(\d+) fitted=(\d+) merge=(\d+)", err)]


def _grid(c):
    """every (bystander, item) of the case as rows"""
    pi = c.pred_items
    return np.repeat(np.asarray(c.others, dtype=np.int32), len(pi)), np.tile(pi, len(c.others))


def _check_case(kn, oracle, c, sim, esim, capfd):
    want_nb, want_pr = uc.expected(oracle, c, sim)
    e = kn.Engine(k=c.k, similarity=esim)
    e.fit(*c.train)
    by = kn.BystanderQueries(e)
    capfd.readouterr()
    got_nb = by.neighbors_with(c.q, c.items, c.ratings, c.others, cap=61)
    others, items = _grid(c)
    got_pr = by.predict_with(c.q, c.items, c.ratings, others, items).reshape(len(c.others), -1)
    lines = _trace(capfd)
    assert lines and all(f == 1 and m == 0 for _, f, m in lines), lines  # one fitted changer per chunk, no merge
    assert lines[0][0] == 60  # the changer's slot and 59 fitted bystanders: the whole-chunk similarity kernel
    for j, v in enumerate(c.others):
        _same_pair(got_nb[j], want_nb[j], (c.name, v))
        assert _bits(got_pr[j]) == _bits(want_pr[j]), (c.name, v)
    e.close()
    return got_nb


@pytest.mark.parametrize("name", NAMES)
def test_cases_cosine(kn, oracle, cases, capfd, monkeypatch, name):
    monkeypatch.setenv(TRACE, "1")
    c = cases[name]
    nb = _check_case(kn, oracle, c, oracle.SIM_COSINE, kn.SIM_COSINE, capfd)
    fitted = [j for j, v in enumerate(c.others) if v != bc.UNKNOWN_USER]
    assert all(len(nb[j][0]) == min(c.k, 59) for j in fitted)
    assert len(nb[c.others.index(bc.UNKNOWN_USER)][0]) == min(c.k, 60)  # |users(aug)| = U for a fitted changer


@pytest.mark.parametrize("name", uc.JACCARD_CASES)
def test_cases_jaccard(kn, oracle, cases, capfd, monkeypatch, name):
    monkeypatch.setenv(TRACE, "1")
    c = cases[name]
    nb = _check_case(kn, oracle, c, oracle.SIM_JACCARD, kn.SIM_JACCARD, capfd)
    if name.startswith("tie"):  # the changer and the user it ties with on both sides of the cut
        ids = nb[c.others.index(c.note["bystander"])][0].tolist()
        assert (c.q in ids) != (c.note["tied_with"] in ids)
        assert ids[-1] == (c.q if c.note["side"] == "before" else c.note["tied_with"])


# ---- identities ---------------------------------------------------------------------------------------------------------------
def test_an_absent_changer_is_the_fold_in_case(kn, synth, oracle, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    for c in (bc.near_clone(synth), bc.new_item(synth)):
        e = kn.Engine(k=c.k)
        e.fit(*c.train)
        by = kn.BystanderQueries(e)
        others = c.others + [bc.UNKNOWN_USER]
        capfd.readouterr()
        got = by.neighbors_with(c.q, c.items, c.ratings, others, cap=61)
        assert _trace(capfd) == [(61, 0, 60)]
        for a, b in zip(got, by.neighbors_for(c.q, c.items, c.ratings, others, cap=61)):
            _same_pair(a, b, c.name)
        rows = (np.repeat(np.asarray(others, dtype=np.int32), len(c.pred_items)), np.tile(c.pred_items, len(others)))
        assert _bits(by.predict_with(c.q, c.items, c.ratings, *rows)) == _bits(by.predict_for(c.q, c.items, c.ratings, *rows))
        with pytest.raises(kn.KnncfError) as err:  # the exception: an empty query of an absent user
            by.neighbors_with(c.q, [], [], others)
        assert err.value.status == kn.E_INVALID
        e.close()


@pytest.mark.parametrize("sim", ["cosine", "jaccard"])
def test_no_additional_rows_is_the_train_answer(kn, cases, sim):
    c = cases["tiny-bystanders"]  # (tiny users among the bystanders: fresh closures on train)
    e = kn.Engine(k=c.k, similarity=kn.SIM_COSINE if sim == "cosine" else kn.SIM_JACCARD)
    e.fit(*c.train)
    by = kn.BystanderQueries(e)
    fitted = [v for v in c.others if v != bc.UNKNOWN_USER]
    pi = c.pred_items
    nb = by.neighbors_with(c.q, [], [], fitted)
    pr = by.predict_with(c.q, [], [], np.repeat(np.asarray(fitted, dtype=np.int32), len(pi)), np.tile(pi, len(fitted))).reshape(len(fitted), -1)
    for j, v in enumerate(fitted):
        _same_pair(nb[j], e.neighbors_with(v, [], []), v)
        assert _bits(pr[j]) == _bits(e.predict_with(v, [], [], pi)), v
    e.close()


def _batch_inputs(kn, synth, cases):
    """queries on the base fit: a fitted changer with 5 bystanders, a newcomer, a fitted changer without rows, a repeated item
    against the train rows, a row that names the changer, a fitted changer whose rows name a new item (a bystander twice, an
    unknown one)"""
    a, n, f = cases["adds-3"], cases["new-item"], bc.near_clone(synth)
    users = [u for u in a.others if u != bc.UNKNOWN_USER]
    mine = a.train[1][a.train[0] == 9]
    queries = [(a.q, a.items, a.ratings), (f.q, f.items, f.ratings), (7, np.empty(0, dtype=np.int32), np.empty(0)),
               (9, np.asarray([uc.unrated(a.train, 9, 1)[0], mine[1]], dtype=np.int32), np.asarray([4.0, 3.0])),
               (11, uc.unrated(a.train, 11, 1), np.asarray([2.5])), (n.q, n.items, n.ratings)]
    others = [[users[0], users[9], users[20], users[30], users[40]], [5, users[1], users[2], users[3], users[50]],
              [users[0], 5, users[8]], users[:5], [users[1], 11, users[3]], [users[50], users[12], bc.UNKNOWN_USER, users[13], users[50]]]
    items = [[int(a.train[1][0]), int(a.train[1][5]), bc.NEW_ITEM, UNKNOWN_ITEM, int(a.items[0])][:len(o)] for o in others]
    return a, queries, others, items, [kn.OK, kn.OK, kn.OK, kn.E_DUPLICATE, kn.E_INVALID, kn.OK]


@pytest.mark.parametrize("chunk", [2, 3, 64])
def test_batch_chunks_statuses_and_permutation(kn, synth, cases, capfd, monkeypatch, chunk):
    """the rows of a batch are the single calls' at every chunk size (at 2 and 3 a query's bystanders continue into the next
    chunk, where its row is prepared again); failed queries leave their rows untouched; permuting the queries permutes the rows"""
    monkeypatch.setenv(TRACE, "1")
    c, queries, others, items, statuses = _batch_inputs(kn, synth, cases)
    e = kn.Engine(k=c.k, workspace_bytes=_workspace_for(chunk, 60, 80))
    e.fit(*c.train)
    ref = kn.Engine(k=c.k)
    ref.fit(*c.train)
    by, rby = kn.BystanderQueries(e), kn.BystanderQueries(ref)
    capfd.readouterr()
    nb, st = by.neighbors_with_batch(queries, others)
    lines = _trace(capfd)
    assert all(s <= chunk for s, _, _ in lines) and sum(f for _, f, _ in lines) >= 4 and sum(m for _, _, m in lines) == 5
    if chunk == 64:
        # slots: 1 + 5, 1 + 5 (the newcomer's), 1 + 3, 1 + 5 (the repeated item shows on the device), none, 1 + 3 distinct fitted
        assert lines == [(26, 4, 5)]
    else:
        assert len(lines) > 4
    pr, st2 = by.predict_with_batch(queries, others, items)
    assert st.tolist() == statuses and st2.tolist() == statuses
    for b, q in enumerate(queries):
        if statuses[b] != kn.OK:
            assert all(len(ids) == 0 for ids, _ in nb[b]) and np.isnan(pr[b]).all(), b
            with pytest.raises(kn.KnncfError) as err:  # the single form returns the query's status
                rby.predict_with(*q, others[b], items[b])
            assert err.value.status == statuses[b] and "query: " in str(err.value)
            continue
        for got, want in zip(nb[b], rby.neighbors_with(*q, others[b])):
            _same_pair(got, want, b)
        assert _bits(pr[b]) == _bits(rby.predict_with(*q, others[b], items[b])), b
    perm = [5, 3, 0, 2, 4, 1]
    nb2, st3 = by.neighbors_with_batch([queries[x] for x in perm], [others[x] for x in perm])
    pr2, _ = by.predict_with_batch([queries[x] for x in perm], [others[x] for x in perm], [items[x] for x in perm])
    assert st3.tolist() == [statuses[x] for x in perm]
    for y, x in enumerate(perm):
        assert _bits(pr2[y]) == _bits(pr[x]) or statuses[x] != kn.OK
        for got, want in zip(nb2[y], nb[x]):
            _same_pair(got, want, (y, x))
    e.close()
    ref.close()


def test_dual_kernel_chunk_mixes_changers_and_repeats_allocate_nothing(kn, synth, oracle, cases, capfd, monkeypatch):
    """one chunk of 42 slots (>= QB_DUAL_MIN: the whole-chunk similarity kernel) with a fitted changer and a newcomer, against
    the single calls (21 slots each: the per-slot kernel) and the oracle; a repeated call allocates no device memory"""
    monkeypatch.setenv(TRACE, "1")
    a, f = cases["adds-3"], bc.near_clone(synth)
    users = [u for u in a.others if u != bc.UNKNOWN_USER]
    queries = [(a.q, a.items, a.ratings), (f.q, f.items, f.ratings)]
    others = [users[:20], users[20:40]]
    items = [[int(a.items[j % 3]) for j in range(20)], [int(a.train[1][j]) for j in range(20)]]
    e = kn.Engine(k=a.k)
    e.fit(*a.train)
    by = kn.BystanderQueries(e)
    capfd.readouterr()
    nb, st = by.neighbors_with_batch(queries, others)
    pr, _ = by.predict_with_batch(queries, others, items)
    assert st.tolist() == [kn.OK, kn.OK]
    assert _trace(capfd) == [(42, 1, 20), (42, 1, 20)]
    free = _free_device_bytes()
    nb2, _ = by.neighbors_with_batch(queries, others)
    pr2, _ = by.predict_with_batch(queries, others, items)
    assert _free_device_bytes() >= free
    for b, q in enumerate(queries):
        m = oracle.Model(*_aug(a.train, *q))
        single = by.neighbors_with(*q, others[b])
        assert _bits(pr[b]) == _bits(by.predict_with(*q, others[b], items[b])) == _bits(pr2[b])
        for j, v in enumerate(others[b]):
            _same_pair(nb[b][j], single[j], (b, v))
            _same_pair(nb[b][j], nb2[b][j], (b, v))
            _same_pair(nb[b][j], m.pipeline(oracle.SIM_COSINE, a.k).neighbors(v), (b, v))
            assert _bits([pr[b][j]]) == _bits([m.pipeline(oracle.SIM_COSINE, a.k).predict(v, items[b][j])]), (b, v)
    e.close()


# ---- statuses -------------------------------------------------------------------------------------------------------------------
def test_per_query_statuses_in_a_mixed_batch(kn, cases):
    c = cases["adds-3"]
    train = c.train
    e = kn.Engine(k=c.k)
    e.fit(*train)
    by = kn.BystanderQueries(e)
    users = [u for u in c.others if u != bc.UNKNOWN_USER]
    known = 9
    mine = train[1][train[0] == known]
    free = uc.unrated(train, known, 3)
    n_over = 65_537 - len(mine)
    bad = [
        ((known, np.asarray([free[0], mine[1]], dtype=np.int32), [4.0, 3.0]), kn.E_DUPLICATE),  # against a train item
        ((known, np.asarray([free[0], free[1], free[0]], dtype=np.int32), [4.0, 3.0, 2.0]), kn.E_DUPLICATE),  # inside the rows
        ((known, free[:1], [np.inf]), kn.E_NONFINITE),
        ((known, free[:2], [-1.0e6, 2.0]), kn.E_UNSUPPORTED),  # negative combined mean
        ((7004, np.empty(0, dtype=np.int32), np.empty(0)), kn.E_INVALID),  # empty rows for an absent user
        ((known, np.arange(200_000, 200_000 + n_over, dtype=np.int32), np.full(n_over, 3.0)), kn.E_UNSUPPORTED),  # 65 537 combined rows
    ]
    good = (c.q, c.items, c.ratings)
    queries, want, others = [], [], []
    for q, status in bad:
        queries += [good, q]
        want += [kn.OK, status]
        others += [users[:3], users[3:6]]
    queries.append((known, free[:1], [3.0]))
    want.append(kn.E_INVALID)
    others.append([users[0], known])  # a row that names the changer
    items = [[int(train[1][0])] * len(o) for o in others]
    nb, st = by.neighbors_with_batch(queries, others)
    assert st.tolist() == want
    assert "query 1:" in e._lib.knncf_last_error(e._h).decode()
    pr, st = by.predict_with_batch(queries, others, items)
    assert st.tolist() == want
    single = by.neighbors_with(*good, users[:3])
    for b in range(len(queries)):
        if want[b] == kn.OK:
            for got, w in zip(nb[b], single):
                _same_pair(got, w, b)
            assert _bits(pr[b]) == _bits(by.predict_with(*good, users[:3], items[b]))
        else:
            assert all(len(x[0]) == 0 for x in nb[b]) and np.isnan(pr[b]).all()
            with pytest.raises(kn.KnncfError) as ex:
                by.neighbors_with(*queries[b], others[b])
            assert ex.value.status == want[b]
    # failed rows at the C boundary: counts 0, sentinels untouched
    us, off, it, rt = e._query_batch(queries)
    roff, oth, _ = by._rows(len(queries), others, None)
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    p = e._ptr
    ids = np.full((len(oth), 3), -7, dtype=np.int32)
    sims = np.full((len(oth), 3), -7.0)
    counts = np.full(len(oth), -7, dtype=np.int32)
    stc = np.zeros(len(queries), dtype=np.int32)
    assert e._lib.knncf_update_bystander_neighbors_batch(e._h, p(us, i32p), p(off, i64p), p(it, i32p), p(rt, f64p), len(us), p(roff, i64p),
                                                         p(oth, i32p), 3, p(ids.reshape(-1), i32p), p(sims.reshape(-1), f64p),
                                                         p(counts, i32p), p(stc, i32p)) == kn.OK
    for b in range(len(queries)):
        rows = slice(roff[b], roff[b + 1])
        if want[b] == kn.OK:
            assert (counts[rows] == c.k).all() and (ids[rows] != -7).all()
        else:
            assert (counts[rows] == 0).all() and (ids[rows] == -7).all() and (sims[rows] == -7.0).all()
    e.close()


def test_a_bystander_of_more_than_65536_train_ratings(kn):
    """six users on 65 537 items: user 1 rates all of them, the others ten each"""
    n = 65_537
    u = np.concatenate([np.full(n, 1), np.repeat(np.arange(2, 7), 10)]).astype(np.int32)
    i = np.concatenate([np.arange(1, n + 1), np.tile(np.arange(1, 11), 5) + np.repeat(np.arange(5), 10)]).astype(np.int32)
    r = ((np.arange(len(u)) * 7) % 5 + 1).astype(np.float64)
    e = kn.Engine(k=3)
    e.fit(u, i, r)
    by = kn.BystanderQueries(e)
    nb, st = by.neighbors_with_batch([(2, [40], [3.0]), (2, [40], [3.0])], [[3, 4], [3, 1]])
    assert st.tolist() == [kn.OK, kn.E_UNSUPPORTED]
    assert [len(x[0]) for x in nb[0]] == [3, 3] and [len(x[0]) for x in nb[1]] == [0, 0]
    e.close()


def test_handle_level_refusals(kn, cases):
    c = cases["adds-3"]
    train, q, it, rt = c.train, c.q, c.items, c.ratings
    good = [(q, it, rt), (1000, [4, 5], [2.0, 3.0])]
    oth, pi = [[1, 2], [3]], [[1, 2], [3]]

    def status_of(call):
        with pytest.raises(kn.KnncfError) as ex:
            call()
        return ex.value.status

    def all_four(e, status):
        by = kn.BystanderQueries(e)
        assert status_of(lambda: by.neighbors_with(q, it, rt, [1, 2])) == status
        assert status_of(lambda: by.predict_with(q, it, rt, [1, 2], [1, 2])) == status
        assert status_of(lambda: by.neighbors_with_batch(good, oth)) == status
        assert status_of(lambda: by.predict_with_batch(good, oth, pi)) == status

    e = kn.Engine(k=5)
    all_four(e, kn.E_STATE)  # before a fit
    e.fit(*train)
    lib, h, p = e._lib, e._h, e._ptr
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    o2, p2, out, st = np.asarray([1, 2], dtype=np.int32), np.asarray([1, 2], dtype=np.int32), np.empty(2), np.zeros(1, dtype=np.int32)
    it32, ids, sims, cnt = np.asarray(it, dtype=np.int32), np.empty(10, dtype=np.int32), np.empty(10), np.zeros(2, dtype=np.int32)
    predict = lambda pred, items, n, m: lib.knncf_update_bystander_predict(h, pred, q, items, p(rt, f64p), n, p(o2, i32p), p(p2, i32p), m, p(out, f64p))
    assert predict(kn.PRED_BASELINE, p(it32, i32p), 3, 2) == kn.E_UNSUPPORTED  # a predictor other than the kNN one
    assert predict(kn.PRED_PERSONALIZED, p(it32, i32p), 3, 2) == kn.E_UNSUPPORTED
    assert predict(kn.PRED_KNN, None, 3, 2) == kn.E_INVALID  # null rows with n_ratings > 0
    assert predict(kn.PRED_KNN, p(it32, i32p), -1, 2) == kn.E_INVALID
    assert predict(kn.PRED_KNN, p(it32, i32p), 3, -1) == kn.E_INVALID
    assert predict(kn.PRED_KNN, p(it32, i32p), 3, 2) == kn.OK
    assert predict(kn.PRED_KNN, None, 0, 2) == kn.OK  # a fitted user without rows
    nbrs = lambda cap, o: lib.knncf_update_bystander_neighbors(h, q, p(it32, i32p), p(rt, f64p), 3, o, 2, cap, p(ids, i32p), p(sims, f64p), p(cnt, i32p))
    assert nbrs(-1, p(o2, i32p)) == kn.E_INVALID and nbrs(5, None) == kn.E_INVALID and nbrs(5, p(o2, i32p)) == kn.OK
    us, off, roff = np.asarray([q], dtype=np.int32), np.asarray([0, 3], dtype=np.int64), np.asarray([0, 2], dtype=np.int64)
    batch = lambda B, off_, roff_: lib.knncf_update_bystander_predict_batch(h, kn.PRED_KNN, p(us, i32p), off_, p(it32, i32p), p(rt, f64p), B, roff_,
                                                                            p(o2, i32p), p(p2, i32p), p(out, f64p), p(st, i32p))
    assert batch(-1, p(off, i64p), p(roff, i64p)) == kn.E_INVALID
    assert batch(1, None, p(roff, i64p)) == kn.E_INVALID
    assert batch(1, p(np.asarray([1, 3], dtype=np.int64), i64p), p(roff, i64p)) == kn.E_INVALID  # offsets[0] != 0
    assert batch(1, p(off, i64p), p(np.asarray([0, -1], dtype=np.int64), i64p)) == kn.E_INVALID  # row_offsets decrease
    assert batch(0, None, None) == kn.OK and batch(1, p(off, i64p), p(roff, i64p)) == kn.OK
    e.close()
    e1 = kn.Engine(k=5, similarity=kn.SIM_ONE)
    e1.fit(*train)
    all_four(e1, kn.E_UNSUPPORTED)
    e1.close()
    es = kn.Engine(k=5, shard_rank=0, shard_count=2)  # a shard handle
    es.fit(*train)
    all_four(es, kn.E_UNSUPPORTED)
    es.close()
    m = np.isin(train[0], np.unique(train[0])[:4])
    e4 = kn.Engine(k=5)
    e4.fit(*(a[m] for a in train))
    all_four(e4, kn.E_UNSUPPORTED)  # fewer than 5 train users
    e4.close()


def test_empty_batches_and_rows(kn, cases):
    c = cases["adds-3"]
    e = kn.Engine(k=c.k)
    e.fit(*c.train)
    by = kn.BystanderQueries(e)
    assert by.neighbors_with_batch([], [])[0] == []
    pr, st = by.predict_with_batch([(c.q, c.items, c.ratings), (1000, [], [])], [[], []], [[], []])
    assert [len(x) for x in pr] == [0, 0] and st.tolist() == [kn.OK, kn.E_INVALID]
    assert len(by.predict_with(c.q, c.items, c.ratings, [], [])) == 0
    e.close()


@pytest.mark.parametrize("built", [True, False])
def test_handle_state(kn, synth, cases, tmp_path, built):
    """the checkpoint bytes and a later mae do not see the calls, on a handle that has built some lists and on one with none"""
    c = cases["adds-3"]
    t = synth.syn_scaled(60, 80, 1500, 3).test
    test = (t.users, t.items, t.ratings)
    users = np.asarray([u for u in c.others if u != bc.UNKNOWN_USER], dtype=np.int32)

    def session(path, with_calls):
        e = kn.Engine(k=c.k)
        e.fit(*c.train)
        if built:
            e.neighbors_batch(users[[3, 17, 40]])
        if with_calls:
            e.neighbors_save(str(path) + ".before")
            kn.BystanderQueries(e).neighbors_with(c.q, c.items, c.ratings, c.others)
            kn.BystanderQueries(e).predict_with(c.q, c.items, c.ratings, users, np.full(len(users), int(c.train[1][0]), dtype=np.int32))
            e.neighbors_save(str(path))
        mae = e.mae(kn.PRED_KNN, *test)
        e.close()
        return mae

    with_calls, fresh = session(tmp_path / "a.bin", True), session(tmp_path / "b.bin", False)
    assert (tmp_path / "a.bin.before").read_bytes() == (tmp_path / "a.bin").read_bytes()
    assert _bits([with_calls]) == _bits([fresh])


@pytest.mark.parametrize("k", [300, 10])
def test_mid_size_fitted_changers(kn, oracle, syn100k, k):
    """syn-100k in shuffled file order (a train row's file place is not its place in the user's row): eight fitted changers add
    their 5 held-out ratings; 16 bystanders each, 8 from the changer's train list and 8 not from it"""
    full = _syn100k(syn100k, shuffled=True)
    rng = np.random.default_rng(11)
    u, cnt = np.unique(full[0], return_counts=True)
    changers = [int(x) for x in rng.choice(u[cnt > 12], 8, replace=False)]
    train, rows = _hold_out(full, changers, 5)
    e = kn.Engine(k=k)
    e.fit(*train)
    by = kn.BystanderQueries(e)
    train_users, train_items = np.unique(train[0]), np.unique(train[1])
    for c in changers:
        it, rt = rows[c]
        near = [int(x) for x in e.neighbors_with(c, [], [])[0][:8]]
        far = [int(x) for x in train_users if int(x) not in near and int(x) != c]
        others = near + [int(x) for x in rng.choice(far, 8, replace=False)]
        items = np.concatenate([rng.choice(train_items, 22, replace=False), it, train[1][train[0] == c][:5]]).astype(np.int32)
        assert len(items) == 32
        m = oracle.Model(*_aug(train, c, it, rt))
        nb = by.neighbors_with(c, it, rt, others, cap=k)
        pr = by.predict_with(c, it, rt, np.repeat(np.asarray(others, dtype=np.int32), len(items)), np.tile(items, len(others))).reshape(16, 32)
        for j, v in enumerate(others):
            p = m.pipeline(oracle.SIM_COSINE, k)  # (every evaluation of this pipeline is v's: v owns every pair)
            _same_pair(nb[j], p.neighbors(v), (c, v))
            assert _bits(pr[j]) == _bits([p.predict(v, int(i)) for i in items]), (c, v)
    e.close()
