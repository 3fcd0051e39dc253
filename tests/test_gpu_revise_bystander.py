"""Bystanders of revise queries (knncf_revise_bystander_neighbors / _predict and their batched forms, csrc/bystander.hip): the
neighbours and kNN predictions of a FITTED user once another user of the fit has removed or re-rated items, without a refit.
Every row is compared bit for bit, ids and values, with the oracle on aug = train without the removed rows ++ the additional
rows, on a fresh pipeline per row whose first evaluation is that row's.  The inputs are those of
tests/revise_bystander_cases.py (tests/test_revise_bystander_premises.py shows what they reach).  The `knncf-dispatch
bystander-revise` line of KNNCF_DEBUG_TRACE_DISPATCH says how many changers with removals a chunk held and how many of their
queries had the file folded again for average(aug)."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import bystander_cases as bc
from tests import revise_bystander_cases as rc
from tests import update_bystander_cases as uc
from tests.query_helpers import UNKNOWN_ITEM, _bits, _same_pair, _workspace_for

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def cases(synth, oracle):
    return {c.name: c for c in rc.all_cases(synth, oracle)}


class _By:
    """BystanderQueries with the revise family spelled out: a query is (user, removed_items, items, ratings), which the binding
    takes as the update calls' `removed` argument"""

    def __init__(self, by):
        self._by = by

    def __getattr__(self, name):
        return getattr(self._by, name)

    @staticmethod
    def _split(queries):
        return [(q, it, rt) for q, _, it, rt in queries], [rm for _, rm, _, _ in queries]

    def neighbors_revised(self, user, removed, items, ratings, others, cap=None):
        return self._by.neighbors_with(user, items, ratings, others, cap=cap, removed=removed)

    def predict_revised(self, user, removed, items, ratings, others, pred_items):
        return self._by.predict_with(user, items, ratings, others, pred_items, removed=removed)

    def neighbors_revised_batch(self, queries, others, cap=None):
        qs, rms = self._split(queries)
        return self._by.neighbors_with_batch(qs, others, cap=cap, removed=rms)

    def predict_revised_batch(self, queries, others, pred_items):
        qs, rms = self._split(queries)
        return self._by.predict_with_batch(qs, others, pred_items, removed=rms)


def _trace(capfd):
    """((slots, fitted, merge) of every bystander chunk, (slots, removed, refold) of every bystander-revise line) since the last read"""
    err = capfd.readouterr().err
    ints = lambda pat: [tuple(int(x) for x in m.groups()) for m in re.finditer(pat, err)]
    return (ints(r"knncf-dispatch bystander slots=(\d+) fitted=(\d+) merge=(\d+)"),
            ints(r"knncf-dispatch bystander-revise slots=(\d+) removed=(\d+) refold=(\d+)"))


def _grid(c):
    pi = c.pred_items
    return np.repeat(np.asarray(c.others, dtype=np.int32), len(pi)), np.tile(pi, len(c.others))


def _check_case(kn, oracle, c, sim, esim, capfd):
    want_nb, want_pr = rc.expected(oracle, c, sim)
    e = kn.Engine(k=c.k, similarity=esim)
    e.fit(*c.train)
    by = _By(kn.BystanderQueries(e))
    capfd.readouterr()
    got_nb = by.neighbors_revised(*c.query, c.others, cap=61)
    chunks, revise = _trace(capfd)
    assert chunks == [(60, 1, 0)] and revise == [(1, len(c.removed), 0)], (chunks, revise)  # the lists need no average
    others, items = _grid(c)
    got_pr = by.predict_revised(*c.query, others, items).reshape(len(c.others), -1)
    chunks, revise = _trace(capfd)
    # one chunk: the changer's slot and the fitted bystanders of mean >= 0; UNKNOWN_USER (and a negative-mean user) are answered
    # with average(aug): a sequential fold over the file where the fit is not dyadic, none where it is
    assert len(chunks) == 1 and chunks[0][1:] == (1, 0), chunks
    assert revise == [(1, len(c.removed), 0 if rc.is_dyadic(c.train) else 1)], revise
    for j, v in enumerate(c.others):
        _same_pair(got_nb[j], want_nb[j], (c.name, v))
        assert _bits(got_pr[j]) == _bits(want_pr[j]), (c.name, v)
    e.close()
    return got_nb


@pytest.mark.parametrize("name", rc.NAMES)
def test_cases_cosine(kn, oracle, cases, capfd, monkeypatch, name):
    monkeypatch.setenv(TRACE, "1")
    c = cases[name]
    nb = _check_case(kn, oracle, c, oracle.SIM_COSINE, kn.SIM_COSINE, capfd)
    fitted = [j for j, v in enumerate(c.others) if v != bc.UNKNOWN_USER]
    assert all(len(nb[j][0]) == min(c.k, 59) for j in fitted)  # c stays a user of aug
    assert len(nb[c.others.index(bc.UNKNOWN_USER)][0]) == min(c.k, 60)
    if name == "membership":
        ids = lambda v: nb[c.others.index(v)][0].tolist()
        assert all(c.q not in ids(v) for v in c.note["leaves"]) and all(c.q in ids(v) for v in c.note["enters"])


@pytest.mark.parametrize("name", rc.JACCARD_NAMES)
def test_cases_jaccard(kn, oracle, cases, capfd, monkeypatch, name):
    monkeypatch.setenv(TRACE, "1")
    _check_case(kn, oracle, cases[name], oracle.SIM_JACCARD, kn.SIM_JACCARD, capfd)


# ---- identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim", ["cosine", "jaccard"])
def test_no_removals_is_the_update_answer(kn, synth, capfd, monkeypatch, sim):
    monkeypatch.setenv(TRACE, "1")
    c = uc.adds_3(synth)
    e = kn.Engine(k=c.k, similarity=kn.SIM_COSINE if sim == "cosine" else kn.SIM_JACCARD)
    e.fit(*c.train)
    by = _By(kn.BystanderQueries(e))
    others, items = _grid(c)
    capfd.readouterr()
    nb = by.neighbors_revised(c.q, [], c.items, c.ratings, c.others, cap=61)
    pr = by.predict_revised(c.q, [], c.items, c.ratings, others, items)
    nbb, st = by.neighbors_revised_batch([(c.q, [], c.items, c.ratings), (7, [], [], [])], [c.others[:7], c.others[:3]], cap=61)
    chunks, revise = _trace(capfd)
    assert chunks[0] == (60, 1, 0) and revise == [] and st.tolist() == [kn.OK, kn.OK]
    for a, b in zip(nb, by.neighbors_with(c.q, c.items, c.ratings, c.others, cap=61)):
        _same_pair(a, b, c.name)
    assert _bits(pr) == _bits(by.predict_with(c.q, c.items, c.ratings, others, items))
    for a, b in zip(nbb[0], nb[:7]):
        _same_pair(a, b, "batch")
    e.close()


def test_an_absent_user_without_removals_is_the_fold_in_case(kn, synth, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    c = bc.new_item(synth)
    e = kn.Engine(k=c.k)
    e.fit(*c.train)
    by = _By(kn.BystanderQueries(e))
    others = c.others + [bc.UNKNOWN_USER]
    capfd.readouterr()
    got = by.neighbors_revised(c.q, [], c.items, c.ratings, others, cap=61)
    chunks, revise = _trace(capfd)
    assert chunks == [(61, 0, 60)] and revise == []
    for a, b in zip(got, by.neighbors_for(c.q, c.items, c.ratings, others, cap=61)):
        _same_pair(a, b, c.name)
    rows = (np.repeat(np.asarray(others, dtype=np.int32), len(c.pred_items)), np.tile(c.pred_items, len(others)))
    assert _bits(by.predict_revised(c.q, [], c.items, c.ratings, *rows)) == _bits(by.predict_for(c.q, c.items, c.ratings, *rows))
    with pytest.raises(kn.KnncfError) as err:  # any removal for a user absent from train
        by.neighbors_revised(c.q, [int(c.train[1][0])], c.items, c.ratings, others)
    assert err.value.status == kn.E_INVALID
    e.close()


# ---- mixed batch ----------------------------------------------------------------------------------------------------------------
def _mixed(kn, synth, cases):
    """a newcomer, a changer without removals, a changer with removals, a second query of the same changer with other removals,
    a refused query (a removal of an item its user did not rate), and a changer with removals and no average row: 8 bystanders
    each, UNKNOWN_USER among those of the queries of user 5"""
    a, r, d, f = uc.adds_3(synth), cases["removes-3-k5"], cases["re-rates-dyadic"], bc.near_clone(synth)
    train = r.train
    users = [u for u in r.others if u != bc.UNKNOWN_USER]
    none_i, none_r = np.empty(0, dtype=np.int32), np.empty(0)
    mine11 = train[1][train[0] == 11]
    queries = [(f.q, none_i, f.items, f.ratings), (a.q, none_i, a.items, a.ratings), r.query, d.query,
               (9, uc.unrated(train, 9, 1), none_i, none_r), (11, mine11[2:4], uc.unrated(train, 11, 1), np.asarray([2.5]))]
    others = [users[0:8], users[8:15] + [bc.UNKNOWN_USER], users[16:23] + [bc.UNKNOWN_USER], users[4:11] + [bc.UNKNOWN_USER],
              users[30:38], users[40:47] + [users[40]]]
    base = [int(train[1][0]), int(r.removed[0]), int(d.items[0]), bc.NEW_ITEM, UNKNOWN_ITEM, int(d.items[1]), int(mine11[2]), int(train[1][7])]
    items = [base for _ in others]
    return train, r.k, queries, others, items, [kn.OK, kn.OK, kn.OK, kn.OK, kn.E_INVALID, kn.OK]


def test_mixed_batch_in_one_chunk_and_in_chunks_of_three(kn, synth, oracle, cases, capfd, monkeypatch):
    monkeypatch.setenv(TRACE, "1")
    train, k, queries, others, items, statuses = _mixed(kn, synth, cases)
    answers = {}
    for chunk in (64, 3):
        e = kn.Engine(k=k, workspace_bytes=_workspace_for(chunk, 60, 80))
        e.fit(*train)
        by = _By(kn.BystanderQueries(e))
        capfd.readouterr()
        nb, st = by.neighbors_revised_batch(queries, others, cap=61)
        chunks, revise = _trace(capfd)
        pr, st2 = by.predict_revised_batch(queries, others, items)
        assert st.tolist() == statuses and st2.tolist() == statuses
        assert "query 4: a removed item that the user did not rate in train" in e._lib.knncf_last_error(e._h).decode()
        if chunk == 64:
            # slots: 1 + 8, 1 + 7, 1 + 7, 1 + 7, 1 + 8 (the bad removal shows on the device), 1 + 7 distinct: the whole-chunk kernel
            assert chunks == [(50, 5, 8)] and revise == [(4, 3 + 2 + 1 + 2, 0)], (chunks, revise)
        else:
            # a query continues in the next chunk, where its revise row is prepared again: every chunk of a changer with removals
            assert all(s <= 3 for s, _, _ in chunks) and len(chunks) >= 18 and len(revise) >= 12, (chunks, revise)
            assert all(s == 1 for s, _, _ in revise)
        answers[chunk] = (nb, pr)
        e.close()
    (nb, pr), (nb3, pr3) = answers[64], answers[3]
    for b, q in enumerate(queries):
        if statuses[b] != kn.OK:  # untouched rows, counts 0
            assert all(len(ids) == 0 for ids, _ in nb[b] + nb3[b]) and np.isnan(pr[b]).all() and np.isnan(pr3[b]).all()
            continue
        assert _bits(pr[b]) == _bits(pr3[b]), b
        for x, y in zip(nb[b], nb3[b]):
            _same_pair(x, y, b)
        m = oracle.Model(*rc.aug_of(train, *q))
        for j, v in enumerate(others[b]):
            _same_pair(nb[b][j], m.pipeline(oracle.SIM_COSINE, k).neighbors(v), (b, v))
            assert _bits([pr[b][j]]) == _bits([m.pipeline(oracle.SIM_COSINE, k).predict(v, items[b][j])]), (b, v)


# ---- statuses -------------------------------------------------------------------------------------------------------------------
def test_per_query_statuses(kn, cases):
    c = cases["removes-3-k5"]
    train = c.train
    e = kn.Engine(k=c.k)
    e.fit(*train)
    by = _By(kn.BystanderQueries(e))
    users = [u for u in c.others if u != bc.UNKNOWN_USER]
    known = 9
    mine = train[1][train[0] == known].astype(np.int32)
    free = uc.unrated(train, known, 3)
    none_i, none_r = np.empty(0, dtype=np.int32), np.empty(0)
    rm1 = mine[:1]
    bad = [
        ((known, rm1, free[:1], [3.0]), [users[0], known], kn.E_INVALID, "a row names the query's own user"),
        ((known, free[:1], none_i, none_r), users[3:6], kn.E_INVALID, "a removed item that the user did not rate in train"),
        ((known, mine[[2, 2]], none_i, none_r), users[3:6], kn.E_INVALID, "a removed item listed twice"),
        ((known, mine, none_i, none_r), users[3:6], kn.E_INVALID, "the removals leave the user without a row"),
        ((known, rm1, np.asarray([free[0], mine[1]], dtype=np.int32), [4.0, 3.0]), users[3:6], kn.E_DUPLICATE, "the ratings repeat an item"),
        ((known, rm1, free[:2], [-1.0e6, 2.0]), users[3:6], kn.E_UNSUPPORTED, "a negative mean rating"),
        ((7004, rm1, free[:1], [3.0]), users[3:6], kn.E_INVALID, "a removed item for a user that is not in the training set"),
    ]
    good = c.query
    single = by.neighbors_revised(*good, users[:3])
    for q, oth, status, text in bad:
        queries, others = [good, q], [users[:3], oth]
        items = [[int(train[1][0])] * len(o) for o in others]
        nb, st = by.neighbors_revised_batch(queries, others)
        assert st.tolist() == [kn.OK, status], text
        assert f"query 1: {text}" in e._lib.knncf_last_error(e._h).decode(), text
        pr, st = by.predict_revised_batch(queries, others, items)
        assert st.tolist() == [kn.OK, status], text
        for got, w in zip(nb[0], single):
            _same_pair(got, w, text)
        assert _bits(pr[0]) == _bits(by.predict_revised(*good, users[:3], items[0]))
        assert all(len(x[0]) == 0 for x in nb[1]) and np.isnan(pr[1]).all(), text
        with pytest.raises(kn.KnncfError) as ex:  # the single form returns the query's status
            by.neighbors_revised(*q, oth)
        assert ex.value.status == status and text in str(ex.value)
        # at the C boundary: counts 0, sentinels untouched
        qargs, keep = e._batch_args("revise", queries)
        roff, o32, _ = by._rows(2, others, None)
        ids = np.full((len(o32), 3), -7, dtype=np.int32)
        sims = np.full((len(o32), 3), -7.0)
        counts = np.full(len(o32), -7, dtype=np.int32)
        stc = np.zeros(2, dtype=np.int32)
        p = e._ptr
        assert e._lib.knncf_revise_bystander_neighbors_batch(e._h, *qargs, p(roff, i64p), p(o32, i32p), 3, p(ids.reshape(-1), i32p),
                                                             p(sims.reshape(-1), f64p), p(counts, i32p), p(stc, i32p)) == kn.OK
        assert (counts[:3] == c.k).all() and (ids[:3] != -7).all()
        assert (counts[3:] == 0).all() and (ids[3:] == -7).all() and (sims[3:] == -7.0).all(), text
    # the 65536-row cap counts the removed rows too
    n_over = 65_537 - len(mine)
    q = (known, rm1, np.arange(200_000, 200_000 + n_over, dtype=np.int32), np.full(n_over, 3.0))
    nb, st = by.neighbors_revised_batch([q], [users[:2]])
    assert st.tolist() == [kn.E_UNSUPPORTED]
    e.close()


def test_handle_level_refusals(kn, cases):
    c = cases["re-rates-dyadic"]
    train, q, rm, it, rt = c.train, c.q, c.removed, c.items, c.ratings
    good = [c.query, (1000, [], [4, 5], [2.0, 3.0])]
    oth, pi = [[1, 2], [3]], [[1, 2], [3]]

    def status_of(call):
        with pytest.raises(kn.KnncfError) as ex:
            call()
        return ex.value.status

    def all_four(e, status):
        by = _By(kn.BystanderQueries(e))
        assert status_of(lambda: by.neighbors_revised(q, rm, it, rt, [1, 2])) == status
        assert status_of(lambda: by.predict_revised(q, rm, it, rt, [1, 2], [1, 2])) == status
        assert status_of(lambda: by.neighbors_revised_batch(good, oth)) == status
        assert status_of(lambda: by.predict_revised_batch(good, oth, pi)) == status

    e = kn.Engine(k=5)
    all_four(e, kn.E_STATE)  # before a fit
    e.fit(*train)
    lib, h, p = e._lib, e._h, e._ptr
    o2, p2, out, st = np.asarray([1, 2], dtype=np.int32), np.asarray([1, 2], dtype=np.int32), np.empty(2), np.zeros(1, dtype=np.int32)
    it32, rm32, ids, sims, cnt = np.asarray(it, dtype=np.int32), np.asarray(rm, dtype=np.int32), np.empty(10, dtype=np.int32), np.empty(10), np.zeros(2, dtype=np.int32)
    n, nr = len(it32), len(rm32)
    predict = lambda pred, removed, n_removed, items, n_items, m: lib.knncf_revise_bystander_predict(
        h, pred, q, removed, n_removed, items, p(rt, f64p), n_items, p(o2, i32p), p(p2, i32p), m, p(out, f64p))
    assert predict(kn.PRED_BASELINE, p(rm32, i32p), nr, p(it32, i32p), n, 2) == kn.E_UNSUPPORTED  # a predictor other than the kNN one
    assert predict(kn.PRED_PERSONALIZED, p(rm32, i32p), nr, p(it32, i32p), n, 2) == kn.E_UNSUPPORTED
    assert predict(kn.PRED_KNN, p(rm32, i32p), nr, None, n, 2) == kn.E_INVALID  # null rows with n_ratings > 0
    assert predict(kn.PRED_KNN, p(rm32, i32p), nr, p(it32, i32p), -1, 2) == kn.E_INVALID
    assert predict(kn.PRED_KNN, p(rm32, i32p), nr, p(it32, i32p), n, -1) == kn.E_INVALID
    assert predict(kn.PRED_KNN, None, nr, p(it32, i32p), n, 2) == kn.E_INVALID  # null removed items with n_removed > 0
    assert predict(kn.PRED_KNN, p(rm32, i32p), -1, p(it32, i32p), n, 2) == kn.E_INVALID
    assert predict(kn.PRED_KNN, p(rm32, i32p), nr, p(it32, i32p), n, 2) == kn.OK
    assert predict(kn.PRED_KNN, p(rm32, i32p), 1, None, 0, 2) == kn.OK  # removals alone
    nbrs = lambda cap, o: lib.knncf_revise_bystander_neighbors(h, q, p(rm32, i32p), nr, p(it32, i32p), p(rt, f64p), n, o, 2, cap, p(ids, i32p),
                                                               p(sims, f64p), p(cnt, i32p))
    assert nbrs(-1, p(o2, i32p)) == kn.E_INVALID and nbrs(5, None) == kn.E_INVALID and nbrs(5, p(o2, i32p)) == kn.OK
    us, off, roff = np.asarray([q], dtype=np.int32), np.asarray([0, n], dtype=np.int64), np.asarray([0, 2], dtype=np.int64)
    rmo = np.asarray([0, nr], dtype=np.int64)
    batch = lambda B, rmo_, off_, roff_: lib.knncf_revise_bystander_predict_batch(
        h, kn.PRED_KNN, p(us, i32p), rmo_, p(rm32, i32p), off_, p(it32, i32p), p(rt, f64p), B, roff_, p(o2, i32p), p(p2, i32p), p(out, f64p), p(st, i32p))
    i64 = lambda *x: p(np.asarray(x, dtype=np.int64), i64p)
    assert batch(-1, p(rmo, i64p), p(off, i64p), p(roff, i64p)) == kn.E_INVALID
    assert batch(1, p(rmo, i64p), None, p(roff, i64p)) == kn.E_INVALID
    assert batch(1, p(rmo, i64p), i64(1, n), p(roff, i64p)) == kn.E_INVALID  # offsets[0] != 0
    assert batch(1, p(rmo, i64p), p(off, i64p), i64(0, -1)) == kn.E_INVALID  # row_offsets decrease
    assert batch(1, None, p(off, i64p), p(roff, i64p)) == kn.E_INVALID       # bad removed CSR offsets: null,
    assert batch(1, i64(1, nr), p(off, i64p), p(roff, i64p)) == kn.E_INVALID  # not starting at 0,
    assert batch(1, i64(0, -1), p(off, i64p), p(roff, i64p)) == kn.E_INVALID  # decreasing
    assert "removed_offsets decrease" in lib.knncf_last_error(h).decode()
    assert batch(0, None, None, None) == kn.OK and batch(1, p(rmo, i64p), p(off, i64p), p(roff, i64p)) == kn.OK
    e.close()
    e1 = kn.Engine(k=5, similarity=kn.SIM_ONE)
    e1.fit(*train)
    all_four(e1, kn.E_UNSUPPORTED)
    e1.close()
    es = kn.Engine(k=5, shard_rank=0, shard_count=2)  # a shard handle
    es.fit(*train)
    all_four(es, kn.E_UNSUPPORTED)
    es.close()
    keep = np.isin(train[0], np.unique(train[0])[:4])
    e4 = kn.Engine(k=5)
    e4.fit(*(a[keep] for a in train))
    all_four(e4, kn.E_UNSUPPORTED)  # fewer than 5 train users
    e4.close()


@pytest.mark.parametrize("name", ["re-rates-dyadic", "off-scale"])
def test_handle_state(kn, synth, cases, tmp_path, name):
    """the checkpoint bytes, a neighbors answer and an mae are the same before and after the calls (off-scale: with the file folded
    again for average(aug))"""
    c = cases[name]
    t = synth.syn_scaled(60, 80, 1500, 3).test
    users = np.asarray([u for u in c.others if u != bc.UNKNOWN_USER], dtype=np.int32)
    e = kn.Engine(k=c.k)
    e.fit(*c.train)
    e.neighbors_batch(users[[3, 17, 40]])
    before, after = str(tmp_path / "before.bin"), str(tmp_path / "after.bin")
    nb0 = e.neighbors(int(users[3]))
    e.neighbors_save(before)
    by = _By(kn.BystanderQueries(e))
    by.neighbors_revised(*c.query, c.others)
    by.predict_revised(*c.query, np.asarray(c.others, dtype=np.int32), np.full(len(c.others), int(c.train[1][0]), dtype=np.int32))
    e.neighbors_save(after)
    assert open(before, "rb").read() == open(after, "rb").read()
    _same_pair(e.neighbors(int(users[3])), nb0, name)
    mae = e.mae(kn.PRED_KNN, t.users, t.items, t.ratings)
    e.close()
    fresh = kn.Engine(k=c.k)
    fresh.fit(*c.train)
    fresh.neighbors_batch(users[[3, 17, 40]])
    assert _bits([mae]) == _bits([fresh.mae(kn.PRED_KNN, t.users, t.items, t.ratings)])
    fresh.close()


# ---- a file longer than one chunk of the sequential fold ------------------------------------------------------------------------
def test_mid_size_shuffled_file_folds_average_across_chunks(kn, oracle, syn100k, capfd, monkeypatch):
    """syn-100k in shuffled file order with ratings that are not dyadic: 80 000 train ratings, so the fold of the surviving
    ratings runs over many 2048-rating pieces of the file and the removed rows — a changer's first, middle and last file row, and
    one re-rated — stand in different ones.  Three changers, 8 fitted bystanders each (4 from the changer's list, 4 not) and a
    user unknown to aug, whose answer is average(aug)"""
    from tests.revise_cases import aug_of, syn100k as shuffled_file

    monkeypatch.setenv(TRACE, "1")
    train = shuffled_file(syn100k, shuffled=True)
    assert not rc.is_dyadic(train) and len(train[2]) > 20 * 2048
    rng = np.random.default_rng(17)
    u, cnt = np.unique(train[0], return_counts=True)
    k = 30
    e = kn.Engine(k=k)
    e.fit(*train)
    by = _By(kn.BystanderQueries(e))
    train_items = np.unique(train[1])
    for c in [int(x) for x in rng.choice(u[cnt > 12], 3, replace=False)]:
        at = np.flatnonzero(train[0] == c)
        gone = at[[0, len(at) // 2, -1, 1]]
        removed = train[1][gone].astype(np.int32)
        items = np.asarray([removed[3], rng.choice(np.setdiff1d(train_items, train[1][at]))], dtype=np.int32)
        ratings = np.asarray([float(np.round(5.9 - train[2][gone[3]], 2)), 3.37])
        near = [int(x) for x in e.neighbors_with(c, [], [])[0][:4]]
        far = [int(x) for x in rng.choice(np.setdiff1d(u, near + [c]), 4, replace=False)]
        others = near + far + [bc.UNKNOWN_USER]
        pis = np.concatenate([removed, items[1:], rng.choice(train_items, 3, replace=False)]).astype(np.int32)
        m = oracle.Model(*aug_of(train, c, removed, items, ratings))
        capfd.readouterr()
        nb = by.neighbors_revised(c, removed, items, ratings, others, cap=k)
        pr = by.predict_revised(c, removed, items, ratings, np.repeat(np.asarray(others, dtype=np.int32), len(pis)),
                                np.tile(pis, len(others))).reshape(len(others), -1)
        _, revise = _trace(capfd)
        assert revise == [(1, 4, 0), (1, 4, 1)], revise
        for j, v in enumerate(others):
            p = m.pipeline(oracle.SIM_COSINE, k)  # (every evaluation of this pipeline is v's)
            _same_pair(nb[j], p.neighbors(v), (c, v))
            assert _bits(pr[j]) == _bits([p.predict(v, int(i)) for i in pis]), (c, v)
        assert _bits(pr[-1]) == _bits([m.average()] * len(pis)), c
    e.close()
