"""knncf_query_explain_personalized* / knncf_update_explain_personalized* / knncf_revise_explain_personalized*: the terms behind the
Personalized predictions of fold-in, update and revise queries, bit for bit.

The expected rows come from tests/personalized_query_explain_cases.py: PersonalTermModel on the oracle's aug, which asks the
oracle only for raw similarities with the query user first and for the deviations (test_personalized_query_explain_premises.py
shows on the CPU that its fold and combine ARE the oracle's prediction on aug, and that every input has the feature its test
here relies on).  Every comparison is == on int32 ids and on fp64 bit patterns.  Raw calls through the C ABI with
sentinel-filled outputs prove which cells a call writes; KNNCF_DEBUG_TRACE_DISPATCH lines show the launches.

Figures: none — every check is exact equality."""
import ctypes as C
import importlib
import re

import numpy as np
import pytest

from tests import personalized_explain_model as pm
from tests import personalized_query_cases as pc
from tests import personalized_query_explain_cases as xc
from tests.personalized_explain_model import BY_WEIGHT, SUM_ORDER
from tests.query_helpers import _chunk, _workspace_for
from tests.test_gpu_personalized_explain import _assert_rows, _bits, _free_device_bytes, _same
from tests.test_gpu_recommend_batch import _table

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"
SENT_I, SENT_F = -7, 7.5
i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _sims(kn, oracle, name):
    return {"cosine": (kn.SIM_COSINE, oracle.SIM_COSINE), "jaccard": (kn.SIM_JACCARD, oracle.SIM_JACCARD)}[name]


def _ptr(a, t):
    return None if a.size == 0 else a.ctypes.data_as(t)


def _outputs(m, cap, null_terms=False, null_sums=False, null_counts=False):
    """sentinel-filled outputs of m rows and their C arguments"""
    w = max(cap, 0)
    raters = np.full((m, w), SENT_I, dtype=np.int32)
    sims, devs = np.full((m, w), SENT_F), np.full((m, w), SENT_F)
    counts = np.full(m, SENT_I, dtype=np.int32)
    sums, preds = np.full((m, 2), SENT_F), np.full(m, SENT_F)
    terms = (None, None, None) if null_terms else (_ptr(raters, i32p), _ptr(sims, f64p), _ptr(devs, f64p))
    args = (*terms, None if null_counts else _ptr(counts, i32p), None if null_sums else _ptr(sums, f64p), None if null_sums else _ptr(preds, f64p))
    return (raters, sims, devs, counts, sums, preds), args


def _raw(e, fam, query, items, cap, order=SUM_ORDER, **nulls):
    """knncf_<fam>_explain_personalized through the C ABI on sentinel-filled outputs: (status, raters, sims, devs, counts, sums,
    preds)"""
    q, removed, its, rts = query
    rm = np.ascontiguousarray(removed, dtype=np.int32)
    its, rts = np.ascontiguousarray(its, dtype=np.int32), np.ascontiguousarray(rts, dtype=np.float64)
    pi = np.ascontiguousarray(items, dtype=np.int32)
    out, args = _outputs(len(pi), cap, **nulls)
    lead = (int(q), _ptr(rm, i32p), len(rm)) if fam == "revise" else (int(q),)
    st = getattr(e._lib, f"knncf_{fam}_explain_personalized")(e._h, *lead, _ptr(its, i32p), _ptr(rts, f64p), len(its), _ptr(pi, i32p), len(pi),
                                                               order, cap, *args)
    return (st, *out)


def _raw_batch(e, queries, pred_items, cap, order=SUM_ORDER, **nulls):
    """knncf_revise_explain_personalized_batch through the C ABI on sentinel-filled outputs: (status, raters, sims, devs, counts,
    sums, preds, statuses, row offsets)"""
    qargs, keep = e._batch_args("revise", queries)
    poff = np.zeros(len(queries) + 1, dtype=np.int64)
    poff[1:] = np.cumsum([len(x) for x in pred_items])
    pi = np.ascontiguousarray(np.concatenate(pred_items), dtype=np.int32)
    out, args = _outputs(len(pi), cap, **nulls)
    statuses = np.full(len(queries), SENT_I, dtype=np.int32)
    st = e._lib.knncf_revise_explain_personalized_batch(e._h, *qargs, _ptr(poff, i64p), _ptr(pi, i32p), order, cap, *args, _ptr(statuses, i32p))
    return (st, *out, statuses, poff)


def _predict(e, kn, fam, query, items):
    q, removed, its, rts = query
    P = kn.PRED_PERSONALIZED
    if fam == "query":
        return e.predict_for(q, its, rts, items, predictor=P)
    if fam == "update":
        return e.predict_with(q, its, rts, items, predictor=P)
    return e.predict_revised(q, removed, its, rts, items, predictor=P)


def _explain(e, kn, fam, query, items, cap, order):
    q, removed, its, rts = query
    kw = dict(order=order, predictor=kn.PRED_PERSONALIZED)
    if fam == "query":
        return e.explain_for(q, its, rts, items, cap, **kw)
    if fam == "update":
        return e.explain_with(q, its, rts, items, cap, **kw)
    return e.explain_revised(q, removed, its, rts, items, cap, **kw)


def _launches(capfd):
    """the dispatch lines since the last look: ([(order, cap, rows)] of qb_explain_all, [stride] of qb_fold_all)"""
    err = capfd.readouterr().err
    found = re.findall(r"^knncf-dispatch qb_explain_all order=(\d+) cap=(\d+) rows=(\d+)$", err, flags=re.M)
    return [tuple(int(x) for x in f) for f in found], [int(x) for x in re.findall(r"^knncf-dispatch qb_fold_all stride=(\d+)$", err, flags=re.M)]


# ---- 1. the edge set: every query, both orders, a range of caps, against the model and against the predict calls ---------------
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_edge_set_against_the_model(kn, oracle, sim_name):
    ksim, osim = _sims(kn, oracle, sim_name)
    train, queries, items = xc.edge_cases()
    e = kn.Engine(k=10, similarity=ksim).fit(*train)
    for name, query in queries.items():
        fam = xc.family(train, query)
        want = xc.want_rows(oracle, "edge", train, query, osim, items[name])
        mean = xc.term_model(oracle, "edge", train, query, osim).model.users_avg(query[0])
        yardstick = _predict(e, kn, fam, query, items[name])
        for order in (SUM_ORDER, BY_WEIGHT):
            for cap in pm.caps_of(max(r.count for r in want)):
                st, *got = _raw(e, fam, query, items[name], cap, order, null_terms=cap == 0)
                assert st == kn.OK, (name, order, cap)
                _assert_rows(got, want, order, (sim_name, name, order, cap), pad=(SENT_I, SENT_F))
                raters, sims, devs, counts, sums, preds = got
                assert np.array_equal(_bits(preds), _bits(yardstick)), (name, order, cap)
                for j in np.flatnonzero(counts <= cap):  # the caller's left fold and combine
                    m = counts[j]
                    if order == SUM_ORDER:
                        assert np.array_equal(_bits(pm.fold(sims[j, :m], devs[j, :m])), _bits(sums[j])), (name, cap, j)
                    assert _bits(pm.combine(oracle, mean, *sums[j].tolist())) == _bits(preds[j]), (name, cap, j)
        st, *_, counts, sums, preds = _raw(e, fam, query, items[name], 3, BY_WEIGHT, null_sums=True)  # sums and predictions may be null
        assert st == kn.OK and counts.tolist() == [r.count for r in want] and (sums == SENT_F).all() and (preds == SENT_F).all()
    e.close()


# ---- 2. segment-length edges: 64 positions per load of the walk, 256 per load group of the select and emit passes, 64 / 256 staged
# terms in the rank, and the appended own term on a load boundary (n = 64, 256) ---------------------------------------------------
@pytest.mark.parametrize("n", xc.DENSE_SIZES)
def test_segment_length_edges(kn, oracle, n):
    train, queries, items = xc.dense_cases(n)
    e = kn.Engine(k=10).fit(*train)
    for name, query in queries:
        fam = xc.family(train, query)
        want = xc.want_rows(oracle, f"dense{n}", train, query, oracle.SIM_COSINE, items)
        count = want[0].count
        assert count == (n + 1 if name == "fold_in" else n)
        for order, cap in ((BY_WEIGHT, 16), (BY_WEIGHT, count), (BY_WEIGHT, count - 1), (SUM_ORDER, count)):
            _assert_rows(_explain(e, kn, fam, query, items, cap, order), want, order, (n, name, order, cap))
    e.close()


# ---- 3. ties: a cap that ends inside a group of equal magnitudes keeps the earliest in summation order -------------------------
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_caps_inside_tie_groups_keep_the_earliest(kn, oracle, sim_name):
    ksim, osim = _sims(kn, oracle, sim_name)
    train, queries, items = xc.clone_cases()
    e = kn.Engine(k=10, similarity=ksim).fit(*train)
    for name, query in queries:
        fam = xc.family(train, query)
        want = xc.want_rows(oracle, "clones", train, query, osim, items)
        cuts = xc.tie_cuts(want)
        caps = sorted(cuts, key=lambda c: -len(cuts[c]))[:4]
        assert caps
        full = _explain(e, kn, fam, query, items, max(r.count for r in want), SUM_ORDER)
        _assert_rows(full, want, SUM_ORDER, (sim_name, name))
        for cap in caps:
            got = _explain(e, kn, fam, query, items, cap, BY_WEIGHT)
            _assert_rows(got, want, BY_WEIGHT, (sim_name, name, cap))
            for j in cuts[cap]:
                t = abs(got[1][j, cap - 1])  # the magnitude the cap cuts through
                place = {r: q for q, r in enumerate(full[0][j, :full[3][j]].tolist())}  # (a rater occurs once per item)
                tied = [q for q in range(full[3][j]) if abs(full[1][j, q]) == t]
                kept = [place[int(r)] for r, s in zip(got[0][j], got[1][j]) if abs(s) == t]
                assert kept == tied[:len(kept)] and len(kept) < len(tied), (name, cap, j)
    e.close()


# ---- 4. a mixed batch equals its single calls at every chunk size and sub-range ------------------------------------------------
def _mixed_batch(train, queries, items):
    """(names, revise-batch queries, requested items, expected statuses by name): every edge query, the three families mixed,
    EDGE_MIDDLE twice in a row, more fold-in users to pass 40, and three failing queries"""
    names, qs, pis = [], [], []

    def add(name, query, pi):
        names.append(name)
        qs.append((int(query[0]), query[1], query[2], query[3]))
        pis.append(np.asarray(pi, dtype=np.int32))

    for name, query in queries.items():
        add(name, query, items[name])
        if name == "update_middle":
            add("update_middle_again", query, items[name])
    every = np.unique(train[1]).astype(np.int32)
    for x in range(16):  # fold-in users 950..965 with 2..7 rows
        its = np.roll(np.append(every, pc.NEW_ITEM), x)[:2 + x % 6].astype(np.int32)
        rts = np.round(0.7 + 0.37 * ((np.arange(len(its)) * (x + 3)) % 11), 2)
        add(f"extra_{x}", (950 + x, pc.NONE_I, its, rts), pc.pred_items(train, 950 + x, pc.NONE_I, its))
    add("bad_duplicate", (970, pc.NONE_I, np.array([12, 13, 12], dtype=np.int32), np.array([1.0, 2.0, 3.0])), every)
    add("bad_removal", (pc.EDGE_FIRST, np.array([pc.EDGE_NEVER], dtype=np.int32), pc.NONE_I, pc.NONE_R), every)
    add("bad_empty", (971, pc.NONE_I, pc.NONE_I, pc.NONE_R), every)
    order = np.random.default_rng(5).permutation(len(names)).tolist()  # (the failing ones land among the others)
    return [names[j] for j in order], [qs[j] for j in order], [pis[j] for j in order]


def test_batch_equals_singles_in_every_chunking(kn, oracle, monkeypatch, capfd):
    train, queries, items = xc.edge_cases()
    names, qs, pis = _mixed_batch(train, queries, items)
    B, cap = len(qs), 130
    assert B >= 40
    U, I = len(np.unique(train[0])), len(np.unique(train[1]))
    bad = {"bad_duplicate": kn.E_DUPLICATE, "bad_removal": kn.E_INVALID, "bad_empty": kn.E_INVALID}
    want_status = [bad.get(n, kn.OK) for n in names]
    monkeypatch.setenv(TRACE, "1")
    runs, strides_seen = {}, set()
    for chunk in (64, 7, 1):
        workspace = _workspace_for(chunk, U, I)
        e = kn.Engine(k=10, workspace_bytes=workspace).fit(*train)
        assert _chunk(e, workspace) == chunk
        R = max(1, (workspace // 2) // (40 * cap + 28))
        for order in (BY_WEIGHT, SUM_ORDER) if chunk == 64 else (BY_WEIGHT,):
            capfd.readouterr()
            st, *out, statuses, poff = _raw_batch(e, qs, pis, cap, order)
            lines, strides = _launches(capfd)
            assert st == kn.OK and statuses.tolist() == want_status, chunk
            assert all(ln[:2] == (order, cap) and 1 <= ln[2] <= R for ln in lines)
            good_rows = sum(len(pis[b]) for b in range(B) if want_status[b] == kn.OK)
            assert sum(ln[2] for ln in lines) == good_rows
            if chunk == 7:  # R = 12 rows: several sub-ranges per chunk
                assert R == 12 and len(lines) >= 3 * len(strides)
            strides_seen.update(strides)
            runs[chunk, order] = out
        if chunk == 64:
            # the single calls of each query's own family, on the same handle
            for order in (BY_WEIGHT, SUM_ORDER):
                raters, sims, devs, counts, sums, preds = runs[64, order]
                for b in range(B):
                    rows = slice(int(poff[b]), int(poff[b + 1]))
                    got = tuple(a[rows] for a in (raters, sims, devs, counts, sums, preds))
                    query = (qs[b][0], qs[b][1], qs[b][2], qs[b][3])
                    fam = xc.family(train, query)
                    st, *single = _raw(e, fam, query, pis[b], cap, order)
                    assert st == want_status[b], names[b]
                    if want_status[b] != kn.OK:  # counts 0, nothing else written (a single form may refuse before it sets counts)
                        assert (got[3] == 0).all() and all((x == (SENT_I if x.dtype == np.int32 else SENT_F)).all() for x in got[:3] + got[4:])
                        continue
                    assert _same(got, single), (names[b], order)
                    if names[b] in queries and order == BY_WEIGHT:
                        _assert_rows(got, xc.want_rows(oracle, "edge", train, queries[names[b]], oracle.SIM_COSINE, pis[b]), order, names[b],
                                     pad=(SENT_I, SENT_F))
            # a truncating cap through the batch
            st, *cut, statuses, _ = _raw_batch(e, qs, pis, 16, BY_WEIGHT)
            assert st == kn.OK and statuses.tolist() == want_status
            assert np.array_equal(cut[3], runs[64, BY_WEIGHT][3]) and np.array_equal(_bits(cut[4]), _bits(runs[64, BY_WEIGHT][4]))
            full = runs[64, BY_WEIGHT]
            for j in np.flatnonzero(full[3] > 0):
                m = min(int(full[3][j]), 16)
                assert cut[0][j, :m].tolist() == full[0][j, :m].tolist() and np.array_equal(_bits(cut[1][j, :m]), _bits(full[1][j, :m]))
                assert (cut[0][j, m:] == SENT_I).all()
        e.close()
    monkeypatch.delenv(TRACE)
    assert _same(runs[64, BY_WEIGHT], runs[7, BY_WEIGHT]) and _same(runs[64, BY_WEIGHT], runs[1, BY_WEIGHT])
    # both similarity kernels: a chunk of more than 32 answerable queries (stride 64), and chunks of at most 7 / of one
    assert 64 in strides_seen and 8 in strides_seen and 1 in strides_seen


# ---- 5. just past 2048 users ---------------------------------------------------------------------------------------------------
def test_wide_set(kn, oracle):
    train, queries, items = xc.wide_cases()
    e = kn.Engine(k=10).fit(*train)
    for name, query in queries:
        fam = xc.family(train, query)
        want = xc.want_rows(oracle, "wide", train, query, oracle.SIM_COSINE, items[name])
        _assert_rows(_explain(e, kn, fam, query, items[name], 16, BY_WEIGHT), want, BY_WEIGHT, name)
        _assert_rows(_explain(e, kn, fam, query, items[name], max(r.count for r in want), SUM_ORDER), want, SUM_ORDER, name)
    e.close()


# ---- 6. read-only on the handle, timings, allocations, k ---------------------------------------------------------------------
def test_state_timings_allocations_and_k(kn, tmp_path):
    train, queries, items = xc.edge_cases()
    names = list(queries)
    qs = [(int(queries[n][0]), *queries[n][1:]) for n in names]
    pis = [items[n] for n in names]
    e = kn.Engine(k=10).fit(*train)
    lists = e.neighbors_batch(np.unique(train[0])[:5])
    before = _table(e, tmp_path / "before.nb")
    e.reset_timings()
    first = e.explain_revised_batch(qs, pis, 16, order=BY_WEIGHT, predictor=kn.PRED_PERSONALIZED)
    t = e.timings()
    assert t["prep_ms"] > 0 and t["predict_ms"] > 0  # the file-order rater copies; the fold and the explain kernel
    e.reset_timings()
    free = _free_device_bytes()
    again = e.explain_revised_batch(qs, pis, 16, order=BY_WEIGHT, predictor=kn.PRED_PERSONALIZED)
    assert _free_device_bytes() >= free  # a repeated call of the same shape allocates no device memory
    t = e.timings()
    assert t["predict_ms"] > 0 and t["prep_ms"] == 0 and t["rerank_ms"] == 0
    assert all(t[name] == 0 for name in ("densify_ms", "gemm_ms", "tail_ms", "select_ms", "gemm_launches", "select_launches"))
    assert first[1].tolist() == again[1].tolist() and all(_same(a, b) for a, b in zip(first[0], again[0]))
    assert _table(e, tmp_path / "after.nb") == before
    assert open(tmp_path / "after.nb", "rb").read() == open(tmp_path / "before.nb", "rb").read()
    assert _same(lists, e.neighbors_batch(np.unique(train[0])[:5]))
    e.close()
    other = kn.Engine(k=3).fit(*train)  # the handle's k plays no part
    third = other.explain_revised_batch(qs, pis, 16, order=BY_WEIGHT, predictor=kn.PRED_PERSONALIZED)
    assert all(_same(a, b) for a, b in zip(first[0], third[0]))
    other.close()


# ---- 7. refusals write nothing -------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(kn):
    train, queries, items = xc.edge_cases()
    query, pi = queries["update_middle"], items["update_middle"]
    batch = ([(int(query[0]), *query[1:])], [pi])

    def untouched(res, n_out=6):
        return all((x == (SENT_I if x.dtype == np.int32 else SENT_F)).all() for x in res[1:1 + n_out])

    def refused(e, status, cap=4, order=SUM_ORDER, **nulls):
        for fam in ("query", "update", "revise"):
            res = _raw(e, fam, query, pi, cap, order, **nulls)
            assert res[0] == status and untouched(res), fam
        res = _raw_batch(e, *batch, cap, order, **nulls)
        assert res[0] == status and untouched(res, 7)  # (the statuses too)

    fresh = kn.Engine(k=10)
    refused(fresh, kn.E_STATE)
    fresh.close()
    one = kn.Engine(k=10, similarity=kn.SIM_ONE).fit(*train)
    refused(one, kn.E_UNSUPPORTED)
    one.close()
    shard = kn.Engine(k=10, shard_rank=0, shard_count=2).fit(*train)
    refused(shard, kn.E_UNSUPPORTED)
    shard.close()
    four = train[0] <= 4
    few = kn.Engine(k=10).fit(train[0][four], train[1][four], train[2][four])
    assert few.num_users == 4
    refused(few, kn.E_UNSUPPORTED)
    few.close()
    e = kn.Engine(k=10).fit(*train)
    refused(e, kn.E_INVALID, cap=-1)
    refused(e, kn.E_INVALID, order=7)
    refused(e, kn.E_INVALID, null_counts=True)
    refused(e, kn.E_INVALID, null_terms=True)  # cap > 0 needs the term arrays
    # the kNN explain calls keep refusing the Personalized predictor
    with pytest.raises(kn.KnncfError) as err:
        e._check(e._lib.knncf_update_explain(e._h, kn.PRED_PERSONALIZED, int(query[0]), None, None, 0, _ptr(pi, i32p), len(pi), 0, 0,
                                             None, None, None, _ptr(np.zeros(len(pi), dtype=np.int32), i32p), None, None))
    assert err.value.status == kn.E_UNSUPPORTED
    st, *got = _raw(e, "update", query, pi, 4)  # and the handle answers afterwards
    assert st == kn.OK and (got[3] >= 0).all()
    e.close()
