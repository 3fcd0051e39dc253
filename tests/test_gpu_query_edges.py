"""The query path (csrc/foldin.hip, csrc/qb_helpers.h, csrc/bystander.hip) at the sizes its kernels are built around, bit for
bit against the oracle on aug = train ++ the query rows, a fresh pipeline per query whose first evaluation is the query user's
neighbourhood (as tests/test_gpu_fold_in.py does on syn-100k).  The fits and queries are those of tests/query_edges.py;
tests/test_query_edge_premises.py proves on the CPU that each of them sits on the edge it is named for:
  A  block_exclusive_scan over take = min(k, U) with 1, 2 and 3 elements per thread (k_qb_offsets, k_by_offsets, qb_rater),
  B  the same scan over the bitmap words W = 1023 .. 4098 (k_qb_rank), every bit_rank behind it, the 32-bit half words of
     k_qb_transpose / k_query_sim_dual, and k_query_sim without LDS,
  C  train rows and rater lists of 63 | 64 | 65 (127 | 128 | 129) entries, full ballots, single matches at row positions 63,
     64 and last, the given-order fold of a query of four rows, FA_AHEAD groups of k_qb_fold_all,
  D  query row counts around k_qb_prep's 1 024-thread stride, the 65 536-row cap and a duplicate pair across the stride."""
import importlib

import numpy as np
import pytest

from tests import bystander_cases as bc
from tests import explain_model
from tests import query_edges as qe
from tests import query_explain_cases as qc
from tests.explain_model import BY_WEIGHT, SUM_ORDER
from tests.query_helpers import _aug, _bits, _chunk, _same_pair, _workspace_for

pytestmark = pytest.mark.gpu

EXPLAIN_NAMES = ("raters", "sims", "devs", "counts", "sums", "predictions")


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _sims(kn, oracle, name):
    return {"cosine": (oracle.SIM_COSINE, kn.SIM_COSINE), "jaccard": (oracle.SIM_JACCARD, kn.SIM_JACCARD)}[name]


def _n_users(train):
    return len(np.unique(train[0]))


class _Want:
    """the oracle's answers for one query on its aug: the neighbour list first, then whatever is asked"""

    def __init__(self, oracle, train, query, sim, k):
        q, items, ratings = query
        self.q = q
        self.model = oracle.Model(*_aug(train, q, items, ratings))
        self.p = self.model.pipeline(sim, k)
        self.neighbors = self.p.neighbors(q)  # first evaluation: the query user's
        self._all = None
        self.sim = sim

    def predict(self, pred_items):
        return [self.p.predict(self.q, int(i)) for i in pred_items]

    def recommend(self, n):
        return self.p.recommend(self.q, n)

    def personalized(self, pred_items):
        """predictor(aug, weightedSumDeviation(aug, S)): a fresh pipeline without a k"""
        if self._all is None:
            self._all = self.model.pipeline(self.sim, -1)
        return [self._all.predict(self.q, int(i)) for i in pred_items]


def _check_fold_in(e, want, query, pred_items, n, expect_count):
    q, items, ratings = query
    assert len(want.neighbors[0]) == expect_count, q
    _same_pair(e.neighbors_for(q, items, ratings), want.neighbors, ("neighbours", q))
    assert _bits(e.predict_for(q, items, ratings, pred_items)) == _bits(want.predict(pred_items)), ("predictions", q)
    _same_pair(e.recommend_for(q, items, ratings, n), want.recommend(n), ("recommendations", q))


def _check_update(e, want, query, pred_items, n, expect_count):
    q, items, ratings = query
    assert len(want.neighbors[0]) == expect_count, q
    _same_pair(e.neighbors_with(q, items, ratings), want.neighbors, ("neighbours", q))
    assert _bits(e.predict_with(q, items, ratings, pred_items)) == _bits(want.predict(pred_items)), ("predictions", q)
    _same_pair(e.recommend_with(q, items, ratings, n), want.recommend(n), ("recommendations", q))


def _batch(kn, e, queries, pred_items, n, personalized=False):
    """(neighbours, kNN predictions, recommendations[, Personalized predictions]) of one batched call each, every status OK"""
    out = []
    calls = [lambda: e.neighbors_for_batch(queries), lambda: e.predict_for_batch(queries, [pred_items] * len(queries)),
             lambda: e.recommend_for_batch(queries, n)]
    if personalized:
        calls.append(lambda: e.predict_for_batch(queries, [pred_items] * len(queries), predictor=kn.PRED_PERSONALIZED))
    for call in calls:
        rows, st = call()
        assert st.tolist() == [kn.OK] * len(queries)
        out.append(rows)
    return out


def _check_batch(kn, e, oracle, train, queries, oracle_slots, sim, k, pred_items, n, personalized=False):
    """the slots of oracle_slots against the oracle, every other slot against the single calls of the same handle"""
    got = _batch(kn, e, queries, pred_items, n, personalized)
    singles = {}
    for b, (q, items, ratings) in enumerate(queries):
        if b in oracle_slots:
            want = _Want(oracle, train, queries[b], sim, k)
            _same_pair(got[0][b], want.neighbors, ("neighbours", b))
            assert _bits(got[1][b]) == _bits(want.predict(pred_items)), ("predictions", b)
            _same_pair(got[2][b], want.recommend(n), ("recommendations", b))
            if personalized:
                assert _bits(got[3][b]) == _bits(want.personalized(pred_items)), ("personalized", b)
            continue
        key = (q, items.tobytes(), ratings.tobytes())
        if key not in singles:
            singles[key] = (e.neighbors_for(q, items, ratings), e.predict_for(q, items, ratings, pred_items), e.recommend_for(q, items, ratings, n),
                            e.predict_for(q, items, ratings, pred_items, predictor=kn.PRED_PERSONALIZED) if personalized else None)
        one = singles[key]
        _same_pair(got[0][b], one[0], ("neighbours", b))
        assert _bits(got[1][b]) == _bits(one[1]), ("predictions", b)
        _same_pair(got[2][b], one[2], ("recommendations", b))
        if personalized:
            assert _bits(got[3][b]) == _bits(one[3]), ("personalized", b)


# ---- A. the scan over take ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan(kn, synth):
    train = qe.scan_train(synth)
    e = kn.Engine(k=qe.SCAN_KS[0])
    e.fit(*train)
    assert e.num_users == qe.SCAN_USERS and e.num_items == qe.SCAN_ITEMS
    yield e, train
    e.close()


@pytest.mark.parametrize("k", qe.SCAN_KS)
def test_scan_fold_in(scan, oracle, k):
    e, train = scan
    e.set_k(k)
    query = qe.scan_query(train)
    _check_fold_in(e, _Want(oracle, train, query, oracle.SIM_COSINE, k), query, qe.scan_pred_items(train), 5, min(k, qe.SCAN_USERS))


def _view(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("k", qe.SCAN_EXPLAIN_KS)
def test_scan_explain(scan, oracle, k):
    """qb_rater searches off for the neighbour of a gathered entry"""
    e, train = scan
    e.set_k(k)
    q, items, ratings = qe.scan_query(train)
    tm = explain_model.TermModel(oracle, oracle.Model(*_aug(train, q, items, ratings)), oracle.SIM_COSINE, k)
    tm._neighbors(q)  # first evaluation: the query user's
    pred_items = qe.scan_explain_items(train)
    rows = [tm.row(q, int(i)) for i in pred_items]
    assert max(r.count for r in rows) > 64
    predicted = e.predict_for(q, items, ratings, pred_items)
    for cap in (16, 512):
        for order in (SUM_ORDER, BY_WEIGHT):
            got = e.explain_for(q, items, ratings, pred_items, cap, order=order)
            for name, g, w in zip(EXPLAIN_NAMES, got, qc.expected(rows, cap, order)):
                assert g.shape == w.shape and np.array_equal(_view(g), _view(w)), (k, cap, order, name)
            assert np.array_equal(_view(got[5]), _view(predicted)), (k, cap, order)


@pytest.mark.parametrize("k", qe.SCAN_UPDATE_KS)
def test_scan_update(scan, oracle, k):
    """a fitted user's slot takes min(take, U - 1) cells of a stride of take"""
    e, train = scan
    e.set_k(k)
    query = qe.scan_update(train)
    _check_update(e, _Want(oracle, train, query, oracle.SIM_COSINE, k), query, qe.scan_pred_items(train), 5, min(k, qe.SCAN_USERS - 1))


@pytest.mark.parametrize("k", qe.SCAN_BATCH_KS)
def test_scan_batch(kn, scan, oracle, k):
    """one chunk of 33 slots: 33 workgroups of the scan, each over its own part of off"""
    e, train = scan
    e.set_k(k)
    _check_batch(kn, e, oracle, train, qe.scan_batch(train), (0, qe.BATCH - 1), oracle.SIM_COSINE, k, qe.scan_pred_items(train), 5)


def test_scan_bystander(kn, scan, oracle, synth):
    """k_by_offsets: the same scan over a bystander's list, in which the newcomer is one of the neighbours"""
    e, train = scan
    k = qe.SCAN_BYSTANDER_K
    e.set_k(k)
    c = bc.near_clone(synth, k=k, q=qe.SCAN_NEWCOMER, train=train)
    users = np.unique(train[0])
    c.others = [int(c.note["clone_of"]), int(users[0]), int(users[-1])]  # (one oracle neighbour table per row)
    want_nb, want_pr = bc.expected(oracle, c, oracle.SIM_COSINE)
    by = kn.BystanderQueries(e)
    got_nb = by.neighbors_for(c.q, c.items, c.ratings, c.others, cap=k)
    pi = c.pred_items
    got_pr = by.predict_for(c.q, c.items, c.ratings, np.repeat(np.asarray(c.others, dtype=np.int32), len(pi)), np.tile(pi, len(c.others)))
    got_pr = got_pr.reshape(len(c.others), len(pi))
    assert any(c.q in nb[0].tolist() for nb in want_nb)
    for j, v in enumerate(c.others):
        assert len(want_nb[j][0]) == k
        _same_pair(got_nb[j], want_nb[j], v)
        assert _bits(got_pr[j]) == _bits(want_pr[j]), v


# ---- B. the scan over the bitmap words; D. row counts ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(kn):
    """(n_items, similarity name) -> (engine with room for a chunk of 33, train), made on first use"""
    made = {}

    def get(n_items, sim_name="cosine"):
        if (n_items, sim_name) not in made:
            train = qe.wide_fit(n_items)
            n_users = _n_users(train)
            ws = _workspace_for(qe.BATCH, n_users, n_items)
            e = kn.Engine(k=qe.K_WIDE, similarity=kn.SIM_JACCARD if sim_name == "jaccard" else kn.SIM_COSINE, workspace_bytes=ws)
            e.fit(*train)
            assert e.num_items == n_items and e.num_users == n_users and _chunk(e, ws) == qe.BATCH
            made[n_items, sim_name] = (e, train)
        return made[n_items, sim_name]

    yield get
    for e, _ in made.values():
        e.close()


def _check_words(kn, oracle, e, train, n_items, sim):
    pred_items = qe.wide_pred_items(n_items)
    for query in (qe.words_query(n_items), qe.words4_query(n_items)):
        want = _Want(oracle, train, query, sim, qe.K_WIDE)
        _check_fold_in(e, want, query, pred_items, 5, qe.K_WIDE)
        q, items, ratings = query
        got = e.predict_for(q, items, ratings, pred_items, predictor=kn.PRED_PERSONALIZED)
        assert _bits(got) == _bits(want.personalized(pred_items)), ("personalized", q)


@pytest.mark.parametrize("n_items", qe.WIDE_ITEMS)
def test_words_single(kn, wide, oracle, n_items):
    """k_qb_rank's scan with 1, 2, 3 and 5 words per thread behind k_query_sim (in LDS up to 4 096 words), k_qb_scatter,
    k_qb_pred and qb_own_term"""
    e, train = wide(n_items)
    _check_words(kn, oracle, e, train, n_items, oracle.SIM_COSINE)


@pytest.mark.parametrize("n_items", qe.WIDE_BATCH_ITEMS)
def test_words_batch(kn, wide, oracle, n_items):
    """a chunk of 33: k_qb_transpose's half words and k_query_sim_dual"""
    e, train = wide(n_items)
    _check_batch(kn, e, oracle, train, qe.wide_batch(n_items), (0, qe.BATCH - 1), oracle.SIM_COSINE, qe.K_WIDE, qe.wide_pred_items(n_items), 5,
                 personalized=True)


def test_words_jaccard(kn, wide, oracle):
    n_items = qe.WIDE_JACCARD_ITEMS
    e, train = wide(n_items, "jaccard")
    _check_words(kn, oracle, e, train, n_items, oracle.SIM_JACCARD)
    _check_batch(kn, e, oracle, train, qe.wide_batch(n_items), (0, qe.BATCH - 1), oracle.SIM_JACCARD, qe.K_WIDE, qe.wide_pred_items(n_items), 5)


def test_all_items_query(kn, wide, oracle):
    """65 536 rows, the cap: every bitmap word all ones, every stripe of every train row a full ballot; one row more is refused"""
    n_items = qe.ROWS_ITEMS
    e, train = wide(n_items)
    query = qe.all_query()
    want = _Want(oracle, train, query, oracle.SIM_COSINE, qe.K_WIDE)
    pred_items = qe.wide_pred_items(n_items)
    _check_fold_in(e, want, query, pred_items, 5, qe.K_WIDE)
    q, items, ratings = query
    got = e.predict_for(q, items, ratings, pred_items, predictor=kn.PRED_PERSONALIZED)
    assert _bits(got) == _bits(want.personalized(pred_items))
    more = (q, np.append(items, qe.NEW_ITEMS).astype(np.int32), np.append(ratings, 3.0))
    with pytest.raises(kn.KnncfError) as ex:
        e.neighbors_for(*more)
    assert ex.value.status == kn.E_UNSUPPORTED
    small = qe.words4_query(n_items)
    rows, st = e.recommend_for_batch([small, more, small], 5)
    assert st.tolist() == [kn.OK, kn.E_UNSUPPORTED, kn.OK] and len(rows[1][0]) == 0
    alone = e.recommend_for(*small, 5)
    _same_pair(rows[0], alone, 0)
    _same_pair(rows[2], alone, 2)


@pytest.mark.parametrize("n", qe.ROW_COUNTS)
def test_query_row_counts(kn, wide, oracle, n):
    """k_qb_prep's stride loop (and k_qb_self_sim's 64-per-trip fold) at these row counts, every 7th row on an unknown item"""
    e, train = wide(qe.ROWS_ITEMS)
    query = qe.count_query(n)
    q, items, ratings = query
    pred_items = qe.count_pred_items(items)
    want = _Want(oracle, train, query, oracle.SIM_COSINE, qe.K_WIDE)
    _check_fold_in(e, want, query, pred_items, 3, qe.K_WIDE)
    if n in qe.ROW_COUNTS_PERSONALIZED:
        got = e.predict_for(q, items, ratings, pred_items, predictor=kn.PRED_PERSONALIZED)
        assert _bits(got) == _bits(want.personalized(pred_items))


@pytest.mark.parametrize("position", [1023, 0])
def test_duplicate_across_the_stride(kn, wide, oracle, position):
    """the equal keys at sorted positions 1 023 | 1 024 are compared by thread 0 in its second trip"""
    e, _ = wide(qe.ROWS_ITEMS)
    dup = qe.duplicate_query(oracle, position)
    with pytest.raises(kn.KnncfError) as ex:
        e.neighbors_for(*dup)
    assert ex.value.status == kn.E_DUPLICATE
    before, after = qe.count_query(5), qe.count_query(64)
    batch = [before, dup, after]
    nb, st = e.neighbors_for_batch(batch)
    assert st.tolist() == [kn.OK, kn.E_DUPLICATE, kn.OK] and len(nb[1][0]) == 0
    rc, st = e.recommend_for_batch(batch, 3)
    assert st.tolist() == [kn.OK, kn.E_DUPLICATE, kn.OK] and len(rc[1][0]) == 0
    for b, query in ((0, before), (2, after)):
        _same_pair(nb[b], e.neighbors_for(*query), b)
        _same_pair(rc[b], e.recommend_for(*query, 3), b)


@pytest.mark.parametrize("m", [1, 2])
def test_update_of_a_1023_row_user(wide, oracle, m):
    """k_qb_seed and its sort put 1 023 train rows in front of the additional ones: 1 024 and 1 025 rows in k_qb_prep"""
    e, train = wide(qe.ROWS_ITEMS)
    query = qe.long_update(m)
    pred_items = qe.count_pred_items(np.concatenate([query[1], train[1][train[0] == qe.LONG_USER][:50]]))
    _check_update(e, _Want(oracle, train, query, oracle.SIM_COSINE, qe.K_WIDE), query, pred_items, 3, qe.K_WIDE)


# ---- C. row stripes ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows(kn):
    """similarity name -> (engine, train) on fit R"""
    made = {}
    train = qe.row_fit()[0]

    def get(sim_name):
        if sim_name not in made:
            e = kn.Engine(k=qe.ROW_K, similarity=kn.SIM_JACCARD if sim_name == "jaccard" else kn.SIM_COSINE)
            e.fit(*train)
            made[sim_name] = e
        return made[sim_name], train

    yield get
    for e in made.values():
        e.close()


def _row_pred_items(train):
    return np.concatenate([np.unique(train[1]), [qe.NEW_ITEMS]]).astype(np.int32)


@pytest.mark.parametrize("name", ["long", "small4", "small5"])
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_row_stripes_single(kn, rows, oracle, sim_name, name):
    """k = U: every planted row's similarity is in the list; k = 20: rows of 63, 64 and 65 entries go through k_qb_gather"""
    e, train = rows(sim_name)
    sim, _ = _sims(kn, oracle, sim_name)
    U = _n_users(train)
    query = qe.row_query(name)
    e.set_k(U)
    want = _Want(oracle, train, query, sim, U)
    _check_fold_in(e, want, query, _row_pred_items(train), 5, U)
    users = qe.row_fit()[1]
    listed = dict(zip(*[x.tolist() for x in e.neighbors_for(*query)]))
    assert listed[users["none"]] == 0.0
    if sim_name == "jaccard" and name == "long":
        assert listed[users["clone"]] == 1.0
    e.set_k(qe.ROW_K)
    _check_fold_in(e, _Want(oracle, train, query, sim, qe.ROW_K), query, _row_pred_items(train), 5, qe.ROW_K)
    if name != "small5":
        q, items, ratings = query
        got = e.predict_for(q, items, ratings, _row_pred_items(train), predictor=kn.PRED_PERSONALIZED)
        assert _bits(got) == _bits(want.personalized(_row_pred_items(train)))


@pytest.mark.parametrize("name", ["long", "small4", "small5"])
@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_row_stripes_batch33(kn, rows, oracle, sim_name, name):
    """k_query_sim_dual's readlane loop over the same rows; the planted query in slots 0, 1 and 32"""
    e, train = rows(sim_name)
    sim, _ = _sims(kn, oracle, sim_name)
    e.set_k(qe.ROW_K)
    queries, slots = qe.row_batch33(name)
    _check_batch(kn, e, oracle, train, queries, slots, sim, qe.ROW_K, _row_pred_items(train), 5, personalized=name != "small5")


@pytest.mark.parametrize("sim_name", ["cosine", "jaccard"])
def test_row_stripes_batch64(kn, rows, oracle, sim_name):
    """every lane live: "small4" in slot 63 beside "long" in slot 62, k = U"""
    e, train = rows(sim_name)
    sim, _ = _sims(kn, oracle, sim_name)
    U = _n_users(train)
    e.set_k(U)
    queries, slots = qe.row_batch64()
    _check_batch(kn, e, oracle, train, queries, slots, sim, U, _row_pred_items(train), 5)
