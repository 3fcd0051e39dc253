"""knncf_recommend_batch (csrc/reco_batch.hip): recommendations for many users of the fit in one call.  Everything is compared
with == on the int32 ids and on the fp64 bit patterns: against the oracle's recommend(user, n) on fresh closures evaluated in
the batch's order, and against a loop of knncf_recommend on a twin handle.  The single call IS the batch over one user, so the
loop twins pin only what differs between the two shapes of call — chunking, the order and numbering of the builds, the output
layout — and the values are pinned by the oracle comparisons alone.

Handle state.  include/knncf.h pins the state after the call to knncf_neighbors_batch over the users of the call whose mean is
not negative, and that is compared through knncf_neighbors_save: header (with the call epoch), list lengths, build numbers and every built list, byte for byte.
(Lists that were never built are not compared: their cells are whatever the allocation held.)  A LOOP of single calls numbers
its builds (call, 0), one call each, where the batch numbers them (call, position): the same order under different numbers.
So against the loop twin the lengths and the built lists are compared byte for byte, the build numbers by the ORDER they put the
users in, and a following mae bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import rating_scales as rs
from tests.test_oracle_semantics import _cols, _no_zero_scale, _random_case

pytestmark = pytest.mark.gpu

FAST_N = 32        # RB_FAST_N of csrc/engine.h: arg-min selection up to here, the segmented full order beyond


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64).tolist()


def _loop(e, predictor, users, n):
    """the single call for every user in order, in the batch's output layout"""
    items = np.full((len(users), n), -1, dtype=np.int32)
    preds = np.full((len(users), n), np.nan)
    counts = np.zeros(len(users), dtype=np.int32)
    for b, u in enumerate(users):
        i, p = e.recommend(predictor, int(u), n)
        counts[b] = len(i)
        items[b, :len(i)] = i
        preds[b, :len(i)] = p
    return items, preds, counts


def _same(a, b, what=""):
    assert a[2].tolist() == b[2].tolist(), what
    assert a[0].tolist() == b[0].tolist(), what
    assert a[1].view(np.int64).tolist() == b[1].view(np.int64).tolist(), what


def _table(e, path):
    """knncf_neighbors_save parsed: header bytes, lengths, build numbers, the built lists"""
    e.neighbors_save(str(path))
    raw = open(path, "rb").read()
    U, kcap = np.frombuffer(raw, dtype=np.int32, count=2, offset=8)
    kc = max(int(kcap), 1)
    at = 48
    cnt = np.frombuffer(raw, dtype=np.int32, count=U, offset=at); at += 4 * U
    seq = np.frombuffer(raw, dtype=np.int64, count=U, offset=at); at += 8 * U
    idx = np.frombuffer(raw, dtype=np.int32, count=U * kc, offset=at).reshape(U, kc); at += 4 * U * kc
    sim = np.frombuffer(raw, dtype=np.int64, count=U * kc, offset=at).reshape(U, kc)
    assert at + 8 * U * kc == len(raw)
    live = np.arange(kc)[None, :] < cnt[:, None]
    return {"header": raw[:48], "cnt": cnt.tolist(), "seq": seq.tolist(), "idx": np.where(live, idx, -1).tolist(),
            "sim": np.where(live, sim, 0).tolist()}


def _same_state(a, b):
    assert a == b


def _same_lists_and_order(a, b):
    assert a["cnt"] == b["cnt"] and a["idx"] == b["idx"] and a["sim"] == b["sim"]
    sa, sb = np.asarray(a["seq"]), np.asarray(b["seq"])
    assert ((sa >= 0) == (sb >= 0)).all()
    built = np.flatnonzero(sa >= 0)
    assert np.argsort(sa[built], kind="stable").tolist() == np.argsort(sb[built], kind="stable").tolist()


def _spread_users(train, count):
    u, c = np.unique(train[0], return_counts=True)
    order = np.argsort(c, kind="stable")
    return [int(u[order[j]]) for j in np.linspace(0, len(u) - 1, count).astype(int)]


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sim_name,k", [("cosine", 300), ("cosine", 10), ("jaccard", 50)])
def test_batch_against_the_oracle(kn, oracle, syn100k, sim_name, k):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    osim, esim = {"cosine": (oracle.SIM_COSINE, kn.SIM_COSINE), "jaccard": (oracle.SIM_JACCARD, kn.SIM_JACCARD)}[sim_name]
    users = _spread_users(train, 40)
    rng = np.random.default_rng(3)
    users = [users[j] for j in rng.permutation(len(users))]
    users.insert(17, 987_654)  # absent from train
    assert 987_654 not in set(train[0].tolist())
    m = oracle.Model(*train)
    for n in (3, 50):
        e = kn.Engine(k=k, similarity=esim)
        e.fit(*train)
        items, preds, counts = e.recommend_batch(kn.PRED_KNN, users, n)
        p = m.pipeline(osim, k)  # fresh closures, evaluated in the batch's order
        for b, u in enumerate(users):
            oi, op = p.recommend(u, n)
            assert counts[b] == len(oi) == n, (u, n)
            assert items[b].tolist() == oi.tolist(), (u, n)
            assert _bits(preds[b]) == _bits(op), (u, n)
        e.close()


# ---- 2. against the single call, every predictor ------------------------------------------------------------------------------
def _mixed_users(train, count, seed):
    rng = np.random.default_rng(seed)
    known = np.unique(train[0])
    users = rng.choice(known, count, replace=True).astype(np.int64)  # with repeats
    users[::29] = 900_000 + np.arange(len(users[::29]))              # ids absent from train
    users[5] = users[3]
    return users.astype(np.int32)


@pytest.mark.parametrize("sim_name,predictors", [
    ("cosine", ("GLOBAL_AVG", "USER_AVG", "ITEM_AVG", "BASELINE", "BASELINE_RDD", "KNN", "PERSONALIZED")),
    ("jaccard", ("KNN", "PERSONALIZED")),
    ("one", ("PERSONALIZED", "BASELINE")),
])
def test_batch_equals_the_single_call_on_twin_handles(kn, syn100k, tmp_path, sim_name, predictors):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    test = (d.test.users, d.test.items, d.test.ratings)
    esim = {"cosine": kn.SIM_COSINE, "jaccard": kn.SIM_JACCARD, "one": kn.SIM_ONE}[sim_name]
    for name in predictors:
        pred = getattr(kn, "PRED_" + name)
        users = _mixed_users(train, 300 if name == "KNN" else 60, seed=11)
        twins = []
        for _ in range(3):
            e = kn.Engine(k=40, similarity=esim)
            e.fit(*train)
            twins.append(e)
        a, b, c = twins
        for n in (3, 40):
            _same(a.recommend_batch(pred, users, n), _loop(b, pred, users, n), (name, n))
        if sim_name != "one":
            c.neighbors_batch(users)
            ta, tb, tc = (_table(e, tmp_path / f"{name}{j}.nb") for j, e in enumerate(twins))
            if name == "KNN":
                _same_state(ta, tc)
                _same_lists_and_order(ta, tb)
                assert any(x >= 0 for x in ta["seq"])
            else:  # the other predictors leave the neighbour table alone
                assert ta == tb and all(x < 0 for x in ta["seq"]) and all(x == 0 for x in ta["cnt"])
            ma, mb = a.mae(kn.PRED_KNN, *test), b.mae(kn.PRED_KNN, *test)
            assert _bits([ma]) == _bits([mb])
        for e in twins:
            e.close()


# ---- 3. order dependence: <= 4-rating users ----------------------------------------------------------------------------------
def _tiny_case(seed):
    rng = np.random.default_rng(4100 + seed)
    rows = _random_case(rng, n_users=14 + 5 * seed, n_items=19, n_ratings=110 + 30 * seed, half=(seed % 2 == 1), tiny_rows=3 + seed)
    return rows[:len(rows) * 4 // 5]


def _first_tiny_seed():
    for seed in range(6):
        if _no_zero_scale(_tiny_case(seed)):
            return seed
    raise AssertionError("no generator seed without a scale() == 0 corner")


def test_order_of_the_batch_is_the_order_of_the_calls(kn, oracle, tmp_path):
    train = _tiny_case(_first_tiny_seed())
    tr = _cols(train)
    users = np.unique(np.asarray(tr[0], dtype=np.int32))
    assert min(np.bincount(np.unique(tr[0], return_inverse=True)[1])) <= 4
    m = oracle.Model(*tr)
    rng = np.random.default_rng(8)
    for j, order in enumerate((users[::-1].copy(), rng.permutation(users))):
        for k in (2, 5):
            a, b = kn.Engine(k=k), kn.Engine(k=k)
            a.fit(*tr)
            b.fit(*tr)
            got = a.recommend_batch(kn.PRED_KNN, order, 4)
            _same(got, _loop(b, kn.PRED_KNN, order, 4), (j, k))
            p = m.pipeline(oracle.SIM_COSINE, k)
            for r, u in enumerate(order):
                oi, op = p.recommend(int(u), 4)
                assert got[0][r, :got[2][r]].tolist() == oi.tolist() and _bits(got[1][r, :got[2][r]]) == _bits(op), (j, k, u)
            _same_lists_and_order(_table(a, tmp_path / "a.nb"), _table(b, tmp_path / "b.nb"))
            a.close()
            b.close()


def _oracle_rows(p, users, n):
    """the pipeline's recommend(u, n) for every user in order: [(item ids, prediction bits)]"""
    out = []
    for u in users:
        ids, preds = p.recommend(int(u), n)
        out.append((ids.tolist(), preds.view(np.int64).tolist()))
    return out


def _rows(got):
    return [(got[0][b, :got[2][b]].tolist(), got[1][b, :got[2][b]].view(np.int64).tolist()) for b in range(len(got[2]))]


def test_history_is_the_reference_s(kn, oracle):
    """rating_scales.history_case, cosine, k = 5: user 17's mean is negative, so recommend(17, 3) is answered at :573 and builds
    no neighbourhood (test_rating_scale_premises: building it changes the bits of other lists).  One chunk, chunks of 7 with a
    remainder, and a loop of single calls all leave the lists the oracle's pipeline holds after the same calls"""
    train, _ = rs.history_case()
    tr = rs.cols(train)
    fitted = np.unique(tr[0]).astype(np.int32)
    users = np.asarray(([17] + fitted.tolist()) * 2, dtype=np.int32)  # (repeats of listed users change no history)
    n_items = len(np.unique(tr[1]))
    p = oracle.Model(*tr).pipeline(oracle.SIM_COSINE, 5)
    rows = _oracle_rows(p, users, 3)
    after = [(i.tolist(), s.view(np.int64).tolist()) for i, s in (p.neighbors(int(u)) for u in fitted)]
    batch = lambda e: e.recommend_batch(kn.PRED_KNN, users, 3)
    for name, workspace, ask in (("one chunk", 0, batch), ("chunks of 7", _workspace_for(7, n_items), batch),
                                 ("loop", 0, lambda e: _loop(e, kn.PRED_KNN, users, 3))):
        e = kn.Engine(k=5, workspace_bytes=workspace).fit(*tr)
        assert _rows(ask(e)) == rows, name
        ids, sims, cnt = e.neighbors_batch(fitted)
        assert [(ids[j, :cnt[j]].tolist(), sims[j, :cnt[j]].view(np.int64).tolist()) for j in range(len(fitted))] == after, name
        e.close()


def test_small_and_large_batches_on_the_order_dependent_case(kn, oracle):
    """B = 1 (the single call's shape), 2 and beyond the number of users, on the tiny case with <= 4-rating users: the batch is the
    loop of single calls and the oracle, for both selections"""
    train = _tiny_case(_first_tiny_seed())
    tr = _cols(train)
    known = np.unique(np.asarray(tr[0], dtype=np.int32))
    pool = np.concatenate([known[::-1], [31_337], np.random.default_rng(9).permutation(known)]).astype(np.int32)
    m = oracle.Model(*tr)
    for B in (1, 2, len(known), len(pool)):
        users = pool[:B]
        for n in (3, FAST_N + 5):
            a, b = kn.Engine(k=5).fit(*tr), kn.Engine(k=5).fit(*tr)
            got = a.recommend_batch(kn.PRED_KNN, users, n)
            _same(got, _loop(b, kn.PRED_KNN, users, n), (B, n))
            assert _rows(got) == _oracle_rows(m.pipeline(oracle.SIM_COSINE, 5), users, n), (B, n)
            a.close()
            b.close()


# ---- 4. chunk independence ------------------------------------------------------------------------------------------------------
def _workspace_for(chunk, n_items):
    """workspace_bytes that makes the chunk rule of include/knncf.h give `chunk`"""
    return 2 * chunk * 96 * n_items + 2


def test_results_do_not_depend_on_the_chunk(kn, syn100k):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    n_items = len(np.unique(train[1]))
    users = _mixed_users(train, 45, seed=5)
    answers = []
    for chunk in (1, 7, 44, None):  # 45 users; 44: a remainder of one
        e = kn.Engine(k=30, workspace_bytes=0 if chunk is None else _workspace_for(chunk, n_items))
        e.fit(*train)
        answers.append([e.recommend_batch(kn.PRED_KNN, users, n) for n in (3, FAST_N + 5)] +
                       [e.recommend_batch(kn.PRED_BASELINE, users, 3)])
        e.close()
    for other in answers[1:]:
        for x, y in zip(answers[0], other):
            _same(x, y)


# ---- 5. both sides of the selection switch, and the edges ---------------------------------------------------------------------
def test_selection_switch_and_edges(kn, syn100k):
    d = syn100k
    u, i, r = d.train.users, d.train.items, d.train.ratings
    all_items = np.unique(i)
    full_user, lone_item = 777_001, 777_002  # a user who rated every item (one of them alone)
    u = np.concatenate([u, np.full(len(all_items) + 1, full_user)]).astype(np.int32)
    i = np.concatenate([i, all_items, [lone_item]]).astype(np.int32)
    r = np.concatenate([r, 1.0 + (np.arange(len(all_items) + 1) % 5)])
    train = (u, i, r)
    I = len(all_items) + 1
    users = np.array(_spread_users(train, 12) + [full_user, 555_555, full_user], dtype=np.int32)
    a, b = kn.Engine(k=25), kn.Engine(k=25)
    a.fit(*train)
    b.fit(*train)
    assert a.num_items == I
    for n in (0, 1, FAST_N - 1, FAST_N, FAST_N + 1, I - 1, I, I + 10):
        got = a.recommend_batch(kn.PRED_KNN, users, n)
        _same(got, _loop(b, kn.PRED_KNN, users, n), n)
        assert got[2][-1] == 0 and got[2][-2] == min(n, I)
        assert got[0].shape == (len(users), n)
    # the item with a single rater is recommended to the others at the user's mean (nobody in a neighbourhood rated it)
    got = a.recommend_batch(kn.PRED_KNN, users[:3], I)
    assert all(lone_item in got[0][row, :got[2][row]].tolist() for row in range(3))
    empty = a.recommend_batch(kn.PRED_KNN, np.empty(0, dtype=np.int32), 3)
    assert empty[0].shape == (0, 3) and len(empty[2]) == 0
    a.close()
    b.close()


# ---- 6. shard handles ------------------------------------------------------------------------------------------------------------
def _shard_case(rows):
    c = _cols(rows)
    return tuple(np.ascontiguousarray(a) for a in (np.asarray(c[0], np.int32), np.asarray(c[1], np.int32), np.asarray(c[2], np.float64)))


def _committed_shards(kn, pkg, trc, world, k):
    """`world` shard handles of device 0 fitted on trc, the means and norms exchanged, committed: (engines, device tensors)"""
    import torch

    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    dev = torch.device("cuda", 0)
    tr = tuple(torch.from_numpy(a).to(dev) for a in trc)
    engines = [kn.Engine(k=k, shard_rank=rk, shard_count=world) for rk in range(world)]
    views = []
    for e in engines:
        e.fit_device(*tr)
        views.append(sharded.DeviceEngineAdapter(e, dev).shard_tensors())
    for me in range(world):
        for other in range(world):
            if other != me:
                lo, hi = views[other]["user_range"]
                for key in ("user_avg", "user_norm"):
                    views[me][key][lo:hi] = views[other][key][lo:hi]
    torch.cuda.synchronize()
    for e in engines:
        e.shard_commit()
    return engines, tr


def test_shard_handles_answer_their_own_users(kn, pkg):
    rng = np.random.default_rng(77)
    trc = _shard_case(_random_case(rng, n_users=40, n_items=30, n_ratings=800, half=True, tiny_rows=0))
    assert min(np.bincount(np.unique(trc[0], return_inverse=True)[1])) > 4
    world, k, n = 3, 6, 4
    engines, tr = _committed_shards(kn, pkg, trc, world, k)
    for e in engines:
        e.mae_device(kn.PRED_KNN, *tr)  # the replicated call numbers every user on every shard
    single = kn.Engine(k=k)
    single.fit(*trc)
    single.mae(kn.PRED_KNN, *trc)
    users = np.concatenate([np.unique(trc[0]), [424_242]]).astype(np.int32)
    want = single.recommend_batch(kn.PRED_KNN, users, n)
    owner = []
    for u in users:
        mine = []
        for rk, e in enumerate(engines):
            try:
                e.recommend(kn.PRED_KNN, int(u), 1)
                mine.append(rk)
            except kn.KnncfError as ex:
                assert ex.status == kn.E_STATE
        assert len(mine) == 1
        owner.append(mine[0])
    owner = np.asarray(owner)
    assert owner[-1] == 0 and set(owner.tolist()) == {0, 1, 2}
    for rk, e in enumerate(engines):
        sel = np.flatnonzero(owner == rk)
        got = e.recommend_batch(kn.PRED_KNN, users[sel], n)
        _same(got, tuple(x[sel] for x in want), rk)
        # a foreign user fails the whole call with nothing written
        foreign = users[np.flatnonzero(owner != rk)[0]]
        mixed = np.concatenate([users[sel][:2], [foreign]]).astype(np.int32)
        items = np.full((3, n), -7, dtype=np.int32)
        preds = np.full((3, n), -7.0)
        counts = np.full(3, -7, dtype=np.int32)
        p = lambda arr, t: arr.ctypes.data_as(C.POINTER(t))
        st = e._lib.knncf_recommend_batch(e._h, kn.PRED_KNN, p(mixed, C.c_int32), 3, n, p(items, C.c_int32), p(preds, C.c_double),
                                          p(counts, C.c_int32))
        assert st == kn.E_STATE
        assert (items == -7).all() and (preds == -7.0).all() and (counts == -7).all()
    for e in engines + [single]:
        e.close()


def test_single_call_on_a_shard_takes_the_batch_s_numbering_rule(kn, pkg):
    """a train set with <= 4-rating users on two shard handles: a recommendation that would have to build (and number, on this
    shard only) a neighbourhood is refused, by the single call as by the batch; after the replicated mae has numbered every user
    on every shard, the single call answers what a single handle answers"""
    rng = np.random.default_rng(78)
    trc = _shard_case(_random_case(rng, n_users=20, n_items=19, n_ratings=200, half=True, tiny_rows=4))
    assert min(np.bincount(np.unique(trc[0], return_inverse=True)[1])) <= 4
    world, k, n = 2, 5, 3
    engines, tr = _committed_shards(kn, pkg, trc, world, k)
    known = np.unique(trc[0]).astype(np.int32)
    p = lambda arr, t: arr.ctypes.data_as(C.POINTER(t))

    def owner_of(u):  # GLOBAL_AVG builds nothing: E_STATE off the owning shard
        mine = []
        for rk, e in enumerate(engines):
            try:
                e.recommend(kn.PRED_GLOBAL_AVG, int(u), 1)
                mine.append(rk)
            except kn.KnncfError as ex:
                assert ex.status == kn.E_STATE
        assert len(mine) == 1
        return mine[0]

    owner = [owner_of(u) for u in known]
    assert set(owner) == {0, 1}
    for rk, e in enumerate(engines):
        u = int(known[owner.index(rk)])
        items, preds, count = np.full(n, -7, dtype=np.int32), np.full(n, -7.0), C.c_int32(-7)
        st = e._lib.knncf_recommend(e._h, kn.PRED_KNN, u, n, p(items, C.c_int32), p(preds, C.c_double), C.byref(count))
        assert st == kn.E_UNSUPPORTED
        assert count.value == 0 and (items == -7).all() and (preds == -7.0).all()
        with pytest.raises(kn.KnncfError) as ex:
            e.recommend_batch(kn.PRED_KNN, [u], n)
        assert ex.value.status == kn.E_UNSUPPORTED
    for e in engines:
        e.mae_device(kn.PRED_KNN, *tr)
    single = kn.Engine(k=k).fit(*trc)
    single.mae(kn.PRED_KNN, *trc)
    for u, rk in zip(known, owner):
        gi, gp = engines[rk].recommend(kn.PRED_KNN, int(u), n)
        wi, wp = single.recommend(kn.PRED_KNN, int(u), n)
        assert gi.tolist() == wi.tolist() and _bits(gp) == _bits(wp), int(u)
    for e in engines + [single]:
        e.close()


# ---- 7. call-level errors ------------------------------------------------------------------------------------------------------
def test_call_level_errors_leave_everything_untouched(kn, syn100k, tmp_path):
    d = syn100k
    train = (d.train.users, d.train.items, d.train.ratings)
    users = np.unique(train[0])[:5].astype(np.int32)
    n = 3
    items = np.full((5, n), -7, dtype=np.int32)
    preds = np.full((5, n), -7.0)
    counts = np.full(5, -7, dtype=np.int32)
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    p = lambda arr, t: arr.ctypes.data_as(t)
    null_i, null_d = C.cast(None, i32p), C.cast(None, f64p)

    def call(e, pred, us, n_users, n_, it=None, pr=None, ct=None):
        return e._lib.knncf_recommend_batch(e._h, pred, us, n_users, n_, p(items, i32p) if it is None else it,
                                            p(preds, f64p) if pr is None else pr, p(counts, i32p) if ct is None else ct)

    e = kn.Engine(k=10)
    assert call(e, kn.PRED_KNN, p(users, i32p), 5, n) == kn.E_STATE  # before a fit
    e.fit(*train)
    before = _table(e, tmp_path / "before.nb")
    assert call(e, kn.PRED_KNN, null_i, 5, n) == kn.E_INVALID
    assert call(e, kn.PRED_KNN, p(users, i32p), 5, n, it=null_i) == kn.E_INVALID
    assert call(e, kn.PRED_KNN, p(users, i32p), 5, n, pr=null_d) == kn.E_INVALID
    assert call(e, kn.PRED_KNN, p(users, i32p), 5, n, ct=null_i) == kn.E_INVALID
    assert call(e, kn.PRED_KNN, p(users, i32p), -1, n) == kn.E_INVALID
    assert call(e, kn.PRED_KNN, p(users, i32p), 5, -1) == kn.E_INVALID
    assert call(e, 99, p(users, i32p), 5, n) == kn.E_INVALID
    assert (items == -7).all() and (preds == -7.0).all() and (counts == -7).all()
    assert _table(e, tmp_path / "after.nb") == before
    assert call(e, kn.PRED_KNN, null_i, 0, n, it=null_i, pr=null_d, ct=null_i) == kn.OK  # n_users == 0 touches nothing
    assert call(e, kn.PRED_KNN, p(users, i32p), 5, 0, it=null_i, pr=null_d) == kn.OK     # n == 0: counts only
    assert (counts == 0).all() and (items == -7).all()
    assert _table(e, tmp_path / "after.nb") == before
    e.close()
    one = kn.Engine(k=10, similarity=kn.SIM_ONE)
    one.fit(*train)
    counts[:] = -7
    assert call(one, kn.PRED_KNN, p(users, i32p), 5, n) == kn.E_UNSUPPORTED
    with pytest.raises(kn.KnncfError) as ex:
        one.recommend(kn.PRED_KNN, int(users[0]), n)  # ... exactly where the single call refuses
    assert ex.value.status == kn.E_UNSUPPORTED
    assert (items == -7).all() and (preds == -7.0).all() and (counts == -7).all()
    one.close()


# ---- 8. the ml-25m shape ----------------------------------------------------------------------------------------------------------
def test_ml25m_shape(kn, oracle, synth):
    d = synth.syn_25m()
    train = (d.train.users, d.train.items, d.train.ratings)
    k, n = 300, 3
    known = np.unique(train[0])
    users = known[::len(known) // 4096][:4096].astype(np.int32)
    assert len(users) == 4096
    a, b = kn.Engine(k=k), kn.Engine(k=k)
    a.fit(*train)
    b.fit(*train)
    assert (a.num_users, a.num_items) == (162_541, 59_047)
    got = a.recommend_batch(kn.PRED_KNN, users, n)
    assert (got[2] == n).all()
    again = a.recommend_batch(kn.PRED_KNN, users, n)  # warm: every list exists
    _same(got, again)
    rows = np.arange(0, 4096, 64)
    b.neighbors_batch(users)  # the twin builds the same lists in the same order, then answers one user at a time
    _same(tuple(x[rows] for x in got), _loop(b, kn.PRED_KNN, users[rows], n))
    p = oracle.Model(*train).pipeline(oracle.SIM_COSINE, k)
    for r in rows[::16]:
        oi, op = p.recommend(int(users[r]), n)
        assert got[0][r].tolist() == oi.tolist() and _bits(got[1][r]) == _bits(op), int(users[r])
    a.close()
    b.close()
