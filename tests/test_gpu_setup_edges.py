"""The fit's set-up stage (prep.hip, sort_util.hip) at its size-class, fold-chunk, scan-tile, sort-tile and id edges, against
the oracle bit for bit.

tests/setup_edges.py builds the inputs: row lengths on, one below and one above the caps of the three per-user LDS sort
classes and one beyond the last (A), user and item segments across the 2 048-element cuts of k_ordered_fold (B), user counts
around the 2 048-user scan tile and files grouped into runs of equal users (C), rating counts around the radix sort's tiles,
its self-scan limit and its pass count (D), ids at the ends of the direct tables and of int32 (E), and fits of at most five
users, ratings or items (F).  tests/test_setup_edge_premises.py proves on the CPU that every case sits where it claims to.

What is compared, every case: the WHOLE arrays of knncf_shard_view_get — the means and norms in dense order, the normalized
deviations and preprocessed ratings in canonical (dense user, dense item) order — with the oracle's, which pins the dense
ids, the canonical order, both fold orders and K1 - K3; the global average, the counts, the per-item statistics and the three
item-side predictors on the test rows (K4 and its two sorts); similarity(u, v) of the planted users against fresh closures;
and, where the case says so, the kNN predictions and the planted users' neighbour lists at k = 10 (prep_commit's item-major
sort and what hangs on it).  Every comparison is on bit patterns; only the MAE keeps MAE_TOL.  Each test also asserts the
`knncf-dispatch prep` / `sort` lines of KNNCF_DEBUG_TRACE_DISPATCH=setup that say which path ran."""
import importlib

import numpy as np
import pytest

from tests import setup_edges as se
from tests.test_gpu_k_classes import MAE_TOL, TRACE, _trace

pytestmark = pytest.mark.gpu
K = se.K
GLOBAL_ORDER, NO_TABLES = "KNNCF_DEBUG_GLOBAL_HASH_ORDER", "KNNCF_DEBUG_NO_ID_TABLES"


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def _same_bits(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


class _Ref:
    """the oracle's answers for one case, each computed once and left unchanged"""

    def __init__(self, oracle, name):
        self.oracle = oracle
        self.case = c = se.case(name)
        self.model = m = oracle.Model(*c.train)
        self.order = m.user_iteration_order()
        self.avg = np.array([m.users_avg(int(u)) for u in self.order])
        self.norm = np.array([m.user_weight(int(u)) for u in self.order])
        canon = se.canonical(c.train, self.order)
        self.dev = m.normalized_deviations()[canon]
        self.pre = m.preprocessed()[canon]
        self.ptr = np.concatenate([[0], np.cumsum(np.bincount(se.rank_of(self.order, c.train[0]), minlength=len(self.order)))])
        self.lengths = se.lengths_of(c.train)
        self._knn = None

    def knn_rows(self):
        """the test rows the kNN comparison uses: not those of a fitted user with at most four ratings"""
        te = self.case.test
        keep = np.array([self.lengths.get(int(u), 5) >= 5 for u in te[0]], dtype=bool)
        return tuple(a[keep] for a in te)

    def knn_users(self):
        return [int(u) for u in self.case.planted if self.lengths[int(u)] >= 5]

    def knn(self):
        """(MAE, predictions, neighbour lists) of one pipeline: the test rows first, then the planted users' lists in order"""
        if self._knn is None:
            p = self.model.pipeline(self.oracle.SIM_COSINE, K)
            te = self.knn_rows()
            want, preds = p.mae(*te, True) if len(te[0]) else (float("nan"), np.empty(0))
            self._knn = (want, preds, [p.neighbors(u) for u in self.knn_users()] if self.case.knn else [])
        return self._knn


@pytest.fixture(scope="module")
def refs(oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Ref(oracle, name)
        return made[name]

    return get


def _hooks(monkeypatch, global_order=False, no_tables=False):
    monkeypatch.setenv(TRACE, "setup")  # (the value that adds the set-up stage's lines)
    for env, on in ((GLOBAL_ORDER, global_order), (NO_TABLES, no_tables)):
        if on:
            monkeypatch.setenv(env, "1")
        else:
            monkeypatch.delenv(env, raising=False)


def _fit(kn, c, capfd, **kw):
    """a fresh handle fitted on the case's training rows; (handle, its `prep` trace line, every trace line of the fit)"""
    e = kn.Engine(k=K, flags=kn.FLAG_VERIFY_BOUND, **kw)
    capfd.readouterr()
    e.fit(*c.train)
    lines = _trace(capfd)
    prep = [ln for ln in lines if ln.startswith("prep ")]
    assert len(prep) == 1, lines
    print(f"[dispatch] {prep[0]}")
    return e, prep[0], lines


def _prep_line(ids="table", order="segments", mid=0, long=0, uf=0, uh=1):
    return f"prep ids={ids} order={order} mid={mid} long={long} uf={uf} uh={uh}"


def _view(pkg, e):
    """the four arrays of knncf_shard_view_get on the host, and the view"""
    import torch

    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    t = sharded.DeviceEngineAdapter(e, torch.device("cuda", e.device)).shard_tensors()
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy().copy() if hasattr(v, "cpu") else v) for k, v in t.items()}


def _check_view(pkg, e, ref, users=None, rows=None):
    """the whole arrays (or the owned user range / position range of a shard that has not exchanged yet)"""
    v = _view(pkg, e)
    U, n = len(ref.order), len(ref.dev)
    assert len(v["user_avg"]) == U and len(v["dev"]) == n
    us = slice(*(users or (0, U)))
    rs = slice(*(rows or (0, n)))
    _same_bits(v["user_avg"][us], ref.avg[us], "user_avg")
    _same_bits(v["user_norm"][us], ref.norm[us], "user_norm")
    _same_bits(v["dev"][rs], ref.dev[rs], "dev")
    _same_bits(v["pre"][rs], ref.pre[rs], "pre")
    return v


def _check_stats(kn, e, ref, every_item=False):
    """K1 and K4: the global average, the counts, the item statistics, the item-side predictors on the test rows"""
    c, m, oracle = ref.case, ref.model, ref.oracle
    assert _bits(e.global_avg()) == _bits(m.average())
    assert (e.num_users, e.num_items) == (m.num_users, m.num_items)
    all_items = np.unique(c.train[1])
    items = all_items if every_item else np.unique(np.concatenate([c.items, all_items[::max(1, len(all_items) // 40)]]))
    items = [int(i) for i in items]
    _same_bits([e.item_avg(i) for i in items], [m.items_avg(i) for i in items], "item_avg")
    _same_bits([e.item_avg_dev(i) for i in items], [m.items_avg_dev(i) for i in items], "item_avg_dev")
    _same_bits([e.item_avg_dev_rdd(i) for i in items], [m.items_avg_dev_spark(i) for i in items], "item_avg_dev_rdd")
    te = c.test
    if len(te[0]):
        for kind, okind in ((kn.PRED_ITEM_AVG, oracle.KIND_ITEM), (kn.PRED_BASELINE, oracle.KIND_BASELINE),
                            (kn.PRED_BASELINE_RDD, oracle.KIND_BASELINE_SPARK)):
            want, preds = m.mae(okind, *te, True)
            _same_bits(e.predict_batch(kind, te[0], te[1]), preds, ("predictor", kind))
            assert abs(e.mae(kind, *te) - want) <= MAE_TOL, kind


def _check_similarity(e, ref):
    """every planted user against about 50 users spaced over the dense order (fresh closures: no memo history)"""
    m, oracle = ref.model, ref.oracle
    others = ref.order[::max(1, len(ref.order) // 50)].tolist()
    for u in ref.case.planted.tolist():
        vs = [v for v in others if v != u]
        _same_bits([e.similarity(u, v) for v in vs], [m.fresh_similarity(oracle.SIM_COSINE, u, v) for v in vs], ("similarity", u))


def _check_knn(kn, e, ref):
    """the kNN predictions of the test rows, then the lists of the planted users with at least five ratings, in the oracle's
    order of calls"""
    want, opreds, lists = ref.knn()
    te = ref.knn_rows()
    if len(te[0]):
        _same_bits(e.predict_batch(kn.PRED_KNN, te[0], te[1]), opreds, "knn predictions")
        got = e.mae(kn.PRED_KNN, *te)
        print(f"[figure] kNN MAE over {len(te[0])} rows: engine {got!r} oracle {want!r}")
        assert abs(got - want) <= MAE_TOL
    for u, (oids, osims) in zip(ref.knn_users(), lists):
        ids, sims = e.neighbors(u)
        assert ids.tolist() == oids.tolist(), u
        _same_bits(sims, osims, ("neighbours", u))
    assert e.timings()["max_bound_violation"] <= 0.0


def _check_all(kn, pkg, e, ref, every_item=False, knn_predictions=None):
    _check_view(pkg, e, ref)
    _check_stats(kn, e, ref, every_item)
    _check_similarity(e, ref)
    if ref.case.knn or knn_predictions:
        _check_knn(kn, e, ref)


def _sort_line(key, n, bits):
    tile = se.RS_TILE_U32 if key == 32 else se.RS_TILE_U64
    tiles = -(-n // tile)
    return f"sort key={key} n={n} tiles={tiles} passes={-(-bits // 8)} scan={'self' if tiles <= se.RS_SELF_SCAN_TILES else 'kernel'}"


def _n_key_sorts(n, U, I, global_order=False, no_tables=False, need_uf=True):
    """the trace lines of every radix sort over all n ratings that a fit, its commit and prep_item_stats run (written out from
    prep.hip's calls, with the key widths of common.h bits_for)"""
    ub, ib, tb = se.bits_for(U), se.bits_for(I), se.bits_for(n)
    want = {_sort_line(32, n, ib),                             # prep_commit: positions by item
            _sort_line(64, n, tb + ib), _sort_line(64, n, 32 + ib)}  # prep_item_stats: (item, file row), (item, trie key)
    if global_order:
        want |= {_sort_line(64, n, ib + ub), _sort_line(64, n, 32 + ub)}  # the canonical order, (user, trie key)
        if need_uf:
            want.add(_sort_line(32, n, ub))                    # (user, file row)
    if no_tables:
        want.add(_sort_line(32, n, 32))                        # every row's user key / item key, before unique_u32
    return want


def _sorts_of(lines, n):
    return {ln for ln in lines if ln.startswith("sort ") and f" n={n} " in ln}


# ---- A: row-length classes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("global_order", [False, True])
@pytest.mark.parametrize("name", ["a_half", "a_off"])
def test_a_row_length_classes(kn, pkg, refs, monkeypatch, capfd, name, global_order):
    """one user per row length 1 .. 5, 2^p - 1, 2^p, 2^p + 1 (p = 6 .. 12) and 8 191, 8 192: both sides of `n > CAP` of every
    class, every padded size of the bitonic network and both sides of its barrier rule (strides of 128 and more).  a_half is
    dyadic — k_exact_sum, usersAvg folded in the canonical order, no perm_uf; its means cannot tell a wrong order, its norms
    can (premise file) — a_off is off the grid: usersAvg folds along perm_uf.  Then the same files with the global sorts forced."""
    ref = refs(name)
    _hooks(monkeypatch, global_order=global_order)
    e, prep, lines = _fit(kn, ref.case, capfd)
    uf = 0 if name == "a_half" else 1
    if global_order:
        assert prep == _prep_line(order="global", uf=uf)
    else:
        assert prep == _prep_line(mid=ref.case.facts["mid"], long=ref.case.facts["long"], uf=uf)
    _check_all(kn, pkg, e, ref)
    e.close()


def test_a_longest_row_alone_takes_the_global_sorts(kn, pkg, refs, monkeypatch, capfd):
    """A': one user of 8 193 ratings beside the same lengths: `max_len <= SEG_BLOCK_CAP` fails and the whole fit is ordered by
    the global radix sorts, no hook set"""
    ref = refs("a_beyond")
    _hooks(monkeypatch)
    e, prep, lines = _fit(kn, ref.case, capfd)
    assert prep == _prep_line(order="global", uf=1)
    n, U, I = len(ref.dev), len(ref.order), ref.model.num_items
    _check_all(kn, pkg, e, ref)
    assert _sorts_of(lines + _trace(capfd), n) == _n_key_sorts(n, U, I, global_order=True)
    e.close()


def _shards(kn, pkg, ref, count, capfd):
    """`count` shard handles in one process: fit, the owned parts of every view against the oracle, the exchange by device
    copies, commit, the completed views against the oracle; (handles, device test columns, prep lines)"""
    import torch

    sharded = importlib.import_module(pkg.__name__ + ".sharded")
    c = ref.case
    dev = torch.device("cuda", 0)
    tr = tuple(torch.from_numpy(np.array(a)).to(dev) for a in c.train)
    te = tuple(torch.from_numpy(np.array(a)).to(dev) for a in ref.knn_rows())
    engines = [kn.Engine(k=K, shard_rank=r, shard_count=count) for r in range(count)]
    views, preps = [], []
    U = len(ref.order)
    per = -(-U // count)
    for r, e in enumerate(engines):
        capfd.readouterr()
        e.fit_device(*tr)
        preps += [ln for ln in _trace(capfd) if ln.startswith("prep ")]
        v = sharded.DeviceEngineAdapter(e, dev).shard_tensors()
        lo, hi = min(per * r, U), min(per * (r + 1), U)
        assert v["user_range"] == (lo, hi) and v["nnz_range"] == (ref.ptr[lo], ref.ptr[hi])
        _check_view(pkg, e, ref, users=(lo, hi), rows=(int(ref.ptr[lo]), int(ref.ptr[hi])))
        views.append(v)
    for me in range(count):  # the exchange: every other shard's per-user (mean, norm)
        for other in range(count):
            lo, hi = views[other]["user_range"]
            if other != me and hi > lo:
                for key in ("user_avg", "user_norm"):
                    views[me][key][lo:hi] = views[other][key][lo:hi]
    torch.cuda.synchronize()
    for e in engines:
        e.shard_commit()
        _check_view(pkg, e, ref)
    return engines, tr, te, preps


def _check_shard_predictions(kn, ref, engines, tr, te):
    """the partial (sum |err|, rows) pairs add up to a single handle's; the predictions, each row written by its owner, are
    the oracle's"""
    import torch

    want, opreds, _ = ref.knn()
    single = kn.Engine(k=K)
    single.fit_device(*tr)
    s1, c1 = single.mae_device(kn.PRED_KNN, *te)
    preds = torch.zeros(len(opreds), dtype=torch.float64, device=te[0].device)
    total, count, parts = 0.0, 0, []
    for e in engines:
        s, c = e.mae_device(kn.PRED_KNN, *te, pred_out=preds)
        parts.append((s, c))
        total += s
        count += c
    print(f"[figure] partial sums {parts}, single ({s1!r}, {c1})")
    assert count == c1 == len(opreds)
    _same_bits(preds.cpu().numpy(), opreds, "shard predictions")
    assert abs(total / count - s1 / c1) <= MAE_TOL and abs(total / count - want) <= MAE_TOL
    single.close()
    return parts


@pytest.mark.parametrize("name", ["a_off", "a_beyond"])
def test_a_two_shards_on_one_gpu(kn, pkg, refs, monkeypatch, capfd, name):
    """two shard handles, each ordering only its own users: by the per-user LDS sorts (a_off) and, with the 8 193-row user,
    by the slice sorts k_slice_file_keys / k_slice_hash_keys (a_beyond)"""
    ref = refs(name)
    _hooks(monkeypatch)
    engines, tr, te, preps = _shards(kn, pkg, ref, 2, capfd)
    if name == "a_off":
        assert preps == [_prep_line(mid=6, long=6, uf=1)] * 2
    else:
        assert preps == [_prep_line(order="global", uf=1)] * 2
    _check_shard_predictions(kn, ref, engines, tr, te)
    for e in engines:
        e.close()


@pytest.mark.parametrize("name,length", [(name, L) for name, ls in se.A_DUPLICATES.items() for L in ls])
def test_a_duplicate_rows_in_every_class(kn, pkg, refs, monkeypatch, capfd, name, length):
    """one (user, item) pair twice in the row of 511 / 512 (then 512 / 513 rows: the one-wave class and the first of the next),
    2 047 / 2 048, 8 191 / 8 192 (then 8 193: the global path by length) and in the 8 193 one: KNNCF_E_DUPLICATE from every
    class and from the global sorts, and the handle fits the clean file afterwards"""
    ref = refs(name)
    c = ref.case
    user = {v: k for k, v in c.facts["lengths"].items()}[length]
    _hooks(monkeypatch)
    e = kn.Engine(k=K)
    capfd.readouterr()
    with pytest.raises(kn.KnncfError) as ex:
        e.fit(*se.with_duplicate(c, user))
    assert ex.value.status == kn.E_DUPLICATE
    prep, = [ln for ln in _trace(capfd) if ln.startswith("prep ")]
    print(f"[dispatch] {prep}")
    if max(c.facts["lengths"].values()) > se.SEG_BLOCK_CAP or length + 1 > se.SEG_BLOCK_CAP:
        assert prep == _prep_line(order="global", uf=1)
    else:  # the row moved to the class of length + 1
        in_mid = lambda L: se.SEG_SHORT_CAP < L <= se.SEG_MID_CAP
        in_long = lambda L: se.SEG_MID_CAP < L <= se.SEG_BLOCK_CAP
        assert prep == _prep_line(mid=c.facts["mid"] + in_mid(length + 1) - in_mid(length),
                                  long=c.facts["long"] + in_long(length + 1) - in_long(length), uf=1)
    e.fit(*c.train)
    _check_view(pkg, e, ref)
    _check_knn(kn, e, ref)
    e.close()


# ---- B: fold chunks ---------------------------------------------------------------------------------------------------------------
def test_b_user_segments_across_the_fold_chunks(kn, pkg, refs, monkeypatch, capfd):
    """600 users, ratings off the grid (fold<false> along perm_uf and fold<true> along perm_uh both see the order): twelve
    users whose segments lie across a cut of their block's 2 048-element chunks with 15 .. 33 elements on either side, at either
    buffer parity; one segment that ends on a cut, one that starts on it, one of 4 097 elements over three chunks"""
    ref = refs("b_users")
    _hooks(monkeypatch)
    e, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _prep_line(long=1, uf=1)
    _check_all(kn, pkg, e, ref)
    e.close()


def test_b_item_segments_across_the_fold_chunks(kn, pkg, refs, monkeypatch, capfd):
    """the same plan over blocks of 16 dense items: the three folds of prep_item_stats along perm_if / perm_ih; every item's
    statistics"""
    ref = refs("b_items")
    _hooks(monkeypatch)
    e, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _prep_line(uf=1)
    _check_all(kn, pkg, e, ref, every_item=True, knn_predictions=True)
    e.close()


@pytest.mark.parametrize("name", ["b_i16", "b_i17", "b_i1", "b_u256", "b_u257"])
def test_b_block_counts(kn, pkg, refs, monkeypatch, capfd, name):
    """exactly 16, 17 and 1 items (one full fold block, one block and a block of one segment, a single segment) and exactly
    256 and 257 users; every item's statistics"""
    ref = refs(name)
    _hooks(monkeypatch)
    e, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _prep_line(uf=1)
    _check_all(kn, pkg, e, ref, every_item=True)
    e.close()


# ---- C: scan tiles and wave runs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", se.C_USERS)
def test_c_scan_tiles(kn, pkg, refs, monkeypatch, capfd, U):
    """U = 1, 2 047, 2 048, 2 049, 4 096, 4 097 users in a file grouped by user: one, two and three tiles of k_user_tile_sums /
    k_user_ptr, the last of 2 047, 2 048 or 1 users; the users at both ends of the dense order are the longest"""
    ref = refs(f"c_u{U}")
    _hooks(monkeypatch)
    e, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _prep_line()
    _check_all(kn, pkg, e, ref)
    e.close()


@pytest.mark.parametrize("rem", se.C_REMAINDERS)
def test_c_wave_runs(kn, pkg, refs, monkeypatch, capfd, rem):
    """runs of exactly 63, 64, 65, 128 and 256 equal users from row offsets 0, 1 and 63 (mod 64), one across a workgroup edge,
    one user twice inside a wave; n = 0, 1, 63 (mod 64): k_count_users and k_scatter_rows aggregate each run per wave"""
    ref = refs(f"c_runs{rem}")
    _hooks(monkeypatch)
    e, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _prep_line()
    _check_all(kn, pkg, e, ref)
    e.close()


# ---- D: sort tiles and passes -----------------------------------------------------------------------------------------------------
def _run_d(kn, pkg, refs, monkeypatch, capfd, name, global_order=False, no_tables=False, every_item=True):
    ref = refs(name)
    c = ref.case
    _hooks(monkeypatch, global_order=global_order, no_tables=no_tables)
    e, prep, lines = _fit(kn, c, capfd)
    dyadic = np.array_equal(c.train[2] * 2, np.round(c.train[2] * 2))
    assert prep == _prep_line(ids="sorted" if no_tables else "table", order="global" if global_order else "segments",
                              uf=0 if dyadic else 1)
    _check_all(kn, pkg, e, ref, every_item=every_item, knn_predictions=True)
    lines += _trace(capfd)
    n, U, I = len(c.train[0]), len(ref.order), ref.model.num_items
    got, want = _sorts_of(lines, n), _n_key_sorts(n, U, I, global_order, no_tables, need_uf=not dyadic)
    print("[dispatch] " + "; ".join(sorted(got)))
    assert got == want
    e.close()
    return got


@pytest.mark.parametrize("n", se.D_SIZES)
def test_d_sort_tiles(kn, pkg, refs, monkeypatch, capfd, n):
    """n = 3 072 / 3 073 and 196 608 / 196 609 (one and 64 full tiles of 64-bit keys, then one key more: the self-scanned table
    against k_radix_scan), 4 096 / 4 097 and 262 144 / 262 145 (the same for 32-bit keys): the u64 sorts of prep_item_stats, the
    u32 sort of prep_commit"""
    got = _run_d(kn, pkg, refs, monkeypatch, capfd, f"d_n{n}")
    want = {3072: (64, 1, "self"), 3073: (64, 2, "self"), 4096: (32, 1, "self"), 4097: (32, 2, "self"),
            196608: (64, 64, "self"), 196609: (64, 65, "kernel"), 262144: (32, 64, "self"), 262145: (32, 65, "kernel")}[n]
    assert any(f"key={want[0]} n={n} tiles={want[1]} " in ln and ln.endswith(f"scan={want[2]}") for ln in got), got


@pytest.mark.parametrize("hook", ["global_order", "no_tables"])
@pytest.mark.parametrize("n", [196609, 262145])
def test_d_sort_tiles_on_the_other_paths(kn, pkg, refs, monkeypatch, capfd, n, hook):
    """the same two sizes with the global sorts forced (the three sorts of the canonical and fold orders) and with the id
    tables off (sort_keys_u32 over n row keys, unique_u32)"""
    _run_d(kn, pkg, refs, monkeypatch, capfd, f"d_n{n}", global_order=hook == "global_order", no_tables=hook == "no_tables",
           every_item=False)


@pytest.mark.parametrize("n", [se.UQ_TILE, se.UQ_TILE + 1])
def test_d_unique_tiles(kn, pkg, refs, monkeypatch, capfd, n):
    """unique_u32 over exactly one tile of UQ_TILE sorted keys, and one key more"""
    _run_d(kn, pkg, refs, monkeypatch, capfd, f"d_q{n}", no_tables=True)


@pytest.mark.parametrize("global_order", [False, True])
@pytest.mark.parametrize("name", [f"d_i{x}" for x in (255, 256, 257)] + [f"d_u{x}" for x in (255, 256, 257)])
def test_d_pass_counts(kn, pkg, refs, monkeypatch, capfd, name, global_order):
    """255, 256 and 257 items, then users: bits_for goes from 8 to 9, a sort keyed by it from one pass to two (and 32 + bits
    from five to six), and the first pass writes to the other buffer.  The item count keys prep_commit's and prep_item_stats'
    sorts; the user count keys the global order sorts, forced here."""
    got = _run_d(kn, pkg, refs, monkeypatch, capfd, name, global_order=global_order)
    x = int(name[3:])
    passes = 1 if x == 255 else 2
    if name.startswith("d_i"):
        assert any(ln.startswith("sort key=32 ") and f"passes={passes} " in ln for ln in got), got
        assert any(ln.startswith("sort key=64 ") and f"passes={passes + 4} " in ln for ln in got), got
    elif global_order:
        assert any(ln.startswith("sort key=32 ") and f"passes={passes} " in ln for ln in got), got  # (user, file row)
        assert any(ln.startswith("sort key=64 ") and f"passes={passes + 4} " in ln for ln in got), got  # (user, trie key)


# ---- E: ids -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", se.E_VARIANTS)
def test_e_id_limits(kn, pkg, refs, monkeypatch, capfd, variant):
    """ids containing 0; the largest ids at 2^24 - 1 (the last cell of the direct tables); one user id, or one item id, at 2^24
    and one user id at -1 (either sends the fit to the general path); INT32_MIN and INT32_MAX on both sides.  The test rows
    also name users and items that are negative, beyond the tables and absent inside them."""
    ref = refs(f"e_{variant}")
    _hooks(monkeypatch)
    e, prep, _ = _fit(kn, ref.case, capfd)
    assert prep == _prep_line(ids="table" if ref.case.facts["table"] else "sorted")
    _check_all(kn, pkg, e, ref)
    e.close()


# ---- F: tiny fits -----------------------------------------------------------------------------------------------------------------------
F_CASES = ([f"f_u{U}" for U in (1, 2, 3, 4, 5)] + ["f_u4_second", "f_u5_second"] + [f"f_n{n}" for n in (1, 2, 3, 4, 5)] +
           [f"f_i{I}" for I in (1, 2, 3, 4, 5)])


@pytest.mark.parametrize("no_tables", [False, True])
@pytest.mark.parametrize("name", F_CASES)
def test_f_tiny_fits(kn, pkg, refs, monkeypatch, capfd, name, no_tables):
    """one to five users (first-occurrence order up to four, trie order at five, in two file orders; two exact clones whose
    tie the dense order decides), one to five ratings (Map1..Map4: the norm folds in file order and perm_uh is not built), one
    to five items; through the direct tables and through the general id path"""
    ref = refs(name)
    c = ref.case
    _hooks(monkeypatch, no_tables=no_tables)
    e, prep, _ = _fit(kn, c, capfd)
    n = len(c.train[0])
    dyadic = np.array_equal(c.train[2] * 2, np.round(c.train[2] * 2))
    assert prep == _prep_line(ids="sorted" if no_tables else "table", uf=1 if (not dyadic or n <= 4) else 0, uh=1 if n > 4 else 0)
    _check_all(kn, pkg, e, ref, every_item=True)
    e.close()


def test_f_empty_shards(kn, pkg, refs, monkeypatch, capfd):
    """five users on eight shard handles: ranks 5 - 7 own no user (prep_fit's `hi > lo` guards, an empty position range, no
    test row to predict); the eight partial sums add up to the single handle's and the predictions are the oracle's"""
    ref = refs("f_u5")
    _hooks(monkeypatch)
    engines, tr, te, preps = _shards(kn, pkg, ref, 8, capfd)
    assert preps == [_prep_line(uf=1)] * 8
    parts = _check_shard_predictions(kn, ref, engines, tr, te)
    assert [c for _, c in parts] == [2, 2, 2, 2, 2, 0, 0, 0] and [s for s, _ in parts[5:]] == [0.0, 0.0, 0.0]
    for e in engines:
        e.close()
