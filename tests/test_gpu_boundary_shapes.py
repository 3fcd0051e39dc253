"""The neighbour build at its tile, chunk and padding edges, against the oracle bit for bit.

tests/boundary_shapes.py puts U, I, the head width, a row's tail length and the build count on, one below and one above the
sizes the kernels are built around: the 256-row GEMM tile / U_pad / R rows per block (A), K_pad = round_up(head, 64) and a
head of all items (B), the 16 384 columns k_tail_select holds at a time (C), the 12 tiles whose rater counts fit in registers
(D), the 256 tail entries of a chunk (E), the 1024-slot piece table (F), and the `count > 256` / `count * 2 >= U` tests of
build_neighbors (G).  tests/test_boundary_premises.py proves from the data and the oracle alone that every case sits where it
claims to; edge users are placed by DENSE index (HashSet rank of the raw id), which is what decides a user's panel column.

Bars: neighbour ids equal, fp64 similarities and predictions equal as bit patterns, |dMAE| <= 1e-9.  Each test prints its path
witnesses (fallback_rows, select_launches, gemm_launches, shortlist_total, head_items) before asserting them; no case here
may leave the ordinary path (fallback_rows == 0)."""
import importlib

import numpy as np
import pytest

from tests import boundary_shapes as bs
from tests.test_gpu_degenerate_rows import _bits, _engine, _equal_pipeline, _rows_equal_table, _symmetric, _witness
from tests.test_gpu_fold_in import _check as _check_fold_in

pytestmark = pytest.mark.gpu
K = bs.K
HEAD_ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def refs(oracle):
    """the oracle's answers, each computed once and left unchanged: the model of a case, its bulk kNN table (cosine) for a
    set of users (None: everybody), and the per-pair closures' lists and predictions (Jaccard) for everybody"""
    models, tables, pipes = {}, {}, {}

    class Refs:
        @staticmethod
        def model(name):
            if name not in models:
                models[name] = oracle.Model(*bs.case(name).train)
            return models[name]

        @staticmethod
        def table(name, k, users=None):
            if (name, k) not in tables:
                tables[name, k] = Refs.model(name).knn_table(k, users=users)
            return tables[name, k]

        @staticmethod
        def jaccard(name, k):
            if (name, k) not in pipes:
                c = bs.case(name)
                p = Refs.model(name).pipeline(oracle.SIM_JACCARD, k)
                users = np.arange(1, c.num_users + 1, dtype=np.int32)
                lists = [p.neighbors(int(u)) for u in users]
                pipes[name, k] = (users, lists, np.ones(len(c.test[0]), dtype=bool)) + p.mae(*c.test, True)
            return pipes[name, k]

    return Refs


def _everybody(c):
    return np.arange(1, c.num_users + 1, dtype=np.int32)


def _lists_equal_table(e, table):
    """every list of the table's users: ids, and similarities as bit patterns (the engine's arrays are k wide, the table's
    min(k, U - 1): cells past a row's count hold -1 / nan)"""
    ids, sims, counts = e.neighbors_batch(table.row_user)
    w = table.width
    assert counts.tolist() == [w] * table.rows
    assert (ids[:, w:] == -1).all() and np.isnan(sims[:, w:]).all()
    bad = np.flatnonzero((ids[:, :w] != table.ids).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} of {table.rows} neighbour lists differ, first user {table.row_user[bad[0]]}"
    assert np.array_equal(_bits(sims[:, :w]), _bits(table.sims))


def _compare(kn, e, table, test):
    """the lists of the table's users, and the predictions (bitwise) and the MAE of all their test rows"""
    _lists_equal_table(e, table)
    mask = np.isin(test[0], table.row_user)
    preds = np.full(len(test[0]), np.nan)
    preds[mask] = e.predict_batch(kn.PRED_KNN, test[0][mask], test[1][mask])
    _rows_equal_table(kn, e, table, test, preds)


def _launches(t):
    return t["gemm_launches"], t["select_launches"]


# ---- A: U around the 256 tile --------------------------------------------------------------------------------------------------
def _a_ks(U):
    return (50, U - 2, U - 1, U + 3)


@pytest.mark.parametrize("path", ["symmetric", "one_block", "blocks256", "blocks256_overlap"])
@pytest.mark.parametrize("U", bs.A_USERS)
def test_a_row_tile_edges_cosine(kn, refs, monkeypatch, U, path):
    """U = 255 .. 513 on the symmetric launch (1, 3 or 6 listed tiles), on one row block and on 256-row blocks (a 1 MiB
    workspace; U = 513: three blocks, the last of one row), each a whole-matrix build.  At k >= U - 1 every list holds every
    other user (k = U - 2: all but one): the six private users' rows are 0.0 in every column — and in every padding column of
    U_pad — so a padding column winning the tie, or a real one lost at the panel's edge, shows in their lists."""
    name = f"a{U}"
    c = bs.case(name)
    _symmetric(monkeypatch, path == "symmetric")
    blocked = path.startswith("blocks256")
    e = _engine(kn, c.train, k=K, flags=kn.FLAG_OVERLAP if path.endswith("overlap") else 0, head_items=64,
                workspace_bytes=(1 << 20) if blocked else 0)
    n_tiles = (U + 255) // 256
    blocks = n_tiles if blocked else 1
    tiles_run = n_tiles * (n_tiles + 1) // 2 if path == "symmetric" else n_tiles * n_tiles
    for k in _a_ks(U):
        e.set_k(k)
        e.reset_timings()
        ids, _, counts = e.neighbors_batch(_everybody(c))
        t = _witness(f"A U={U} {path} k={k}", e)
        print(f"[witness] gemm_flops_executed={t['gemm_flops_executed']!r}")
        assert t["fallback_rows"] == 0 and t["head_items"] == 64 and _launches(t) == (blocks, blocks)
        assert t["gemm_flops_executed"] == 2.0 * 256 * 256 * 64 * tiles_run  # (one tile: the two launch forms cost the same)
        assert (counts == min(k, U - 1)).all()
        if k >= U - 1:
            want = [np.delete(np.arange(1, U + 1), u) for u in range(U)]
            assert (ids[:, U - 1:] == -1).all()  # (the arrays are k wide; cells past a row's count hold -1)
            assert np.array_equal(np.sort(ids[:, :U - 1], axis=1), np.asarray(want))
        _compare(kn, e, refs.table(name, k), c.test)
        assert _witness(f"A U={U} {path} k={k}, after the comparison", e)["fallback_rows"] == 0
    e.close()


@pytest.mark.parametrize("U", bs.A_USERS)
def test_a_row_tile_edges_jaccard(kn, refs, monkeypatch, U):
    """the same shapes and k under the Jaccard coefficient (counting GEMM, per-column denominators read from row_len, whose
    padding holds 1.0), symmetric launch"""
    name = f"a{U}"
    c = bs.case(name)
    _symmetric(monkeypatch, True)
    e = _engine(kn, c.train, k=K, sim=kn.SIM_JACCARD, head_items=64)
    for k in _a_ks(U):
        e.set_k(k)
        e.reset_timings()
        e.neighbors_batch(_everybody(c))
        t = _witness(f"A U={U} jaccard k={k}", e)
        assert t["fallback_rows"] == 0 and t["head_items"] == 64 and _launches(t) == (1, 1)
        preds = e.predict_batch(kn.PRED_KNN, c.test[0], c.test[1])
        _equal_pipeline(kn, e, refs.jaccard(name, k), c.test, preds)
        assert e.timings()["fallback_rows"] == 0
    e.close()


# ---- B: head width around 64 and around I ------------------------------------------------------------------------------------------
def _run_b(kn, refs, monkeypatch, name, head, sim):
    c = bs.case(name)
    I = c.num_items
    _symmetric(monkeypatch, True)
    jac = sim == "jaccard"
    e = _engine(kn, c.train, k=K, sim=kn.SIM_JACCARD if jac else kn.SIM_COSINE, head_items=head)
    e.neighbors_batch(_everybody(c))
    t = _witness(f"B {name} head={head:#x} {sim}", e)
    print(f"[witness] tail_pair_updates={t['tail_pair_updates']!r}")
    # head_items = 0 asks the cost model, whose candidates are multiples of 64 cut at I: at I <= 64 the only one is I
    want_head = I if head == 0 else min(head, I)
    assert I <= 64 or head != 0
    assert t["head_items"] == want_head
    assert (t["tail_pair_updates"] > 0) == (want_head < I)
    assert t["fallback_rows"] == 0 and _launches(t) == (1, 1)
    if jac:
        preds = e.predict_batch(kn.PRED_KNN, c.test[0], c.test[1])
        _equal_pipeline(kn, e, refs.jaccard(name, K), c.test, preds)
    else:
        _compare(kn, e, refs.table(name, K), c.test)
    assert e.timings()["fallback_rows"] == 0
    e.close()


@pytest.mark.parametrize("sim", ["cosine", "jaccard"])
@pytest.mark.parametrize("head", [1, 63, 64, 65, 127, 128, 129, 130, HEAD_ALL])
def test_b_head_widths(kn, refs, monkeypatch, head, sim):
    """U = 257, I = 130: K_pad 64 / 128 / 192, a head of one column, a tail of one item (129 = I - 1), no tail at all (I, ALL)"""
    _run_b(kn, refs, monkeypatch, "a257", head, sim)


@pytest.mark.parametrize("sim", ["cosine", "jaccard"])
@pytest.mark.parametrize("head", [HEAD_ALL, 0])
@pytest.mark.parametrize("name", ["b_i64", "b_i40"])
def test_b_few_items(kn, refs, monkeypatch, name, head, sim):
    """I = 64 (K_pad == I exactly) and I = 40 (an operand panel wider than the item set), all items dense"""
    _run_b(kn, refs, monkeypatch, name, head, sim)


# ---- C: U around the 16 384-column tile ----------------------------------------------------------------------------------------------
def _c_users(c):
    U = c.num_users
    return np.unique(np.concatenate([c.groups["edge"], c.groups["edge_item_raters"], _everybody(c)[::(U + 39) // 40]]))


@pytest.mark.parametrize("path", ["symmetric", "row_blocks"])
@pytest.mark.parametrize("U", bs.C_USERS)
def test_c_column_tile_edges(kn, refs, monkeypatch, U, path):
    """U = 16 383 .. 32 769, whole-matrix builds.  The edge users (dense indices 0, 8191, 16 382 .. 16 385, 32 767, 32 768,
    U - 1, those that exist) are each other's nearest neighbours through 12 tail items nobody else rates; one tail item is
    rated by the last cell of tile 0 and the first of tile 1 only, one has every rater in tile 1, one none in tile 0 or 1:
    a rater dropped or counted twice at a tile edge moves an approximate value by far more than the error band."""
    name = f"c{U}"
    c = bs.case(name)
    _symmetric(monkeypatch, path == "symmetric")
    e = _engine(kn, c.train, k=K, head_items=64)
    e.neighbors_batch(_everybody(c))
    t = _witness(f"C U={U} {path}", e)
    assert t["fallback_rows"] == 0 and t["head_items"] == 64 and _launches(t) == (1, 1)
    _compare(kn, e, refs.table(name, K, _c_users(c)), c.test)
    t = _witness(f"C U={U} {path}, after the comparison", e)
    assert t["fallback_rows"] == 0 and _launches(t) == (1, 1)
    e.close()


# ---- D: the MAXT edge -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", bs.D_USERS)
def test_d_register_tile_limit(kn, refs, U):
    """U = 196 608 is 12 tiles — the rater counts of a single-chunk row are held in registers, all 12 slots used — and
    196 609 is 13: the last tile holds one user and every row reads its ranges from the tile table.  A partial build of 48
    users (edge users at dense 0, 16 383, 16 384, 180 223, 180 224, 196 607 and 196 608) through fit_device: one row block
    of one 256-row panel, no U x U panel."""
    import torch

    name = f"d{U}"
    c = bs.case(name)
    dev = torch.device("cuda", 0)
    tr = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in c.train)
    e = kn.Engine(k=K, flags=kn.FLAG_VERIFY_BOUND, head_items=64)
    e.fit_device(*tr)
    assert e.num_users == U
    table = refs.table(name, K, bs.d_sample(c))
    assert table.rows == 48
    _compare(kn, e, table, c.test)
    t = _witness(f"D U={U}, partial build of 48 rows", e)
    assert t["fallback_rows"] == 0 and t["head_items"] == 64 and _launches(t) == (1, 1)
    e.close()


# ---- E: tail entries per row around a chunk ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", bs.E_USERS)
def test_e_tail_entries_per_row(kn, refs, monkeypatch, U):
    """planted rows of exactly 0, 1, 255, 256, 257, 511, 512 and 513 tail entries (0 to 3 chunks; a last chunk of one entry)
    and one of 300 tail entries without a head entry (row_head_sq == 0), in one tile (U = 600) and in two (U = 16 500:
    multi-chunk rows re-read their chunks per tile)"""
    name = f"e{U}"
    c = bs.case(name)
    _symmetric(monkeypatch, True)
    e = _engine(kn, c.train, k=K, head_items=64)
    e.neighbors_batch(_everybody(c))
    t = _witness(f"E U={U}", e)
    assert t["fallback_rows"] == 0 and t["head_items"] == 64 and _launches(t) == (1, 1)
    users = np.unique(np.concatenate([c.groups["planted"], bs.every(c.groups["background"], 20)]))
    _compare(kn, e, refs.table(name, K, users), c.test)
    assert _witness(f"E U={U}, after the comparison", e)["fallback_rows"] == 0
    e.close()


# ---- F: pieces per (chunk, tile) around the table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f1024", "f1025", "f_wide"])
def test_f_pieces_per_chunk(kn, refs, monkeypatch, name):
    """head_items = 4.  f1024: 256 users x 256 tail items, 4 pieces per entry: P = 1024, the last slot of the direct piece ->
    entry table; f1025: one more rater on one item, P = 1025, the binary search; f_wide: 400 x 260, P = 1792 in chunk 0 and a
    4-entry chunk 1 (the premise file mirrors the kernel's piece rule)"""
    c = bs.case(name)
    _symmetric(monkeypatch, True)
    e = _engine(kn, c.train, k=K, head_items=4)
    e.neighbors_batch(_everybody(c))
    t = _witness(f"F {name}", e)
    assert t["fallback_rows"] == 0 and t["head_items"] == 4 and _launches(t) == (1, 1)
    users = np.unique(np.concatenate([c.groups["block"], c.groups.get("extra", c.groups["exact"]), bs.every(c.groups["background"], 10)]))
    _compare(kn, e, refs.table(name, K, users), c.test)
    assert _witness(f"F {name}, after the comparison", e)["fallback_rows"] == 0
    e.close()


# ---- G: build-count edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("n_first", [256, 257])
def test_g_build_counts(kn, refs, monkeypatch, n_first, symmetric):
    """U = 513, a fresh handle with a 1 MiB workspace (256-row blocks): the first n_first users, then the others.  257 users
    switch the longest-row reorder on (`count > 256`) and, where the symmetric launch is allowed, pick it (`count * 2 >= U`):
    one GEMM launch and two select launches, against two and two on the row-block path and one and one for 256 users."""
    U = 513
    c = bs.case("a513")
    _symmetric(monkeypatch, symmetric)
    e = _engine(kn, c.train, k=K, head_items=64, workspace_bytes=1 << 20)

    def expect(n):
        blocks = (n + 255) // 256
        return (1 if symmetric and 2 * n >= U else blocks, blocks)

    first, rest = _everybody(c)[:n_first], _everybody(c)[n_first:]
    e.neighbors_batch(first)
    t1 = _witness(f"G first {n_first} users, symmetric allowed={symmetric}", e)
    assert t1["fallback_rows"] == 0 and _launches(t1) == expect(n_first)
    e.neighbors_batch(rest)
    t2 = _witness(f"G then the other {len(rest)}", e)
    assert t2["fallback_rows"] == 0
    assert (t2["gemm_launches"] - t1["gemm_launches"], t2["select_launches"] - t1["select_launches"]) == expect(len(rest))
    _compare(kn, e, refs.table("a513", K), c.test)
    assert _launches(e.timings()) == _launches(t2)  # (nothing was left to build)
    e.close()


# ---- fold-in queries at the same shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a256", "a257", "c16384", "c16385"])
def test_fold_in_at_tile_edges(kn, oracle, name):
    """the fold-in similarity kernels walk all train rows with U-dependent loops of their own: one new user rates the planted
    edge items (A: the items of the private user at dense index U - 1 — one neighbour, then the 0.0 tie; C: the edge users'
    shared items and the planted tile-edge items), another six popular items"""
    c = bs.case(name)
    U = c.num_users
    e = _engine(kn, c.train, k=K, head_items=64)
    if name.startswith("a"):
        planted = c.items["private"][int(c.groups["private"][1])]
    else:
        planted = np.concatenate([c.items["shared"][:6], [c.items[n] for n in ("pair", "tile1", "tile2") if n in c.items]])
    some = np.unique(c.train[1])[::17]
    for q, its in ((U + 1000, planted), (U + 1001, c.items["popular"])):
        its = np.asarray(its, dtype=np.int32)
        r = np.array([1.0, 4.5, 2.5, 5.0, 3.0, 1.5, 4.0, 2.0, 3.5])[:len(its)]
        _check_fold_in(kn, oracle, e, c.train, q, its, r, oracle.SIM_COSINE, K, np.concatenate([some, its, [999_999]]), ns=(3,))
    assert _witness(f"fold-in {name}", e)["fallback_rows"] == 0
    e.close()
