"""The premises of tests/test_gpu_boundary_shapes.py, from the data and the oracle alone (no GPU): every case of
tests/boundary_shapes.py sits where it claims to sit relative to the fixed sizes of the neighbour build.  Those sizes appear
here as LITERALS: a product change that moves one of them must fail here, visibly, instead of silently turning the GPU tests
into ordinary-shape tests.

One premise of the plan could not be met as written: a user's dense index is not its raw id minus one but the rank of its id
in HashSet iteration order, also when the ids are exactly 1..U.  The planted edge users are therefore placed BY DENSE INDEX
(boundary_shapes.users_by_dense, checked against the oracle's order below): "the users with raw ids 16384 and 16385" of the
plan are the users at dense indices 16383 and 16384 — the last cell of tile 0 and the first of tile 1, the edge they stood for."""
import numpy as np
import pytest

from tests import boundary_shapes as bs

ROW_TILE = 256        # api.cpp U_pad = round_up(U, 256), gemm.hip's 256 x 256 tile, R rows per block, `count > 256` reorder
K_PAD = 64            # api.cpp K_pad = round_up(head, 64)
SELECT_TCOLS = 16384  # engine.h SELECT_TCOLS
MAXT = 12             # select.hip MAXT
EMAX = 256            # select.hip EMAX
PMAX = 1024           # select.hip PMAX
K = bs.K


def _round_up(x, m):
    return (x + m - 1) // m * m


@pytest.fixture(scope="module")
def model(oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = oracle.Model(*bs.case(name).train)
        return made[name]

    return get


def _tail_head_counts(c, user, head):
    """(tail entries, head entries) of the row of raw user `user` at head width `head`"""
    mine = c.train[1][c.train[0] == user]
    in_head = np.isin(mine, bs.head_items(c.train, head))
    return int((~in_head).sum()), int(in_head.sum())


def _head_is_unambiguous(c, head):
    """the head-th and the (head + 1)-th most rated items differ in their counts: the head set does not hang on a tie"""
    counts = np.sort(np.unique(c.train[1], return_counts=True)[1])[::-1]
    return counts[head - 1] > counts[head]


# ---- conventions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bs.CASES))
def test_conventions(name):
    c = bs.case(name)
    U, I = c.num_users, c.num_items
    assert bs.TILE == SELECT_TCOLS
    for cols in (c.train, c.test):
        assert cols[0].dtype == np.int32 and cols[1].dtype == np.int32 and cols[2].dtype == np.float64
        assert np.array_equal(2 * cols[2], np.round(2 * cols[2])) and cols[2].min() >= 1.0 and cols[2].max() <= 5.0
    assert np.array_equal(np.unique(c.train[0]), np.arange(1, U + 1))
    assert np.array_equal(np.unique(c.train[1]), np.arange(1, I + 1))
    n = np.bincount(c.train[0], minlength=U + 1)[1:]
    assert n.min() >= 5
    pairs = np.concatenate([c.train[0], c.test[0]]).astype(np.int64) * (1 << 32) + np.concatenate([c.train[1], c.test[1]])
    assert len(np.unique(pairs)) == len(pairs)
    # scale(x, mean) is 0 only at a mean of exactly 1 or 5, i.e. a constant user; no row has a zero norm either
    mean = np.bincount(c.train[0], weights=c.train[2], minlength=U + 1)[1:] / n
    assert mean.min() > 1.0 and mean.max() < 5.0
    planted = [g for g in c.groups if g not in ("background", "edge_item_raters", "extra")]
    for g in planted:  # every planted user has a test row on a rated item
        assert np.isin(c.groups[g], c.test[0]).all(), (name, g)
    assert not np.array_equal(c.train[0], np.sort(c.train[0]))  # shuffled


def test_generators_are_deterministic():
    for name in ("a513", "c16385", "e600", "f1025"):
        a, b = bs.CASES[name](), bs.CASES[name]()
        for x, y in zip(a.train + a.test, b.train + b.test):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["a257", "a513", "c16385", "e600"])
def test_dense_order_is_the_oracles(model, name):
    c = bs.case(name)
    assert np.array_equal(model(name).user_iteration_order(), bs.users_by_dense(c.num_users))


def test_dense_order_at_the_largest_shape(oracle):
    U = 196609
    assert oracle.int_set_order(np.arange(1, U + 1)) == bs.users_by_dense(U).tolist()
    assert not np.array_equal(bs.users_by_dense(U), np.arange(1, U + 1))  # (dense index is NOT id - 1)


# ---- A, G: the 256-row tile ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", bs.A_USERS)
def test_a_shapes_and_private_users(model, oracle, U):
    c = bs.case(f"a{U}")
    assert c.num_users == U and c.num_items == 130
    assert {255: 1, 256: 1, 257: 2, 511: 2, 512: 2, 513: 3}[U] == _round_up(U, ROW_TILE) // ROW_TILE
    private = c.groups["private"]
    dense = bs.dense_of(U)[private]
    assert len(private) == 6 and {0, U - 1} <= set(dense.tolist())
    assert {d for d in (255, 256, 511, 512) if d < U} <= set(dense.tolist())  # both sides of every tile edge that exists
    # nobody else rates a private user's items: 5 tail entries, no head entry, at any head width below I - 29
    for x in private:
        its = c.items["private"][int(x)]
        assert np.array_equal(np.sort(c.train[1][c.train[0] == x]), its)
        assert (c.train[0][np.isin(c.train[1], its)] == x).all()
        assert _tail_head_counts(c, x, 64) == (5, 0)
    # ... so, from the oracle alone: similarity exactly 0.0 with EVERY other user, cosine (bulk form) and Jaccard (per pair)
    t = model(f"a{U}").knn_table(U + 3, users=private)
    assert t.width == U - 1 and t.rows == 6  # kcap = U - 1 for k >= U - 1 (and U - 2 at k = U - 2: one user of the tie is cut)
    assert (t.sims == 0.0).all() and not np.signbit(t.sims).any()
    m = model(f"a{U}")
    others = np.arange(1, U + 1)[::9]
    assert all(m.fresh_similarity(oracle.SIM_JACCARD, int(private[0]), int(v)) == 0.0 for v in others if v != private[0])
    # background rows are ordinary: positive at rank 50
    assert (m.knn_table(K, users=bs.every(c.groups["background"], 10)).sims[:, K - 1] > 0.0).all()


def test_a_row_blocks_and_g_counts():
    U = 513
    blocks = [min(ROW_TILE, U - r) for r in range(0, U, ROW_TILE)]
    assert blocks == [256, 256, 1]  # the last row block of the 256-row launches holds one row
    # G: the reorder test is `count > 256`, the symmetric launch's `count * 2 >= U`: both flip between 256 and 257 users
    assert not 256 > ROW_TILE and 257 > ROW_TILE
    assert 256 * 2 < U <= 257 * 2
    assert (U - 256) * 2 >= U and (U - 257) * 2 < U  # the builds of the remaining users take the other path each


# ---- B: head widths ----------------------------------------------------------------------------------------------------------------
def test_b_head_widths():
    I = bs.case("a257").num_items
    assert I == 130
    heads = [1, 63, 64, 65, 127, 128, 129, I - 1, I]
    assert [_round_up(h, K_PAD) for h in heads] == [64, 64, 64, 128, 128, 128, 192, 192, 192]
    assert bs.case("b_i64").num_items == 64 == K_PAD and bs.case("b_i40").num_items == 40 < K_PAD
    assert bs.case("b_i64").num_users == 257 and bs.case("b_i40").num_users == 257


# ---- C, D: the 16 384-column tile and the 12 register-held tiles ---------------------------------------------------------------------
def _check_edge_case(c, m, edge_dense, edge_items, n_tiles):
    U = c.num_users
    dense = bs.dense_of(U)
    assert (U + SELECT_TCOLS - 1) // SELECT_TCOLS == n_tiles
    edge = c.groups["edge"]
    assert dense[edge].tolist() == [d for d in dict.fromkeys(edge_dense) if d < U] and len(edge) >= 3
    assert _head_is_unambiguous(c, 64)
    head = bs.head_items(c.train, 64)
    assert np.isin(c.items["popular"][:3], head).all() and not np.isin(c.items["shared"], head).any()
    # the planted items: exactly the named raters, by dense index and tile; all of them tail items
    rated = {}
    for name, ds in edge_items.items():
        want = [d for d in ds if d < U]
        assert (name in c.items) == bool(want)
        if want:
            got = np.sort(dense[c.train[0][c.train[1] == c.items[name]]])
            assert got.tolist() == want and c.items[name] not in head
            rated[name] = (got // SELECT_TCOLS).tolist()
    raters = np.unique(c.train[0][np.isin(c.train[1], c.items["shared"])])
    assert np.array_equal(raters, np.sort(edge))
    # an edge row: 3 head entries, the 12 shared tail entries and the planted items it rates
    for x in edge:
        n_extra = sum(int(x) in c.train[0][c.train[1] == c.items[name]] for name in rated)
        assert _tail_head_counts(c, x, 64) == (12 + n_extra, 3)
    # from the oracle alone: the edge users are in each other's top 10
    t = m.knn_table(10, users=edge)
    for row, x in enumerate(t.row_user):
        assert np.isin(edge[edge != x], t.ids[row]).all(), x
    return rated


@pytest.mark.parametrize("U", bs.C_USERS)
def test_c_edge_users_and_items(model, U):
    c = bs.case(f"c{U}")
    assert c.num_items == 400
    rated = _check_edge_case(c, model(f"c{U}"), bs.C_EDGE + (U - 1,), bs.C_ITEMS, {16383: 1, 16384: 1, 16385: 2, 32768: 2, 32769: 3}[U])
    want = {16383: {}, 16384: {"pair": [0]}, 16385: {"pair": [0, 1], "tile1": [1]},
            32768: {"pair": [0, 1], "tile1": [1, 1, 1, 1]}, 32769: {"pair": [0, 1], "tile1": [1, 1, 1, 1], "tile2": [2]}}[U]
    assert rated == want
    assert np.isin(c.groups["edge_item_raters"], c.groups["background"]).all()
    assert len(c.groups["edge_item_raters"]) == (2 if U >= 32768 else 0)


@pytest.mark.parametrize("U", bs.D_USERS)
def test_d_edge_users_and_items(oracle, U):
    c = bs.case(f"d{U}")
    n_tiles = {196608: 12, 196609: 13}[U]
    assert (n_tiles <= MAXT) == (U == 196608)  # one tile more and the rater counts no longer fit the registers
    rated = _check_edge_case(c, oracle.Model(*c.train), bs.D_EDGE, bs.D_ITEMS, n_tiles)
    assert rated == {"pair": [0, 1], "last": [11, 11] + ([12] if U == 196609 else [])}
    sample = bs.d_sample(c)
    assert len(sample) == len(np.unique(sample)) == 48 and np.isin(c.groups["edge"], sample).all()
    assert 48 * 2 < U and 48 <= ROW_TILE  # a partial build: one row block of one 256-row panel
    assert np.isin(c.groups["edge"], c.test[0]).all() and np.isin(sample, c.test[0]).sum() >= 40


# ---- E: tail entries per row around a chunk --------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", bs.E_USERS)
def test_e_tail_entries_per_row(U):
    c = bs.case(f"e{U}")
    assert c.num_items == 700 and (U + SELECT_TCOLS - 1) // SELECT_TCOLS == {600: 1, 16500: 2}[U]
    counts = np.bincount(c.train[1], minlength=701)
    assert counts[1:65].min() > counts[65:].max() and _head_is_unambiguous(c, 64)  # the head is exactly the hot items
    assert np.array_equal(np.sort(bs.head_items(c.train, 64)), np.arange(1, 65))
    got = [_tail_head_counts(c, x, 64) for x in c.groups["planted"]]
    assert got == [(n, 10) for n in (0, 1, 255, 256, 257, 511, 512, 513)] + [(300, 0)]
    assert got == [c.items["entries"][int(x)] for x in c.groups["planted"]]
    chunks = [(n + EMAX - 1) // EMAX for n, _ in got]
    assert chunks == [0, 1, 1, 1, 2, 2, 2, 3, 2]
    # background rows stay inside one chunk
    bg_tail = np.bincount(c.train[0][c.train[1] > 64], minlength=U + 1)[c.groups["background"]]
    assert 0 < bg_tail.max() < EMAX


# ---- F: pieces per (chunk, tile) around the table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,want", [("f1024", [[1024]]), ("f1025", [[1025]]), ("f_wide", [[256 * 7], [4 * 7]])])
def test_f_pieces_per_chunk_and_tile(name, want):
    c = bs.case(name)
    assert c.num_users == 1000
    assert _head_is_unambiguous(c, 4) and np.array_equal(np.sort(bs.head_items(c.train, 4)), [1, 2, 3, 4])
    x = int(c.groups["exact"][0])
    P = bs.pieces_per_chunk_and_tile(c.train, x, 4)
    assert P == want
    assert (P[0][0] <= PMAX) == (name == "f1024")  # the last slot of the direct table / the first binary search
    assert _tail_head_counts(c, x, 4)[0] == len(c.items["block"])
    # the block items are rated by the block users and by nobody else (f1025: by one background user more, on one item)
    n_raters = np.bincount(c.train[1], minlength=c.num_items + 1)[c.items["block"]]
    extra = np.zeros(len(n_raters), dtype=int)
    extra[0] = name == "f1025"
    assert np.array_equal(n_raters, len(c.groups["block"]) + extra)
    if name == "f1025":
        a, b = bs.case("f1024"), c
        assert len(b.train[0]) == len(a.train[0]) + 1  # the same fit with one more rating
    # other block users carry three ordinary tail items: two chunks, the second of 3 entries
    longer = [int(u) for u in c.groups["block"][2:7:2]]
    assert all(_tail_head_counts(c, u, 4)[0] == len(c.items["block"]) + 3 for u in longer)
