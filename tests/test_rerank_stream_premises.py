"""The premises of tests/test_gpu_rerank_stream.py, from the data and the oracle alone (no GPU): every case of
tests/rerank_stream_shapes.py is what it claims to be relative to the fixed sizes of the re-rank's candidate stream.  Those
sizes appear here as LITERALS: a product change that moves one of them must fail here, visibly, instead of silently turning the
GPU tests into ordinary-shape tests.

The stream's bookkeeping (rerank.hip: wave_sims) has NO window: the start mask of a piece is built from a scalar walk whose
state is two numbers (candidates started, next start), whatever the distance to the next boundary.  WINDOW_PIECES is
therefore 0, and the giant case is measured against the pipeline depth and a whole trip instead."""
import numpy as np
import pytest

from tests import rerank_stream_shapes as rs

PIECE = 64           # rerank.hip: entries per piece of the stream (one per lane)
PIPE = 8             # rerank.hip PIPE: pieces in flight = pieces per trip of the stream loop
GRP = 4              # rerank.hip GRP: pieces consumed at a time
WINDOW_PIECES = 0    # pieces covered by one refill of the bookkeeping (0: there is no window)
UPRE_LDS_512 = 512   # RerankPlan<512>::UPRE_LDS: longer rows of u take the global-upre instantiation
WAVES = 8            # waves of a re-rank workgroup; a trip deals up to 64 candidates to each
WBUF = {512: 336, 1024: 512}  # products per wave buffer: RerankPlan<512, WIDE> (these item counts fit three workgroups), RerankPlan<1024>

UNIFORM = {"all63": 63, "all64": 64, "all65": 65, "all5": 5}
# (case, k) of the GPU tests and the shortlist tile launch_rerank picks for it: kcap <= 384 -> 512, <= 512 -> 1024
RUNS = {("all63", 512): 1024, ("all64", 512): 1024, ("all65", 512): 1024, ("all64", 50): 512, ("all63", 50): 512,
        ("all65", 50): 512, ("all5", 50): 512, ("giant", 299): 512, ("clones", 199): 512, ("clones400", 399): 1024}


def _tile_of(k):
    return 512 if k <= 384 else 1024 if k <= 512 else 2048 if k <= 1024 else 4096


@pytest.fixture(scope="module")
def model(oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = oracle.Model(*rs.case(name).train)
        return made[name]

    return get


@pytest.mark.parametrize("name", list(rs._CASES))
def test_conventions(name):
    c = rs.case(name)
    U, I = c.num_users, c.num_items
    assert rs.PIECE == PIECE
    for cols in (c.train, c.test):
        assert cols[0].dtype == np.int32 and cols[1].dtype == np.int32 and cols[2].dtype == np.float64
        assert np.array_equal(2 * cols[2], np.round(2 * cols[2])) and cols[2].min() >= 1.0 and cols[2].max() <= 5.0
    assert np.array_equal(np.unique(c.train[0]), np.arange(1, U + 1))
    assert np.array_equal(np.unique(c.train[1]), np.arange(1, I + 1))
    n = rs.row_lengths(c)
    assert n.min() >= 5  # every row takes the streamed path (rows of <= 4 ratings go to the scalar one)
    pairs = np.concatenate([c.train[0], c.test[0]]).astype(np.int64) * (1 << 32) + np.concatenate([c.train[1], c.test[1]])
    assert len(np.unique(pairs)) == len(pairs)
    lo, hi = np.full(U + 1, 9.0), np.zeros(U + 1)
    np.minimum.at(lo, c.train[0], c.train[2])
    np.maximum.at(hi, c.train[0], c.train[2])
    assert (lo[1:] < hi[1:]).all()
    assert np.isin(c.test[1], c.train[1]).all() and len(c.test[0]) > 0


@pytest.mark.parametrize("name", list(UNIFORM))
def test_uniform_row_lengths(name):
    """every row is exactly L long: candidate j of any wave starts at stream position j * L, whoever the candidates are"""
    c = rs.case(name)
    L = UNIFORM[name]
    assert (rs.row_lengths(c) == L).all()
    starts = np.arange(64) * L
    lanes = starts % PIECE
    if L == 64:
        assert (lanes == 0).all()  # every first entry at lane 0, every last at lane 63, E a multiple of 64
    elif L in (63, 65):
        assert len(np.unique(lanes)) == 64  # the boundary visits every lane position within one wave's 64 candidates
    else:
        per_piece = np.bincount(starts[:13] // PIECE)
        assert per_piece.max() == 13 and (64 // L) in (12, 13)  # 12-13 boundaries in one piece


def test_uniform_cases_fill_the_waves(model):
    """U - 1 = 519 >= 512: at k = 512 the first trip of every row deals 64 candidates to each of the 8 waves; at k = 50 a
    shortlist of 50 .. 64 candidates gives every wave 7 or 8"""
    c = rs.case("all64")
    assert c.num_users - 1 >= WAVES * 64 == 512
    for n in (50, 56, 57, 64):
        per = -(-n // WAVES)
        assert per in (7, 8)


def test_giant(model):
    c = rs.case("giant")
    n = rs.row_lengths(c)
    assert c.groups["giant"].tolist() == [1] and n[0] == 3000
    pieces = -(-3000 // PIECE)
    assert pieces == 47 and pieces > PIPE and pieces > WINDOW_PIECES and pieces > 5 * PIPE  # more than five whole trips
    assert n[0] > UPRE_LDS_512  # the giant's own row: the global-upre instantiation
    heavy = n[c.groups["heavy"] - 1]
    assert len(heavy) == 20 and heavy.min() >= 513 and heavy.max() <= 700 and heavy.min() > UPRE_LDS_512
    light = n[c.groups["light"] - 1]
    assert light.min() >= 5 and light.max() <= 70 and len(light) == c.num_users - 21
    # the rows overlap: the giant shares items with (nearly) every light user, so its row produces hits all along
    its = c.train[1][c.train[0] != 1]
    assert np.isin(its, np.arange(1, 3001)).mean() > 0.9
    assert model("giant").knn_table(299).width == 299 == c.num_users - 1


@pytest.mark.parametrize("name,n_clones", [("clones", 100), ("clones400", 300)])
def test_clones(model, name, n_clones):
    """(the stored lists are min(k, U - 1) long, and that length picks the tile: the 200-user case cannot reach the 1024 tile
    whatever k is, so a second case of 400 users does)"""
    c = rs.case(name)
    k = c.num_users - 1
    u, it = c.train[0], c.train[1]
    shared = np.arange(1, 65)
    for x in c.groups["clones"]:
        assert np.array_equal(np.sort(it[u == x]), shared)  # the clone sets are identical: every streamed entry is a hit
    seen = set(shared.tolist())
    for x in c.groups["disjoint"]:
        mine = set(it[u == x].tolist())
        assert len(mine) == 8 and not (mine & seen)  # pairwise disjoint, and disjoint from the clones' items: no entry is a hit
        seen |= mine
    assert len(c.groups["clones"]) == n_clones and len(c.groups["disjoint"]) == 100
    assert _tile_of(min(k, c.num_users - 1)) == (512 if n_clones == 100 else 1024) and _tile_of(min(400, 199)) == 512
    # a group of GRP all-hit pieces adds GRP * 64 products: as many as the fold rule reserves, in either buffer
    assert GRP * PIECE == 256 and all(w >= 256 for w in WBUF.values())
    assert 256 + 256 > WBUF[512]   # TILE = 512: a fold in front of every group that follows an all-hit group
    assert 256 + 256 == WBUF[1024]  # TILE = 1024: two all-hit groups fill the buffer to its last slot, then the fold
    ratings = {x: tuple(c.train[2][u == x][np.argsort(it[u == x])]) for x in c.groups["clones"]}
    assert len(set(ratings.values())) == n_clones  # differing ratings
    t = model(name).knn_table(k)
    assert t.width == k
    # the oracle agrees: a disjoint user's similarities are all exactly 0.0, a clone's with the disjoint block too
    row = {int(x): r for r, x in enumerate(t.row_user)}
    d0 = int(c.groups["disjoint"][0])
    assert (t.sims[row[d0]] == 0.0).all()
    c0 = int(c.groups["clones"][0])
    zero = t.ids[row[c0]][t.sims[row[c0]] == 0.0]
    assert np.isin(c.groups["disjoint"], zero).all()


@pytest.mark.parametrize("name,k", list(RUNS))
def test_list_widths_and_tiles(model, name, k):
    c = rs.case(name)
    assert _tile_of(k) == RUNS[name, k]
    t = model(name).knn_table(k)
    assert t.width == min(k, c.num_users - 1) and t.rows == c.num_users
