"""The premises of tests/test_gpu_rerank_pipeline.py, from the data and the oracle alone (no GPU): every row length of
tests/rerank_pipeline_shapes.py puts a full wave's stream where the docstrings say relative to the two stream loops of the
re-rank (rerank.hip: wave_sims).  The loop constants appear here as LITERALS and the trip counts are DERIVED from them by the
loops' own conditions: a product change that moves a constant, or the split between the loops, must fail here instead of
silently turning the GPU tests into ordinary-shape tests.

    p0 = 0
    while p0 + 2 * PIPE <= NPF: trip(full, p0); p0 += PIPE     # steady: every piece consumed or requested is full
    while p0 < NP:              trip(tail, p0); p0 += PIPE     # drain
    (a trip consumes the groups p0 .. p0 + GRP - 1 and p0 + GRP .. p0 + PIPE - 1, both unconditionally, and requests their
    successors; the prologue requests pieces 0 .. PIPE - 1 with the full copies iff PIPE <= NPF)"""
import numpy as np
import pytest

from tests import rerank_pipeline_shapes as ps
from tests import rerank_stream_shapes as rs

PIECE = 64   # rerank.hip: entries per piece of the stream (one per lane)
PIPE = 8     # rerank.hip PIPE: pieces in flight = pieces per trip of either stream loop
GRP = 4      # rerank.hip GRP: pieces consumed at a time; a trip is two groups
WAVES = 8    # waves of a re-rank workgroup; a trip of the shortlist deals up to 64 candidates to each

# L: (steady trips, drain trips, pieces present in the last drain trip's first group, in its second group, prologue takes `full`)
CLAIMS = {
    5: (0, 1, 4, 1, False),   # fewer than PIPE pieces: the steady loop is not entered, one drain trip, three of its pieces absent
    8: (0, 1, 4, 4, True),    # exactly PIPE pieces: the prologue takes `full`, the drain consumes them
    15: (0, 2, 4, 3, True),   # 2 PIPE - 1: one short of a steady trip
    16: (1, 1, 4, 4, True),   # exactly one steady trip, then a drain trip of full pieces
    17: (1, 2, 1, 0, True),   # the last drain trip holds ONE piece: its second group is absent
    24: (2, 1, 4, 4, True),   # two steady trips
}


def _tile_of(k):
    return 512 if k <= 384 else 1024 if k <= 512 else 2048 if k <= 1024 else 4096


def _trips(E):
    """the trips wave_sims makes for a stream of E entries: (steady, drain, pieces of the last drain trip in its first and
    second group, prologue full)"""
    NP, NPF = -(-E // PIECE), E // PIECE
    p0 = steady = drain = 0
    while p0 + 2 * PIPE <= NPF:
        steady += 1
        p0 += PIPE
    last = p0
    while p0 < NP:
        drain += 1
        last = p0
        p0 += PIPE
    g0 = max(0, min(NP - last, GRP))
    g1 = max(0, min(NP - last - GRP, GRP))
    return steady, drain, g0, g1, PIPE <= NPF


def test_constants():
    assert rs.PIECE == PIECE == 64 and PIPE == 2 * GRP == 8
    assert set(CLAIMS) == set(ps.LENGTHS)
    assert ps.KS == (512, 50) and ps.JACCARD == (16, 512) and 16 in ps.LENGTHS


@pytest.mark.parametrize("L", ps.LENGTHS)
def test_full_waves_make_the_claimed_trips(L):
    """64 candidates of L entries: E = 64 L, exactly L pieces, every one full; the trips follow from the constants"""
    E = 64 * L
    assert E % PIECE == 0 and E // PIECE == L
    assert _trips(E) == CLAIMS[L]
    steady, drain, g0, g1, full = CLAIMS[L]
    assert steady * PIPE + (drain - 1) * PIPE + g0 + g1 == L  # every piece is consumed exactly once
    assert drain >= 1  # the steady loop never consumes a stream's last PIPE pieces


def test_the_cases_cover_the_loop_edges():
    steady = {L: CLAIMS[L][0] for L in CLAIMS}
    assert sorted(set(steady.values())) == [0, 1, 2]               # not entered, exactly once, more than once
    assert steady[2 * PIPE - 1] == 0 and steady[2 * PIPE] == 1     # the steady loop's entry condition, both sides
    assert steady[3 * PIPE] == 2 and steady[2 * PIPE + 1] == 1
    assert CLAIMS[PIPE][4] and not CLAIMS[5][4]                     # the prologue's choice, both sides
    assert CLAIMS[2 * PIPE + 1][2:4] == (1, 0)                      # a drain trip with an absent second group
    assert CLAIMS[5][3] == 1 and CLAIMS[15][3] == GRP - 1           # drain groups with absent pieces behind present ones
    assert {CLAIMS[L][1] for L in CLAIMS} == {1, 2}                 # one and two drain trips, with and without a steady loop
    assert CLAIMS[15][:2] == (0, 2) and CLAIMS[17][:2] == (1, 2)


@pytest.mark.parametrize("L", ps.LENGTHS)
def test_uniform_row_lengths(L):
    c = ps.case(L)
    assert c.num_users == rs.UNIFORM_U == 520 and c.num_items == ps.items_of(L) and ps.items_of(L) in (150, 300)
    assert np.array_equal(np.unique(c.train[1]), np.arange(1, c.num_items + 1))
    assert (rs.row_lengths(c) == L).all()
    assert L >= 5  # every row takes the streamed path (rows of <= 4 ratings go to the scalar one)
    assert np.array_equal(np.unique(c.train[0]), np.arange(1, c.num_users + 1))
    assert len(c.test[0]) > 0 and np.isin(c.test[1], c.train[1]).all()


@pytest.fixture(scope="module")
def tables(oracle):
    made = {}

    def get(L, k):
        if (L, k) not in made:
            made[L, k] = oracle.Model(*ps.case(L).train).knn_table(k)
        return made[L, k]

    return get


@pytest.mark.parametrize("L", ps.LENGTHS)
def test_shortlists_fill_the_waves_at_k_512(tables, L):
    """the oracle's lists are 512 long for every user, so every shortlist holds at least WAVES * 64 candidates: the first trip
    of every row deals 64 to each wave (the candidates behind them make a second trip of at most 7 one-candidate waves)"""
    c = ps.case(L)
    t = tables(L, 512)
    assert t.rows == c.num_users and t.width == 512 == WAVES * 64 <= c.num_users - 1
    assert _tile_of(512) == 1024
    rest = c.num_users - 1 - 512
    assert 0 <= rest < WAVES and _trips(L)[:2] == (0, 1)  # those waves stream one row: one drain trip


@pytest.mark.parametrize("L", ps.LENGTHS)
def test_k_50_is_the_benchmarks_tile_with_partial_waves(tables, L):
    """k = 50: TILE = 512, a shortlist of 50 .. 64 candidates gives every wave 7 or 8 (more, and every wave still has fewer
    than 64): streams of 7 L or 8 L entries, one drain trip whose last piece is partial"""
    c = ps.case(L)
    assert _tile_of(50) == 512
    t = tables(L, 50)
    assert t.rows == c.num_users and t.width == 50
    for n in (50, 56, 57, 64):
        assert -(-n // WAVES) in (7, 8)
    for n_c in (7, 8):
        assert -(-n_c * L // PIECE) <= PIPE and _trips(n_c * L)[:2] == (0, 1)  # at most 3 pieces: one drain trip
