"""The re-rank's two stream loops at their edges, against the oracle bit for bit.

wave_sims (rerank.hip) consumes a wave's candidate stream in trips of 8 pieces: a steady loop while every piece a trip consumes
or requests is full, then a drain loop.  The cases of tests/test_gpu_rerank_stream.py put 63 .. 65 pieces in a stream — seven
steady trips and one drain trip, always.  Here every row is L long, so a full wave of 64 candidates streams exactly L pieces:

    L =  5   steady loop not entered; one drain trip with three absent pieces; the prologue takes the tail copies
    L =  8   steady loop not entered; one drain trip; the prologue takes the full copies
    L = 15   steady loop not entered; two drain trips
    L = 16   exactly one steady trip, one drain trip
    L = 17   one steady trip, two drain trips: the last holds one piece, its second group is absent
    L = 24   two steady trips, one drain trip

each at k = 512 (TILE = 1024, the first trip of a row deals 64 candidates to every wave) and at k = 50 (TILE = 512, the
benchmark's instantiation; 7 or 8 candidates per wave: a short drain with a partial last piece), L = 16 once with Jaccard.
tests/test_rerank_pipeline_premises.py derives the trip counts from the loop constants and proves the rest from the data and
the oracle.

Bars (those of tests/test_gpu_rerank_stream.py): neighbour ids equal, fp64 similarities and predictions equal as bit patterns
for every user, |dMAE| <= 1e-9, no row off the ordinary path (fallback_rows == 0), and the `rerank TILE=...` dispatch line."""
import importlib

import numpy as np
import pytest

from tests import rerank_pipeline_shapes as ps
from tests.test_gpu_boundary_shapes import _compare, _everybody
from tests.test_gpu_degenerate_rows import _engine, _equal_pipeline, _symmetric, _witness
from tests.test_gpu_rerank_stream import TRACE, _rerank_lines, _tile_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def refs(oracle):
    """the oracle's answers, each computed once and left unchanged"""
    models, tables = {}, {}

    class Refs:
        @staticmethod
        def model(L):
            if L not in models:
                models[L] = oracle.Model(*ps.case(L).train)
            return models[L]

        @staticmethod
        def table(L, k):
            if (L, k) not in tables:
                tables[L, k] = Refs.model(L).knn_table(k)
            return tables[L, k]

        @staticmethod
        def jaccard(L, k, users):
            test = ps.case(L).test
            p = Refs.model(L).pipeline(oracle.SIM_JACCARD, k)
            lists = [p.neighbors(int(u)) for u in users]
            mask = np.isin(test[0], users)
            return (users, lists, mask) + p.mae(*(a[mask] for a in test), True)

    return Refs


@pytest.mark.parametrize("k", ps.KS)
@pytest.mark.parametrize("L", ps.LENGTHS)
def test_stream_loop_edges(kn, refs, monkeypatch, capfd, L, k):
    c = ps.case(L)
    monkeypatch.setenv(TRACE, "1")
    monkeypatch.delenv("KNNCF_DEBUG_SLICE_ROWS", raising=False)
    _symmetric(monkeypatch, True)
    e = _engine(kn, c.train, k=k)
    capfd.readouterr()
    e.neighbors_batch(_everybody(c))
    lines = _rerank_lines(capfd)
    t = _witness(f"L={L} k={k}", e)
    print(f"[witness] dispatch: {lines}")
    assert t["fallback_rows"] == 0
    assert lines and set(lines) == {f"rerank TILE={_tile_of(k)} jaccard=0"}
    _compare(kn, e, refs.table(L, k), c.test)
    assert _witness(f"L={L} k={k}, after the comparison", e)["fallback_rows"] == 0
    e.close()


def test_one_steady_trip_jaccard(kn, refs, monkeypatch, capfd):
    """L = 16 at k = 512 with every hit counting 1.0: one steady and one drain trip of the Jaccard instantiation, against the
    oracle's per-pair closures for every 13th user"""
    L, k = ps.JACCARD
    c = ps.case(L)
    users = _everybody(c)[::13]
    monkeypatch.setenv(TRACE, "1")
    monkeypatch.delenv("KNNCF_DEBUG_SLICE_ROWS", raising=False)
    _symmetric(monkeypatch, True)
    e = _engine(kn, c.train, k=k, sim=kn.SIM_JACCARD)
    capfd.readouterr()
    e.neighbors_batch(_everybody(c))
    lines = _rerank_lines(capfd)
    t = _witness(f"L={L} jaccard k={k}", e)
    print(f"[witness] dispatch: {lines}")
    assert t["fallback_rows"] == 0
    assert lines and set(lines) == {f"rerank TILE={_tile_of(k)} jaccard=1"}
    preds = e.predict_batch(kn.PRED_KNN, c.test[0], c.test[1])
    _equal_pipeline(kn, e, refs.jaccard(L, k, users), c.test, preds)
    assert e.timings()["fallback_rows"] == 0
    e.close()
