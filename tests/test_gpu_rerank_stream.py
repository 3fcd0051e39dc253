"""The re-rank's candidate stream at the places where it changes candidate, against the oracle bit for bit.

k_rerank reads the rows of a wave's candidates as one stream of 64-entry pieces and finds each entry's candidate from a
per-piece start mask (rerank.hip: wave_sims).  tests/rerank_stream_shapes.py makes the row lengths uniform — the only way to
pin a boundary to a lane, since the order of a shortlist depends on atomics in select: boundaries on every piece edge (all64),
drifting through every lane (all63, all65), a dozen per piece (all5) — and adds one candidate of 47 pieces (giant) and rows
where every entry or no entry is a hit (clones).  tests/test_rerank_stream_premises.py proves from the data and the oracle
alone that every case is what it claims to be.

Bars (those of tests/test_gpu_boundary_shapes.py): neighbour ids equal, fp64 similarities and predictions equal as bit
patterns, |dMAE| <= 1e-9.  Each test prints its path witnesses before asserting them; no case may leave the ordinary path
(fallback_rows == 0), and each asserts the `rerank TILE=...` dispatch line it intends."""
import importlib

import numpy as np
import pytest

from tests import rerank_stream_shapes as rs
from tests.test_gpu_boundary_shapes import _compare, _everybody
from tests.test_gpu_degenerate_rows import _engine, _equal_pipeline, _symmetric, _witness

pytestmark = pytest.mark.gpu
TRACE = "KNNCF_DEBUG_TRACE_DISPATCH"


@pytest.fixture(scope="module")
def kn(pkg):
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def refs(oracle):
    """the oracle's answers, each computed once and left unchanged: the model of a case, its bulk kNN table (cosine) of
    everybody, and the per-pair closures' lists and predictions (Jaccard) of a set of users"""
    models, tables, pipes = {}, {}, {}

    class Refs:
        @staticmethod
        def model(name):
            if name not in models:
                models[name] = oracle.Model(*rs.case(name).train)
            return models[name]

        @staticmethod
        def table(name, k):
            if (name, k) not in tables:
                tables[name, k] = Refs.model(name).knn_table(k)
            return tables[name, k]

        @staticmethod
        def jaccard(name, k, users):
            if (name, k) not in pipes:
                test = rs.case(name).test
                p = Refs.model(name).pipeline(oracle.SIM_JACCARD, k)
                lists = [p.neighbors(int(u)) for u in users]
                mask = np.isin(test[0], users)
                pipes[name, k] = (users, lists, mask) + p.mae(*(a[mask] for a in test), True)
            return pipes[name, k]

    return Refs


def _tile_of(k):
    return 512 if k <= 384 else 1024 if k <= 512 else 2048 if k <= 1024 else 4096


def _rerank_lines(capfd):
    return [ln[len("knncf-dispatch "):] for ln in capfd.readouterr().err.splitlines() if ln.startswith("knncf-dispatch rerank")]


def _run_cosine(kn, refs, monkeypatch, capfd, name, k, flags=0, sliced=False):
    c = rs.case(name)
    monkeypatch.setenv(TRACE, "1")
    if sliced:
        monkeypatch.setenv("KNNCF_DEBUG_SLICE_ROWS", "100000")
    else:
        monkeypatch.delenv("KNNCF_DEBUG_SLICE_ROWS", raising=False)
    _symmetric(monkeypatch, True)
    e = _engine(kn, c.train, k=k, flags=flags)
    capfd.readouterr()
    e.neighbors_batch(_everybody(c))
    lines = _rerank_lines(capfd)
    t = _witness(f"{name} k={k} flags={flags} sliced={sliced}", e)
    print(f"[witness] dispatch: {lines}")
    assert t["fallback_rows"] == 0
    assert lines and set(lines) == {f"rerank TILE={_tile_of(k)} jaccard=0"}
    _compare(kn, e, refs.table(name, k), c.test)
    assert _witness(f"{name} k={k}, after the comparison", e)["fallback_rows"] == 0
    e.close()


def _run_jaccard(kn, refs, monkeypatch, capfd, name, k, users):
    c = rs.case(name)
    monkeypatch.setenv(TRACE, "1")
    monkeypatch.delenv("KNNCF_DEBUG_SLICE_ROWS", raising=False)
    _symmetric(monkeypatch, True)
    e = _engine(kn, c.train, k=k, sim=kn.SIM_JACCARD)
    capfd.readouterr()
    e.neighbors_batch(_everybody(c))
    lines = _rerank_lines(capfd)
    t = _witness(f"{name} jaccard k={k}", e)
    print(f"[witness] dispatch: {lines}")
    assert t["fallback_rows"] == 0
    assert lines and set(lines) == {f"rerank TILE={_tile_of(k)} jaccard=1"}
    preds = e.predict_batch(kn.PRED_KNN, c.test[0], c.test[1])
    _equal_pipeline(kn, e, refs.jaccard(name, k, users), c.test, preds)
    assert e.timings()["fallback_rows"] == 0
    e.close()


@pytest.mark.parametrize("k", [512, 50])
@pytest.mark.parametrize("name", ["all64", "all63", "all65"])
def test_uniform_rows(kn, refs, monkeypatch, capfd, name, k):
    """U = 520, I = 300, every row 63 / 64 / 65 long.  k = 512 (TILE = 1024): the first trip deals 64 candidates to every
    wave — 64 boundaries on piece edges (all64: first entry at lane 0, last at lane 63, E a multiple of 64) or one lane
    further per candidate, through all 64 lanes (all63 backwards, all65 forwards).  k = 50 (TILE = 512): 7 or 8 per wave."""
    _run_cosine(kn, refs, monkeypatch, capfd, name, k)


def test_many_boundaries_per_piece(kn, refs, monkeypatch, capfd):
    """U = 300, I = 40, every row exactly 5 long, k = 50: 12 or 13 candidates start in one piece, and a wave's whole stream is
    one piece (7 or 8 candidates: 35 or 40 entries) — the lanes behind it carry no entry"""
    _run_cosine(kn, refs, monkeypatch, capfd, "all5", 50)


@pytest.mark.parametrize("sliced", [False, True])
def test_giant_candidate(kn, refs, monkeypatch, capfd, sliced):
    """U = 300, I = 3200, k = U - 1: one candidate of 3000 entries spans 47 pieces — nearly six trips of the stream loop
    without a boundary — between candidates of 5 .. 700; the giant's own row (and the twenty of 513 .. 700) is longer than
    UPRE_LDS and takes the global-upre instantiation.  sliced: every row as slices (KNNCF_DEBUG_SLICE_ROWS)."""
    _run_cosine(kn, refs, monkeypatch, capfd, "giant", 299, sliced=sliced)


@pytest.mark.parametrize("name", ["clones", "clones400"])
def test_all_hits_and_no_hits(kn, refs, monkeypatch, capfd, name):
    """100 (300) clones over the same 64 items, 100 users with 8 private items each, k = U - 1.  A clone's row against the clone
    block: every streamed entry is a hit, every group adds 256 products (U = 200, lists of 199, TILE = 512: a fold in front of
    every group; U = 400, lists of 399, TILE = 1024: two groups fill the 512-product buffer to its last slot — the list length
    min(k, U - 1) picks the tile, so 200 users cannot reach that one).  Against the disjoint block no entry is a hit: the
    product offsets of consecutive candidates coincide.  Rows of the disjoint users are 0.0 everywhere: the oracle's order
    decides."""
    _run_cosine(kn, refs, monkeypatch, capfd, name, rs.case(name).num_users - 1)


def test_bf16_filter_wider_shortlists(kn, refs, monkeypatch, capfd):
    """all65 at k = 50 with bf16 filter operands: the wider error band lengthens the shortlists (more candidates per wave)"""
    _run_cosine(kn, refs, monkeypatch, capfd, "all65", 50, flags=kn.FLAG_BF16_FILTER)


@pytest.mark.parametrize("name,k", [("all64", 512), ("giant", 299)])
def test_jaccard(kn, refs, monkeypatch, capfd, name, k):
    """the same streams with every hit counting 1.0 (the fold yields the number of common items): all64 at k = 512 and the
    giant at k = U - 1, against the oracle's per-pair closures for a spread of users (the giant and the heavy ones among them)"""
    c = rs.case(name)
    users = _everybody(c)[::13] if name == "all64" else np.unique(np.concatenate([[1], c.groups["heavy"][::4], c.groups["light"][::11]])).astype(np.int32)
    _run_jaccard(kn, refs, monkeypatch, capfd, name, k, users)
