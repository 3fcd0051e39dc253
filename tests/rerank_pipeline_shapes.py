"""Uniform-row rating sets that put a wave's candidate stream on the edges of the re-rank's two stream loops (numpy only).

wave_sims (rerank.hip) consumes a stream of NP 64-entry pieces in trips of PIPE = 8 pieces: a STEADY loop while every piece a
trip consumes or requests is full (p0 + 2 PIPE <= NPF), then a DRAIN loop for the rest.  With every row L long and 64 candidates
in a wave, the stream is exactly L pieces, all of them full (tests/rerank_stream_shapes.py: uniform_rows), so L alone picks the
trip counts of both loops.  tests/test_rerank_pipeline_premises.py derives them from the loop constants;
tests/test_gpu_rerank_pipeline.py pins every case to the oracle."""
import functools

from tests import rerank_stream_shapes as rs

LENGTHS = (5, 8, 15, 16, 17, 24)
KS = (512, 50)         # TILE 1024 with full waves of 64 candidates; TILE 512 (the benchmark's instantiation), 7 or 8 per wave
JACCARD = (16, 512)    # (L, k) of the one Jaccard run


def items_of(L):
    """I = 300 as in the uniform cases of rerank_stream_shapes; 150 for the two shortest rows, whose 520 L ratings leave some of
    300 skewed items unrated (the conventions want raw item ids exactly 1..I)"""
    return rs.UNIFORM_I if L >= 15 else 150


@functools.lru_cache(maxsize=None)
def case(L):
    """U = 520, every row exactly L long (computed once, shared and left unchanged)"""
    return rs.uniform_rows(L, I=items_of(L))
