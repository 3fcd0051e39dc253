"""The fp16 similarity panel of k_gemm_nt_ov against the fp32 panel of k_gemm_nt_bf16 (tests/gemm_panel_check.hip, built here
against the library the way scripts/microbench/gemm_bench.hip is): bit for bit the fp32 sums clamped and rounded to the nearest
even fp16, with clamping on and off; symmetric launches bit-symmetric; at N = 512 the fp32 panel itself within
K * 2^-24 * sum |a||b| of the fp64 product.

Shapes: the widths give 1, 2, 3, 5, 6, 7 and 12 k-tiles (one k-tile per tile, the k-tile requested across the tile end,
both sides of the launcher's switch at six k-steps, fewer k-steps than epilogue units and more); the symmetric sizes give
one diagonal tile, fewer tiles than workgroups, just over one tile per CU and three tiles per workgroup (the hand-over of
the epilogue units and of the operand stream from tile to tile); the row-block form runs one and two tile rows."""
import importlib
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "movie-recommender-system_amd")
WIDTHS = (64, 128, 192, 320, 384, 448, 768)
BF16_WIDTHS = (128, 384)
SYM_N = (256, 768, 5888, 9984)
ROWS_M = (256, 512)
ROWS_N = 9984


@pytest.fixture(scope="module")
def checker(pkg, tmp_path_factory):
    importlib.import_module(pkg.__name__ + ".build").build()
    hipcc = next((c for c in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("gemm_panel") / "gemm_panel_check")
    cmd = [hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(PKG_DIR, "csrc"),
           os.path.join(ROOT, "tests", "gemm_panel_check.hip"), "-L", PKG_DIR, "-lknncf", "-Wl,-rpath," + PKG_DIR, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, form, n, m, k, dtype):
    r = subprocess.run([exe, form, str(n), str(m), str(k), dtype], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, f"{form} N={n} M={m} K={k} {dtype}:\n{r.stdout}\n{r.stderr}"
    assert "FAIL" not in r.stdout
    return r.stdout


@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("n", SYM_N)
def test_symmetric_fp16_operands(checker, n, k):
    out = _run(checker, "sym", n, 0, k, "fp16")
    assert out.count("panel clamp=") == 2 and out.count("mirror clamp=") == 2
    assert ("fp64: ok" in out) == (n <= 512)


@pytest.mark.parametrize("k", BF16_WIDTHS)
@pytest.mark.parametrize("n", SYM_N)
def test_symmetric_bf16_operands(checker, n, k):
    out = _run(checker, "sym", n, 0, k, "bf16")
    assert out.count("panel clamp=") == 2 and out.count("mirror clamp=") == 2


@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("m", ROWS_M)
def test_row_block_fp16_operands(checker, m, k):
    out = _run(checker, "rows", ROWS_N, m, k, "fp16")
    assert out.count("panel clamp=") == 2


@pytest.mark.parametrize("k", BF16_WIDTHS)
@pytest.mark.parametrize("m", ROWS_M)
def test_row_block_bf16_operands(checker, m, k):
    out = _run(checker, "rows", ROWS_N, m, k, "bf16")
    assert out.count("panel clamp=") == 2


@pytest.mark.parametrize("k", WIDTHS)
def test_fp32_reference_against_fp64(checker, k):
    """N = 512: the reference of the checks above is itself within K * 2^-24 * sum |a||b| of the fp64 product."""
    out = _run(checker, "sym", 512, 0, k, "fp16")
    assert "fp64: ok" in out
