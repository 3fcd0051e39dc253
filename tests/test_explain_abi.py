"""knncf_explain* at the C boundary and in the binding, without a GPU: the three symbols are declared, exported and listed in
EXPORTS, the order constants exist on both sides, the ctypes signatures are the header's, a null handle gets KNNCF_E_INVALID,
the chunk rule and the out-of-scope note are written in the header, and the wrappers reject bad input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_explain", "knncf_explain_batch", "knncf_explain_batch_device")


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _header(comments=False):
    text = open(os.path.join(ROOT, "include", "knncf.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_listed(kn, name):
    assert re.search(r"\bint\s+" + name + r"\s*\(", _header())
    assert hasattr(kn.load_library(), name)
    assert name in kn.EXPORTS


def test_constants(kn):
    text = _header()
    assert re.search(r"#define\s+KNNCF_EXPLAIN_SUM_ORDER\s+0\b", text) and re.search(r"#define\s+KNNCF_EXPLAIN_BY_WEIGHT\s+1\b", text)
    assert (kn.EXPLAIN_SUM_ORDER, kn.EXPLAIN_BY_WEIGHT) == (0, 1)


def _ctype_of(param, device):
    """the ctypes type of one parameter of the header's declaration"""
    param = " ".join(param.split())
    if "knncf_handle*" in param:
        return C.c_void_p
    if "*" in param:
        if device:
            return C.c_void_p
        return C.POINTER({"int32_t": C.c_int32, "double": C.c_double}[param.replace("const ", "").split("*")[0].strip()])
    return {"int32_t": C.c_int32, "int64_t": C.c_int64}[param.split()[0]]


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_signature_is_the_headers(kn, name):
    decl = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S).group(1)
    want = [_ctype_of(p, name.endswith("_device")) for p in decl.split(",")]
    assert len(want) == {"knncf_explain": 11}.get(name, 12)
    assert list(getattr(kn.load_library(), name).argtypes) == want


def test_chunk_rule_state_and_scope_are_documented():
    text = _header(comments=True)
    assert "C = max(1, budget / (20 * cap + 28))" in text and "workspace_bytes / 2" in text
    assert re.search(r"STATE\s+THAT\s+knncf_predict_batch\s+OVER\s+THE\s+SAME\s+ROWS\s+LEAVES", text)
    assert re.search(r"SHARDED\s+EXPLANATIONS\s+ARE\s+OUT\s+OF\s+SCOPE", text)


def test_null_handle(kn):
    lib = kn.load_library()
    us, its = np.array([5, 6], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    raters, sims, devs = np.empty(6, dtype=np.int32), np.empty(6), np.empty(6)
    cnt, sums, preds = np.zeros(2, dtype=np.int32), np.zeros(4), np.zeros(2)
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    out = (p(raters, i32p), p(sims, f64p), p(devs, f64p), p(cnt, i32p), p(sums, f64p), p(preds, f64p))
    assert lib.knncf_explain_batch(None, p(us, i32p), p(its, i32p), 2, 0, 3, *out) == kn.E_INVALID
    assert lib.knncf_explain(None, 5, 1, 0, 3, *out) == kn.E_INVALID
    assert lib.knncf_explain_batch_device(None, None, None, 2, 0, 3, None, None, None, None, None, None) == kn.E_INVALID


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return e


@pytest.mark.parametrize("cap,order", [(-1, 0), (2.0, 0), (True, 0), (2**31, 0), (4, 2), (4, -1), (4, None)])
def test_wrappers_reject_bad_input(engine, cap, order):
    with pytest.raises(ValueError):
        engine.explain_batch([1, 2], [3, 4], cap, order=order)
    with pytest.raises(ValueError):
        engine.explain(1, 3, cap=cap, order=order)


def test_batch_wrapper_rejects_ragged_rows(engine):
    with pytest.raises(ValueError):
        engine.explain_batch([1, 2], [3], 4)
    with pytest.raises(ValueError):
        engine.explain_batch([[1, 2]], [[3, 4]], 4)
