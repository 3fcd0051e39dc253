"""knncf_recommend_batch at the C boundary and in the binding, without a GPU: the symbol is declared, exported and listed in
EXPORTS, a null handle gets KNNCF_E_INVALID, the chunk rule is written in the header, and Engine.recommend_batch rejects bad
input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "knncf_recommend_batch"


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def test_declared_exported_and_listed(kn):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "knncf.h")).read(), flags=re.S)
    lib = kn.load_library()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", text)
    assert hasattr(lib, NAME)
    assert NAME in kn.EXPORTS


def test_chunk_rule_and_state_are_documented():
    text = open(os.path.join(ROOT, "include", "knncf.h")).read()
    assert "min(1024, budget / (96 * num_items), (2^31 - 1) / num_items)" in text and "workspace_bytes / 2" in text
    assert re.search(r"STATE\s+THAT\s+knncf_neighbors_batch\s+OVER\s+THE\s+SAME\s+users\s+LEAVES", text)


def test_null_handle(kn):
    lib = kn.load_library()
    us = np.array([5, 6], dtype=np.int32)
    items = np.empty(6, dtype=np.int32)
    preds = np.empty(6, dtype=np.float64)
    cnt = np.zeros(2, dtype=np.int32)
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    assert lib.knncf_recommend_batch(None, kn.PRED_KNN, p(us, i32p), 2, 3, p(items, i32p), p(preds, f64p), p(cnt, i32p)) == kn.E_INVALID


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return e


@pytest.mark.parametrize("users,n", [
    ([1.5, 2.0], 3),          # non-integer users
    ([1, 2**31], 3),          # beyond int32
    ([-2**31 - 1], 3),
    ([[1, 2], [3, 4]], 3),    # 2-D
    (7, 3),                   # 0-D
    (["a"], 3),
    ([1, 2], -1),
    ([1, 2], 2.0),
    ([1, 2], True),
    ([1, 2], 2**31),
])
def test_wrapper_rejects_bad_input(engine, kn, users, n):
    with pytest.raises(ValueError):
        engine.recommend_batch(kn.PRED_KNN, users, n)
