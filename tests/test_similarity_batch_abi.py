"""knncf_similarity_batch, knncf_similarity_batch_device and knncf_knn_similarity_batch at the C boundary and in the binding,
without a GPU: the symbols are declared, exported and listed in EXPORTS, a null handle gets KNNCF_E_INVALID, the chunk rule
and the handle-state sentence are written in the header, and the Engine wrappers reject bad input before any C call."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_similarity_batch", "knncf_similarity_batch_device", "knncf_knn_similarity_batch")


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_listed(kn, name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "knncf.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert hasattr(kn.load_library(), name)
    assert name in kn.EXPORTS


def test_chunk_rule_and_state_are_documented():
    text = open(os.path.join(ROOT, "include", "knncf.h")).read()
    section = text[text.index("Bulk similarities"):]
    section = section[:section.index("knncf_knn_similarity_batch(")]
    assert "budget / 16" in section and "workspace_bytes / 2" in section
    assert re.search(r"STATE\s+THAT\s+knncf_neighbors_batch\s+OVER", section)
    assert "closure of its OWN" in section and "no device form" in section


@pytest.mark.parametrize("name", NAMES)
def test_null_handle(kn, name):
    lib = kn.load_library()
    us, vs = np.array([5, 6], dtype=np.int32), np.array([6, 5], dtype=np.int32)
    out = np.full(2, 7.0)
    if name.endswith("_device"):  # (never dereferenced: the handle is checked first)
        args = (C.c_void_p(us.ctypes.data), C.c_void_p(vs.ctypes.data), 2, C.c_void_p(out.ctypes.data))
    else:
        i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        args = (us.ctypes.data_as(i32p), vs.ctypes.data_as(i32p), 2, out.ctypes.data_as(f64p))
    assert getattr(lib, name)(None, *args) == kn.E_INVALID
    assert out.tolist() == [7.0, 7.0]


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return e


BAD_PAIRS = [
    ([1.5, 2.0], [1, 2]),         # non-integer ids
    ([1, 2], [1.0, 2.0]),
    ([1, 2**31], [1, 2]),         # beyond int32
    ([1, 2], [-2**31 - 1, 2]),
    ([[1, 2], [3, 4]], [1, 2]),   # 2-D
    ([1, 2], [[1, 2]]),
    (7, 3),                       # 0-D
    (["a"], [1]),
    ([1, 2], [1]),                # lengths differ
    ([], [1]),
]


@pytest.mark.parametrize("method", ["similarity_batch", "knn_similarity_batch"])
@pytest.mark.parametrize("us,vs", BAD_PAIRS)
def test_wrapper_rejects_bad_input(engine, method, us, vs):
    with pytest.raises(ValueError):
        getattr(engine, method)(us, vs)


def test_device_wrapper_rejects_bad_input(engine):
    import torch

    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64)
    for us, vs, out in [
        (np.zeros(2, np.int32), i32(2), f64(2)),          # not a tensor
        (i32(2).long(), i32(2), f64(2)),                  # int64 ids
        (i32(2), i32(2), f64(2).float()),                 # float32 out
        (i32(2), i32(3), f64(2)),                         # lengths differ
        (i32(2), i32(2), f64(3)),
        (i32(4).reshape(2, 2), i32(4).reshape(2, 2), f64(4)),  # 2-D
        (i32(2), i32(2), f64(2)),                         # host tensors
    ]:
        with pytest.raises(ValueError):
            engine.similarity_batch_device(us, vs, out)
