"""knncf_append at the C boundary and in the binding, without a GPU: the symbol is declared, exported and listed in EXPORTS with
the documented argument types; the header has its section and the constant KNNCF_APPEND_MAX_CHANGERS, which the binding exports
with the same value; a null handle gets KNNCF_E_INVALID; Appends.append — a class of its own beside Engine, as the entered and bystander families
have — rejects ragged input before any C call."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def kn(pkg):
    importlib.import_module(pkg.__name__ + ".build").build()
    mod = importlib.import_module(pkg.__name__ + ".knncf")
    mod.load_library()
    return mod


def _header():
    return open(os.path.join(ROOT, "include", "knncf.h")).read()


def test_declared_exported_and_listed(kn):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+knncf_append\s*\(", text)
    assert hasattr(kn.load_library(), "knncf_append") and "knncf_append" in kn.EXPORTS


def test_the_constant(kn):
    m = re.search(r"^#define\s+KNNCF_APPEND_MAX_CHANGERS\s+(\d+)\s*$", _header(), flags=re.M)
    assert m and kn.APPEND_MAX_CHANGERS == int(m.group(1))
    n = kn.APPEND_MAX_CHANGERS
    assert n >= 1 and n & (n - 1) == 0  # a power of two (DESIGN.md "Append": half the measured crossover, rounded down)


def test_header_text():
    text = " ".join(_header().replace(" * ", " ").split())
    assert "---- Append:" in text
    section = text[text.index("---- Append:"):]
    section = section[:section.index("int knncf_append(")]
    for word in ("bit for bit as a handle on which knncf_fit(aug) was called", "K = B \\ S", "knncf_update_entered_batch reports",
                 "ascending raw id", "Why S is enough", "Plain refits", "KNNCF_APPEND_MAX_CHANGERS", "KNNCF_E_DUPLICATE",
                 "KNNCF_E_NONFINITE", "SECOND copy", "n == 0", "prep_ms", "OUT OF SCOPE: removals"):
        assert word in section, word


def test_argtypes_and_signature(kn):
    lib = kn.load_library()
    assert lib.knncf_append.argtypes == [C.c_void_p, i32p, i32p, f64p, C.c_int64, i64p, i64p, i32p, C.c_int64]
    assert lib.knncf_append.argtypes[:5] == lib.knncf_fit.argtypes  # the rows as knncf_fit takes them
    sig = inspect.signature(kn.Appends.append)
    assert inspect.isfunction(kn.Appends.append)
    assert list(sig.parameters) == ["self", "users", "items", "ratings", "return_dropped"]
    assert sig.parameters["return_dropped"].default is False
    # the call is not an Engine method: Engine's methods are the calls that the call-sequence model of the suite replays
    assert not hasattr(kn.Engine, "append")


def test_null_handle(kn):
    lib = kn.load_library()
    u = np.array([5, 5], dtype=np.int32)
    i = np.array([1, 2], dtype=np.int32)
    r = np.array([3.0, 4.0])
    a, b = C.c_int64(-7), C.c_int64(-7)
    p = lambda x, t: x.ctypes.data_as(t)
    assert lib.knncf_append(None, p(u, i32p), p(i, i32p), p(r, f64p), 2, C.byref(a), C.byref(b), None, 0) == kn.E_INVALID
    assert (a.value, b.value) == (-7, -7)


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"C entry point {name} called with bad arguments")


@pytest.fixture
def engine(kn):
    e = kn.Engine.__new__(kn.Engine)  # no device: every C call would fail loudly
    e._lib, e._h, e.k, e.device = _NoCalls(), None, 10, 0
    return kn.Appends(e)


@pytest.mark.parametrize("rows", [
    ([5, 5], [1, 2], [3.0]),          # lengths differ
    ([5], [1, 2], [3.0, 4.0]),
    ([[5]], [[1]], [[3.0]]),          # 2-D
    ([5.5], [1], [3.0]),              # non-integer user
    ([2**31], [1], [3.0]),            # user beyond int32
    ([5], [1.5], [3.0]),              # non-integer item
    ([5], [1], ["x"]),                # a rating that is no number
])
def test_the_wrapper_rejects_ragged_input(engine, rows):
    with pytest.raises(ValueError):
        engine.append(*rows)


def test_no_rows_reach_the_library(engine):
    """n == 0 is a valid call (it reports |B|): the wrapper passes it on"""
    with pytest.raises(AssertionError, match="knncf_append"):
        engine.append([], [], [])
