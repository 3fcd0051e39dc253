"""knncf_amend at the C boundary and in the binding, without a GPU: the symbol is declared, exported and listed in EXPORTS with
the documented argument types — the removals in front of knncf_append's arguments; the header has its section and the constant
KNNCF_AMEND_TILE, which the binding exports with the same value; a null handle gets KNNCF_E_INVALID (a handle needs a device, so
KNNCF_E_STATE before a fit is test_gpu_amend.py's); Appends.append stays what it was and Appends.amend beside it refuses bad
shapes and dtypes with ValueError before the library is called."""
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
    assert re.search(r"\bint\s+knncf_amend\s*\(", text)
    assert hasattr(kn.load_library(), "knncf_amend") and "knncf_amend" in kn.EXPORTS
    assert text.index("knncf_append(") < text.index("knncf_amend(")  # after "Append"


def test_the_tile_constant(kn):
    m = re.search(r"^#define\s+KNNCF_AMEND_TILE\s+(\d+)\s*$", _header(), flags=re.M)
    assert m and kn.AMEND_TILE == int(m.group(1))
    t = kn.AMEND_TILE
    assert t % 256 == 0 and t // 64 <= 64  # whole passes of a 256-thread workgroup; one wave scans a tile's bitmap words


def test_header_text():
    text = " ".join(_header().replace(" * ", " ").split())
    assert "---- Amend:" in text
    section = text[text.index("---- Amend:"):]
    section = section[:section.index("int knncf_amend(")]
    for word in ("bit for bit as a handle on which knncf_fit(aug) was called", "K = B \\ S", "knncf_revise_entered_batch reports",
                 "ascending raw id", "Why S is still enough", "A re-rating is a removal plus a row", "leaves the fit: num_items shrinks",
                 "leaves the fit: num_users shrinks", "Plain refits", "a user leaves the fit", "Jaccard carries",
                 "KNNCF_APPEND_MAX_CHANGERS", "is not a train row", "listed twice", "an aug without any row", "KNNCF_E_DUPLICATE",
                 "KNNCF_E_NONFINITE", "Precedence", "n_removed == 0 && n == 0", "knncf_append is the call without removals",
                 "KNNCF_AMEND_TILE", "prep_ms", "knncf-dispatch amend removers=", "OUT OF SCOPE: carrying when a user leaves"):
        assert word in section, word
    # knncf_append's own section still says that it takes no removals, and now where they go
    append = text[text.index("---- Append:"):text.index("int knncf_append(")]
    assert "OUT OF SCOPE: removals (knncf_amend below takes them)" in append


def test_argtypes_and_signature(kn):
    lib = kn.load_library()
    assert lib.knncf_amend.argtypes == [C.c_void_p, i32p, i32p, C.c_int64, i32p, i32p, f64p, C.c_int64, i64p, i64p, i32p, C.c_int64]
    assert lib.knncf_amend.argtypes[4:] == lib.knncf_append.argtypes[1:]
    assert list(inspect.signature(kn.Appends.append).parameters) == ["self", "users", "items", "ratings", "return_dropped"]
    assert not hasattr(kn.Engine, "amend")


def _call(lib, h, removals, rows):
    ru, ri = (np.ascontiguousarray(a, dtype=np.int32) for a in removals)
    u, i, r = (np.ascontiguousarray(a, dtype=t) for a, t in zip(rows, (np.int32, np.int32, np.float64)))
    a, b = C.c_int64(-7), C.c_int64(-7)
    p = lambda x, t: x.ctypes.data_as(t)
    rc = lib.knncf_amend(h, p(ru, i32p), p(ri, i32p), len(ru), p(u, i32p), p(i, i32p), p(r, f64p), len(u), C.byref(a), C.byref(b), None, 0)
    return rc, a.value, b.value


def test_null_handle(kn):
    assert _call(kn.load_library(), None, ([5], [1]), ([5, 5], [1, 2], [3.0, 4.0])) == (kn.E_INVALID, -7, -7)


class _NoLibrary:
    """an engine whose every attribute access fails: the method must refuse before it touches the handle or the library"""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were validated")


def test_the_method_validates_before_the_library_is_called(kn):
    assert list(inspect.signature(kn.Appends.amend).parameters) == ["self", "removed_users", "removed_items", "users", "items", "ratings",
                                                                    "return_dropped"]
    assert inspect.signature(kn.Appends.amend).parameters["return_dropped"].default is False
    a = kn.Appends(_NoLibrary())
    good = ([5], [1], [5, 5], [1, 2], [3.0, 4.0])
    bad = [
        ([5, 6], [1]) + good[2:],                                   # removals of two lengths
        ([[5]], [[1]]) + good[2:],                                  # 2-D removals
        ([5.0], [1]) + good[2:],                                    # float ids
        ([5], [2**31]) + good[2:],                                  # an id past 32 bits
        ([5], [-2**31 - 1]) + good[2:],
        good[:2] + ([5, 5], [1], [3.0, 4.0]),                       # rows of two lengths
        good[:2] + ([5, 5], [1, 2], [3.0]),
        good[:2] + ([[5, 5]], [[1, 2]], [[3.0, 4.0]]),              # 2-D rows
        good[:2] + ([5, 5], [1.5, 2], [3.0, 4.0]),                  # float ids
        good[:2] + ([2**31, 5], [1, 2], [3.0, 4.0]),
        good[:2] + ([5, 5], [1, 2], ["3", "4"]),                    # ratings that are no numbers
        good[:2] + (5, 1, 3.0),                                     # scalars
    ]
    for args in bad:
        with pytest.raises(ValueError):
            a.amend(*args)
        with pytest.raises(ValueError):
            a.amend(*args, return_dropped=True)
    # the same checks as append's on the rows
    for args in bad[5:]:
        with pytest.raises(ValueError):
            a.append(*args[2:])
    # good arguments, empty parts included, pass the validation and reach the engine
    for args in (good, ([], []) + good[2:], good[:2] + ([], [], []), ([], [], [], [], [])):
        with pytest.raises(AssertionError, match="the engine was touched"):
            a.amend(*args)
