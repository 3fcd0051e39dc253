"""knncf_remove_users at the C boundary and in the binding, without a GPU: the symbol is declared, exported and listed in EXPORTS
with the documented argument types; the header has its section behind "Amend", and knncf_amend's own section points to it; a
null handle gets KNNCF_E_INVALID (a handle needs a device, so the other statuses are test_gpu_remove_users.py's); remove_users is
a module-level function of the binding — not a method of Engine or Appends, whose public methods the call-sequence model of the
tests enumerates — and refuses bad shapes and dtypes with ValueError before the library is called."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


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
    assert re.search(r"\bint\s+knncf_remove_users\s*\(", text)
    assert hasattr(kn.load_library(), "knncf_remove_users") and "knncf_remove_users" in kn.EXPORTS
    assert text.index("knncf_amend(") < text.index("knncf_remove_users(")  # behind "Amend"


def test_header_text():
    text = " ".join(_header().replace(" * ", " ").split())
    assert "---- Remove users:" in text
    section = text[text.index("---- Remove users:"):]
    section = section[:section.index("int knncf_remove_users(")]
    for word in ("bit for bit as a handle on which knncf_fit(aug) was called", "knncf_amend given every row of those users", "K = B \\ S",
                 "STORED list holds a leaver", "+0.0 and -0.0 included", "ascending raw id", "Why the lists that hold a leaver are enough",
                 "A leaver without a list is not counted", "Plain refits", "KNNCF_SIM_ONE", "KNNCF_APPEND_MAX_CHANGERS",
                 "fewer than 5 users or fewer than 5 items", "Jaccard carries", "is no user of train", "listed twice", "leaves no row",
                 "Precedence", "n_users == 0 is KNNCF_OK", "KNNCF_AMEND_TILE", "KNNCF_DEBUG_NO_LDS_BITMAPS", "prep_ms",
                 "knncf-dispatch remove users=", "OUT OF SCOPE: a device-pointer form", "the call-sequence model"):
        assert word in section, word
    # knncf_amend's own section keeps its leaver rule and says where the carrying call is
    amend = text[text.index("---- Amend:"):text.index("int knncf_amend(")]
    assert "OUT OF SCOPE: carrying when a user leaves (knncf_remove_users below carries" in amend and "a user leaves the fit" in amend


def test_argtypes(kn):
    lib = kn.load_library()
    assert lib.knncf_remove_users.argtypes == [C.c_void_p, i32p, C.c_int64, i64p, i64p, i32p, C.c_int64]
    assert lib.knncf_remove_users.argtypes[3:] == lib.knncf_append.argtypes[5:]


def test_null_handle(kn):
    u = np.asarray([5, 23], dtype=np.int32)
    a, b = C.c_int64(-7), C.c_int64(-7)
    rc = kn.load_library().knncf_remove_users(None, u.ctypes.data_as(i32p), 2, C.byref(a), C.byref(b), None, 0)
    assert (rc, a.value, b.value) == (kn.E_INVALID, -7, -7)


def test_a_module_level_function(kn):
    assert inspect.isfunction(kn.remove_users)
    sig = inspect.signature(kn.remove_users)
    assert list(sig.parameters) == ["engine", "users", "return_dropped"] and sig.parameters["return_dropped"].default is False
    assert not hasattr(kn.Engine, "remove_users") and not hasattr(kn.Appends, "remove_users")
    assert "call-sequence model" in kn.remove_users.__doc__
    # the classes keep what they had
    assert list(inspect.signature(kn.Appends.amend).parameters) == ["self", "removed_users", "removed_items", "users", "items", "ratings",
                                                                    "return_dropped"]


class _NoLibrary:
    """an engine whose every attribute access fails: the function must refuse before it touches the handle or the library"""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were validated")


def test_it_validates_before_the_library_is_called(kn):
    e = _NoLibrary()
    bad = [
        [[5, 23]],            # 2-D
        [[5], [23, 41]],      # ragged
        5,                    # a scalar
        [5.0, 23.0],          # float ids
        ["5"],                # no numbers
        [2**31],              # past 32 bits
        [-2**31 - 1],
    ]
    for users in bad:
        with pytest.raises(ValueError):
            kn.remove_users(e, users)
        with pytest.raises(ValueError):
            kn.remove_users(e, users, return_dropped=True)
    # good arguments, the empty list included, pass the validation and reach the engine
    for users in ([5], [23, 5], np.asarray([5], dtype=np.int64), []):
        with pytest.raises(AssertionError, match="the engine was touched"):
            kn.remove_users(e, users)
