"""knncf_mae_sweep / knncf_mae_sweep_device: declared, exported and bound (no GPU needed)."""
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("knncf_mae_sweep", "knncf_mae_sweep_device")


def test_sweep_symbols_declared_exported_and_bound(pkg):
    text = open(os.path.join(ROOT, "include", "knncf.h")).read()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), f"{n} not declared in include/knncf.h"
    importlib.import_module(pkg.__name__ + ".build").build()
    kn = importlib.import_module(pkg.__name__ + ".knncf")
    lib = kn.load_library()
    for n in NAMES:
        assert hasattr(lib, n) and n in kn.EXPORTS
        assert getattr(lib, n).argtypes is not None, f"{n} has no argtypes"
    assert callable(getattr(kn.Engine, "mae_sweep", None))
    assert callable(getattr(kn.Engine, "mae_sweep_device", None))


def test_header_cites_the_reference_entry_point():
    text = open(os.path.join(ROOT, "include", "knncf.h")).read()
    i = text.index("knncf_mae_sweep(")
    assert "predict/kNN.scala:73" in text[max(0, i - 2500):i]
