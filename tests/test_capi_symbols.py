"""The C-ABI shared library loads and exports every symbol include/zafx.h declares
(no compute calls: this runs on machines without a GPU)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "zafx.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(zafx_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    from zafx import _lib
    assert declared_symbols() == sorted(_lib.SYMBOLS)


def test_library_exports_every_declared_symbol(built_library):
    lib = ctypes.CDLL(built_library)
    for name in declared_symbols():
        assert hasattr(lib, name), name
    lib.zafx_version.restype = ctypes.c_int
    assert lib.zafx_version() == 101


def test_compute_units_entry_point_is_declared_bound_and_checks_its_arguments(built_library):
    """zafx_plan_compute_units(plan, in_use, on_device): in the header, in the binding with its three pointers, behind two read-only properties of
    Plan; a null plan is an error with a message, not a crash (no device is needed to say so)."""
    import zafx
    from zafx import _lib
    assert "zafx_plan_compute_units" in declared_symbols()
    res, args = _lib.SYMBOLS["zafx_plan_compute_units"]
    assert res is ctypes.c_int and len(args) == 3
    for name in ("compute_units", "device_compute_units"):
        prop = getattr(zafx.Plan, name)
        assert isinstance(prop, property) and prop.fset is None
    lib = _lib.load()
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.zafx_plan_compute_units(None, ctypes.byref(a), ctypes.byref(b)) != 0
    assert b"null" in lib.zafx_last_error() and (a.value, b.value) == (-1, -1)


def test_live_allocations_entry_point_is_declared_bound_and_needs_no_device(built_library):
    """zafx_plan_live_allocations(count): in the header, in the binding with its one pointer; the count is readable where there is no GPU, and a
    null pointer is an error with a message."""
    from zafx import _lib
    assert "zafx_plan_live_allocations" in declared_symbols()
    res, args = _lib.SYMBOLS["zafx_plan_live_allocations"]
    assert res is ctypes.c_int and len(args) == 1
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    assert lib.zafx_plan_live_allocations(ctypes.byref(n)) == 0 and n.value >= 0
    assert lib.zafx_plan_live_allocations(None) != 0 and b"null" in lib.zafx_last_error()


def test_params_struct_layout(built_library):
    from zafx import _lib
    assert ctypes.sizeof(_lib.ZafxParams) == 16 * 4   # 12 fields + 4 reserved int32


def test_errors_are_reported_not_swallowed(built_library):
    """Without a GPU every entry point that needs one returns a code and a message."""
    from zafx import _lib
    lib = _lib.load()
    n = ctypes.c_int(-1)
    rc = lib.zafx_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    assert rc != 0 or n.value == 0
    if rc != 0:
        assert lib.zafx_last_error()
    bad = _lib.ZafxParams()
    h = ctypes.c_void_p()
    assert lib.zafx_plan_create(ctypes.byref(h), 0, _lib.STFT, ctypes.byref(bad)) != 0   # struct_size mismatch
    assert b"struct_size" in lib.zafx_last_error()


def test_missing_library_fails_loudly():
    """No CPU fallback: a missing libzafx.so is an error, never a silent NumPy path."""
    code = (
        "import os, sys; os.environ['ZAFX_LIBRARY'] = '/nonexistent/libzafx.so';"
        f"sys.path.insert(0, {os.path.join(ROOT, 'zaf-python_amd')!r});"
        "import numpy as np, zafx;\n"
        "try:\n"
        "    zafx.stft(np.zeros(4096, np.float32), zafx.hamming(2048), 1024)\n"
        "except zafx.ZafxError as e:\n"
        "    print('LOUD', e)\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert "LOUD" in out.stdout and "no CPU fallback" in out.stdout, out.stdout + out.stderr


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "zaf-python_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"(from|import)\s+oracle|zaf_oracle|oracle/", text), os.path.join(dirpath, f)
