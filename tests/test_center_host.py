"""Center / sides extraction (ZAFX_CENTER, ZAFX_CENTER_SIDES) without a GPU: the constants of the C-ABI and their Python mirror, the
geometry that zafx_plan_create rejects before it touches a device, the argument checks of the Python layer, and the kernel's
algorithm -- packed stereo transform, split, mask, re-pack, inverse, overlap-add (zafx_center.hpp + the FFT core, compiled by g++) --
against the reference's own composition of zaf.stft / zaf.istft (tests/golden/center.npz, made by tests/golden/make_center_golden.py)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, relerr

TOL_FFT = 1e-5   # the project's normwise bound for a float32 transform chain against the float64 reference


def _cases():
    g = np.load(os.path.join(GOLDEN, "center.npz"))
    for i in range(len([k for k in g.files if k.startswith("w")])):
        wl, n = (int(v) for v in g[f"w{i}"])
        yield wl, n, g[f"x{i}"], g[f"c{i}"]


def test_fixture_cases():
    got = {(wl, n) for wl, n, _, _ in _cases()}
    assert {(2048, 22050), (1024, 7168), (512, 7000), (256, 1)} <= got
    for wl, n, x, c in _cases():
        assert x.dtype == np.float32 and x.shape == (n, 2) and c.dtype == np.float64 and c.shape == (n, 2)
        assert np.isfinite(c).all()


def test_constants_in_header_and_binding():
    from zafx import _lib
    header = open(os.path.join(ROOT, "include", "zafx.h")).read()
    assert re.search(r"\bZAFX_CENTER\s*=\s*11\b", header) and re.search(r"\bZAFX_CENTER_SIDES\s*=\s*12\b", header)
    assert "zaf.py:155-198" in header
    assert (_lib.CENTER, _lib.CENTER_SIDES) == (11, 12)
    import zafx
    assert (zafx.CENTER, zafx.CENTER_SIDES) == (11, 12)


def _create(built_library, kind, **fields):
    from zafx import _lib
    lib = _lib.load()
    prm = _lib.ZafxParams()
    prm.struct_size = ctypes.sizeof(_lib.ZafxParams)
    prm.window_length, prm.step_length = 2048, 1024
    for k, v in fields.items():
        setattr(prm, k, v)
    h = ctypes.c_void_p()
    rc = lib.zafx_plan_create(ctypes.byref(h), 0, kind, ctypes.byref(prm))
    msg = (lib.zafx_last_error() or b"").decode()
    if rc == 0:
        lib.zafx_plan_destroy(h)
    return rc, msg


@pytest.mark.parametrize("fields, names", [
    (dict(step_length=512), "step_length"),
    (dict(window_length=4096, step_length=2048), "window_length"),
    (dict(window_length=128, step_length=64), "window_length"),
    (dict(window_length=1000, step_length=500), "window_length"),
    (dict(precision=1), "precision"),
    (dict(struct_size=60), "struct_size"),
])
@pytest.mark.parametrize("kind", [11, 12])
def test_plan_creation_rejects_geometry_without_a_device(built_library, kind, fields, names):
    rc, msg = _create(built_library, kind, **fields)
    assert rc != 0 and names in msg, (rc, msg)


def test_argument_validation_before_the_library_is_loaded(monkeypatch):
    import zafx
    from zafx import _lib

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    w = zafx.hamming(1024)
    with pytest.raises(ValueError):
        zafx.centersides_batch(np.zeros((3, 4000), np.float32), w)
    with pytest.raises(ValueError):
        zafx.centersides_batch(np.zeros((3, 4000, 3), np.float32), w)
    with pytest.raises(ValueError, match="step_length"):
        zafx.centersides_batch(np.zeros((3, 4000, 2), np.float32), w, step_length=256)
    with pytest.raises(ValueError):
        zafx.centersides(np.zeros(4000), w, 512)
    with pytest.raises(ValueError, match="step_length"):
        zafx.centersides(np.zeros((4000, 2)), w, 256)
    with pytest.raises(ValueError, match="window_length"):
        zafx.centersides_batch(np.zeros((1, 9000, 2), np.float32), zafx.hamming(4096))


@pytest.fixture(scope="module")
def center_emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("center_emu") / "center_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-DZAFX_HOST_EMU", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "center_emu.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _emulate(exe, x, w):
    payload = struct.pack("ii", len(w), x.shape[0]) + np.asarray(w, np.float32).tobytes() + np.ascontiguousarray(x, np.float32).tobytes()
    res = subprocess.run([exe], input=payload, capture_output=True, check=True)
    return np.frombuffer(res.stdout, np.float32).reshape(x.shape)


def test_host_emulation_matches_the_reference(center_emu):
    import zafx
    for wl, n, x, c in _cases():
        got = _emulate(center_emu, x, zafx.hamming(wl))
        err = relerr(got.astype(np.float64), c)
        print(f"W={wl} N={n}: normwise error {err:.3e}")
        assert err <= TOL_FFT, (wl, n, err)


def test_host_emulation_special_signals(center_emu):
    """Silence gives zeros (the mask's 0 / 0 departure: no NaN); L == R is all center; R = 0 has no center."""
    import zafx
    w, n = zafx.hamming(512), 3000
    assert not _emulate(center_emu, np.zeros((n, 2), np.float32), w).any()
    s = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    both = _emulate(center_emu, np.stack([s, s], axis=1), w)
    assert relerr(both, np.stack([s, s], axis=1)) <= TOL_FFT
    left = _emulate(center_emu, np.stack([s, np.zeros_like(s)], axis=1), w)
    assert np.isfinite(left).all() and np.abs(left).max() <= TOL_FFT * np.abs(s).max()
