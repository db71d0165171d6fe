"""Center / sides extraction (ZAFX_CENTER, ZAFX_CENTER_SIDES) without a GPU: the constants of the C-ABI and their Python mirror, the
geometry that zafx_plan_create rejects before it touches a device, the argument checks of the Python layer, and the kernel's
algorithm -- packed stereo transform, split, mask, re-pack, inverse, overlap-add (zafx_center.hpp + the FFT core, compiled by g++) --
against the reference's own composition of zaf.stft / zaf.istft (tests/golden/center.npz, made by tests/golden/make_center_golden.py),
and on the eleven stereo signals of tests/signals.py against the float64 oracle (test_host_emulation_on_the_stereo_signals)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import signals as sig
from center_oracle import C_CENTER, assert_center_contract, center_figures, oracle_center
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


N_STEREO = 1024 * 9 + 300


@pytest.mark.parametrize("wl", [2048, 256])
def test_host_emulation_on_the_stereo_signals(center_emu, wl):
    """The mask arithmetic where white noise does not take it: the eleven stereo signals of tests/signals.py (0 / 0 in every bin, hard-panned
    tones, a mask of exactly 0.5, a == b in every bin, loud then quiet, a reference that is identically zero) through the float32 emulation
    against oracle_center, N = 1024 * 9 + 300.  Per signal (center_oracle.assert_center_contract): every output finite; silence gives exact
    zeros; center <= 1e-5 normwise -- max|center| <= 1e-5 max|x| where the reference is identically zero (left_only: held to the input's
    level, not skipped); sides <= 1e-5 max|x|; and per hop of H samples per channel
        |out - ref| <= 10 * 1e-5 * max_hop|ref| + C eps32 max|x|,
    the floor on the INPUT's peak.  C = 16 is a measurement: the smallest power of two that leaves this emulation's worst hop at or below
    half the bound over all eleven signals and both windows (the factor two is for the device's 1-ulp v_rcp_f32 and v_sqrt_f32, which the
    emulation replaces by an exact division and std::sqrt).  Measured, emulation against the float64 oracle: the worst hop is left_only at
    W = 2048, 0.353 of the bound with C = 16 (0.707 with C = 8) -- the packed transform of a clip whose right channel is zero leaves the
    split's X_R at round-off level, 5.4e-7 max|x| of center where the reference has none; the next are loud_quiet (0.035 at W = 256) and
    tones_chirp (0.067).  Normwise every signal is below 1.1e-6 (pan_tones at W = 2048), the sides below 1.1e-6 of max|x|.
    Not reached here: the clamp in center_ratio.  It is there for v_rcp_f32, which takes a denormal for zero, and matters only below |X| = 1e-19;
    the emulation divides exactly, so with or without the clamp it gives the same numbers.  The device's clamp is held on the GPU
    (tests/test_gpu_signals.py::test_center_below_the_smallest_normal)."""
    import zafx
    w = zafx.hamming(wl)
    worst = (0.0, "")
    for name in sig.STEREO_NAMES:
        x = sig.stereo_signal(name, N_STEREO)
        assert x.shape == (N_STEREO, 2) and x.dtype == np.float32
        got = _emulate(center_emu, x, w)
        ref = oracle_center(x, w)
        f = assert_center_contract(f"emu W={wl} {name}", got, x - got, x, ref, wl // 2)
        print(f"W={wl} {name}: normwise {f['normwise']:.3e}, sides {f['sides']:.3e} of max|x|, worst hop {f['hop']:.3f} of the bound")
        worst = max(worst, (f["hop"], name))
        if name == "left_only":
            assert not np.any(ref)   # the reference's center is exactly zero: the case that decides C
        if name == "gain":
            assert relerr(ref, 0.5 * np.stack([x[:, 0], x[:, 0]], axis=1).astype(np.float64)) <= 1e-12   # m0 = 0.5, m1 = 1
    # C leaves the emulation half the bound (the other half is the device's rcp / sqrt) and is the smallest power of two that does
    assert C_CENTER == 16.0 and worst[0] <= 0.5, worst
    if wl == 2048:
        x = sig.stereo_signal("left_only", N_STEREO)
        assert center_figures(_emulate(center_emu, x, w), None, x, oracle_center(x, w), wl // 2, c=C_CENTER / 2)["hop"] > 0.5


@pytest.mark.parametrize("wl", [2048, 256])
def test_host_emulation_on_the_stereo_signals_under_a_window_that_is_not_symmetric(center_emu, wl):
    """The same eleven signals, contract and C = 16 under tests/windows.py's `skew` -- periodic Hamming, the only window the center kinds were
    ever given, is one sample short of mirror-symmetric --: the emulation stays at or below half the bound (measured: worst hop 0.464 of it,
    left_only at W = 2048, against 0.353 under Hamming; the next is tones_chirp at 0.116; normwise every signal below 9e-7), so the GPU test of this window (tests/test_gpu_windows.py) runs under the bound as it is."""
    import windows as win
    w = win.skew(wl)
    assert abs(win.cola_gain(w, wl // 2)) >= win.MIN_COLA
    worst = (0.0, "")
    for name in sig.STEREO_NAMES:
        x = sig.stereo_signal(name, N_STEREO)
        got = _emulate(center_emu, x, w)
        f = assert_center_contract(f"emu skew W={wl} {name}", got, x - got, x, oracle_center(x, w), wl // 2)
        print(f"skew W={wl} {name}: normwise {f['normwise']:.3e}, sides {f['sides']:.3e} of max|x|, worst hop {f['hop']:.3f} of the bound")
        worst = max(worst, (f["hop"], name))
    assert C_CENTER == 16.0 and worst[0] <= 0.5, worst


def test_stereo_signals_are_what_the_table_says():
    n = 4096
    assert len(sig.STEREO_NAMES) == 11 and len(set(sig.STEREO_NAMES)) == 11
    s = {name: sig.stereo_signal(name, n) for name in sig.STEREO_NAMES}
    assert all(v.shape == (n, 2) and v.dtype == np.float32 and v.flags.c_contiguous for v in s.values())
    assert not s["silence"].any() and not s["left_only"][:, 1].any()
    assert np.array_equal(s["dc"], np.tile(np.float32([0.5, 0.25]), (n, 1)))
    assert np.array_equal(s["pan_tones"][:, 0], sig.signal("sine_bin", n)) and np.array_equal(s["pan_tones"][:, 1], sig.signal("sine_half", n))
    assert np.array_equal(s["gain"][:, 1], np.float32(0.5) * s["gain"][:, 0]) and np.array_equal(s["gain"][:, 0], sig.signal("sine_half", n))
    assert np.array_equal(s["anti"][:, 1], -s["anti"][:, 0]) and np.array_equal(s["anti"][:, 0], sig.signal("chirp", n))
    assert np.array_equal(s["tones_chirp"][:, 0], sig.signal("two_tones", n)) and np.array_equal(s["tones_chirp"][:, 1], sig.signal("chirp", n))
    assert np.array_equal(s["impulse"][:, 1], np.roll(s["impulse"][:, 0], 3)) and s["impulse"][:, 0].sum() == 4
    lv = [float(np.sqrt(np.mean(s["noise_m90"][:, c].astype(np.float64) ** 2))) for c in (0, 1)]
    assert all(0.9 * 10 ** -4.5 < v < 1.1 * 10 ** -4.5 for v in lv) and not np.array_equal(s["noise_m90"][:, 0], s["noise_m90"][:, 1])
    assert np.array_equal(s["clipped"][:, 0], sig.signal("clipped_pcm", n)) and np.abs(s["clipped"][:, 1]).max() <= 0.7 + 1 / 32768
    assert np.array_equal(s["clipped"][:, 1] * 32768, np.rint(s["clipped"][:, 1] * 32768))
    lq = s["loud_quiet"]
    assert np.array_equal(lq[:, 1], lq[::-1, 0]) and np.abs(lq[:n // 2, 0]).max() > 1 and np.abs(lq[n // 2:, 0]).max() < 2e-4
    assert np.array_equal(s["left_only"][:, 0], sig.signal("chirp", n))
