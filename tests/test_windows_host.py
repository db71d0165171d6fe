"""Windows that are not mirror-symmetric (tests/windows.py: skew, signed, random), without a GPU.

KBD and the sine window -- the only windows any mdct / imdct test used to be given -- satisfy w[n] == w[W-1-n] exactly, and the MDCT kernels are
built around that mirror: a tap of the sign-folded table taken at its mirror position (zafx_wfold.hpp), or a mirrored tap in the inverse's unfold,
is invisible under them.  This module holds what the GPU tests of tests/test_gpu_windows.py rest on:
  * the oracle equals the REAL reference on these windows (tests/golden/windows.npz, made by tests/golden/make_windows_golden.py);
  * each recipe discriminates: the oracle's result moves by at least 5 % when the window is mirrored, at every geometry the GPU module uses
    (measured: the smallest is 0.086, `signed` at W = 256 through the STFT;
    where W - 1 is a multiple of 3 its sign pattern is its own mirror image and only its ramp tells the two apart) -- and by exactly 0 under KBD and the sine window, the gap being closed;
  * every (window, W, hop) the ISTFT and center tests use has a COLA sum zaf.istft can divide by;
  * the suite's float32 tolerances apply unchanged: the reference MDCT restated in float32 is as far from the oracle under the new windows as
    under KBD (within a factor 2 at every W);
  * the fold table the forward MDCT kernels read, with their fold and tap pairing restated in double, gives the direct MDCT on these windows
    (tests/host_emu/mdct_fold_emu.cpp on zafx_wfold.hpp).
"""
import os
import struct
import subprocess

import numpy as np
import pytest
import scipy.fft

import windows as win
from conftest import GOLDEN, ROOT, relerr, synth_clip
from oracle import zaf_oracle as orc

def _f32_exact(make):
    return lambda wl: make(wl).astype(np.float32).astype(np.float64)


# KBD and sine as the kernels are handed them, rounded to float32: exactly mirror-symmetric (in float64 the sine window's two halves differ by an ulp)
SYMMETRIC = {"kbd": _f32_exact(orc.kbd_window), "sine": _f32_exact(orc.sine_window)}


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "windows.npz"))


# ---------------------------------------------------------------------------------------------------------------- the recipes
@pytest.mark.parametrize("name", win.NAMES)
def test_recipes_are_float32_exact_and_not_symmetric(name):
    for wl in (64, 256, 1000, 2048, 8192):
        w = win.window(name, wl)
        assert w.dtype == np.float64 and w.shape == (wl,) and np.array_equal(w, w.astype(np.float32).astype(np.float64))
        assert np.array_equal(w, win.window(name, wl)) and np.abs(w).max() <= 1.0
        assert np.abs(w - w[::-1]).max() >= 0.05, (name, wl)   # far from its mirror image, not by a rounding
    assert (win.skew(2048) > 0).all() and np.argmax(win.skew(2048)) < 1024 - 100
    s = win.signed(2048)
    assert (s < 0).sum() == len(range(0, 2048, 3)) and np.abs(s[:1024]).mean() > 1.05 * np.abs(s[1024:]).mean()
    assert np.abs(win.random(2048)).max() == 1.0
    for sym in SYMMETRIC.values():
        assert all(np.array_equal(sym(wl), sym(wl)[::-1]) for wl in win.MDCT_LENGTHS)


def test_fixture_inputs_have_not_drifted(fixture):
    for wl, hop, n in win.GOLDEN_CASES:
        x = win.clip(wl, n).astype(np.float64)
        assert float(x.sum()) == float(fixture[f"x_{wl}_{n}_sum"]) and float(np.abs(x).sum()) == float(fixture[f"x_{wl}_{n}_abs"])
        for name in win.NAMES:
            w = win.window(name, wl)
            assert float(w.sum()) == float(fixture[f"{name}_{wl}_sum"]) and float(np.abs(w).sum()) == float(fixture[f"{name}_{wl}_abs"])


# ---------------------------------------------------------------------------------------------------------------- oracle against the reference
@pytest.mark.parametrize("name", win.NAMES)
@pytest.mark.parametrize("wl,hop,n", win.GOLDEN_CASES)
def test_oracle_equals_the_reference_on_these_windows(fixture, name, wl, hop, n):
    x, w, tag = win.clip(wl, n).astype(np.float64), win.window(name, wl), f"{name}_{wl}"
    m = orc.mdct(x, w)
    got = {"mdct": m, "imdct": orc.imdct(fixture[f"{tag}_mdct"], w)}
    if hop is not None:
        s = orc.stft(x, w, hop)
        assert relerr(s[wl // 2 + 1:], np.conj(s[wl // 2 - 1:0:-1])) <= 1e-15
        filters, coefs = win.GOLDEN_MEL[wl]
        fb = orc.melfilterbank(win.FS, wl, filters)
        full = np.concatenate([fixture[f"{tag}_stft"], np.conj(fixture[f"{tag}_stft"][-2:0:-1])], axis=0)
        got.update(stft=s[: wl // 2 + 1], istft=orc.istft(full, w, hop), mel=orc.melspectrogram(x, w, hop, fb), mfcc=orc.mfcc(x, w, hop, fb, coefs))
    keys = {k[len(tag) + 1:] for k in fixture.files if k.startswith(tag + "_")} - {"sum", "abs"}
    assert keys == set(got), (tag, keys)
    for k, v in got.items():
        ref = fixture[f"{tag}_{k}"]
        assert v.shape == ref.shape and np.abs(ref).max() > 0
        assert relerr(v, ref) <= 1e-12, (tag, k, relerr(v, ref))


# ---------------------------------------------------------------------------------------------------------------- the windows discriminate
def _mirror_moves(fn, w):
    return relerr(fn(w[::-1]), fn(w))


@pytest.mark.parametrize("wl", win.MDCT_LENGTHS)
def test_a_mirrored_window_moves_the_mdct_and_the_imdct(wl):
    """relerr(oracle(x, w[::-1]), oracle(x, w)) >= 0.05 for every recipe at every MDCT window length of the GPU module; exactly 0 under KBD and
    the sine window -- the blind spot of every mdct / imdct test before this module."""
    x = synth_clip(31, 0, 3 * wl + 7).astype(np.float64)
    coefs = orc.mdct(x, orc.sine_window(wl))
    for name in win.NAMES:
        w = win.window(name, wl)
        fwd, inv = _mirror_moves(lambda v: orc.mdct(x, v), w), _mirror_moves(lambda v: orc.imdct(coefs, v), w)
        print(f"W={wl} {name}: mdct {fwd:.3f}, imdct {inv:.3f}")
        assert fwd >= 0.05 and inv >= 0.05, (wl, name, fwd, inv)
    for name, sym in SYMMETRIC.items():
        w = sym(wl)
        assert _mirror_moves(lambda v: orc.mdct(x, v), w) == 0.0 and _mirror_moves(lambda v: orc.imdct(coefs, v), w) == 0.0, (wl, name)


@pytest.mark.parametrize("wl,hop", sorted(set(win.STFT_GEOMETRIES) | {(64, 16), (256, 128)}))
def test_a_mirrored_window_moves_the_stft(wl, hop):
    x = synth_clip(32, 0, 6 * hop + 300).astype(np.float64)
    for name in win.NAMES:
        moved = _mirror_moves(lambda v: orc.stft(x, v, hop), win.window(name, wl))
        print(f"W={wl} hop={hop} {name}: stft {moved:.3f}")
        assert moved >= 0.05, (wl, hop, name, moved)
    for name, sym in SYMMETRIC.items():
        assert _mirror_moves(lambda v: orc.stft(x, v, hop), sym(wl)) == 0.0, (wl, hop, name)
    # periodic Hamming, the STFT family's only window so far, is one sample short of symmetric: at the tiled kernels' lengths a fully mirrored
    # one moves the result by about 1e-3 only (measured 1.5e-3 at W = 2048, 4e-4 at 8192)
    if wl >= 2048:
        assert _mirror_moves(lambda v: orc.stft(x, v, hop), orc.hamming_periodic(wl)) < 5e-3


# ---------------------------------------------------------------------------------------------------------------- the ISTFT's windows are usable
def test_cola_sums_of_the_istft_and_center_cases():
    """zaf.istft divides by sum(w[0:W:H]) (zaf.py:241): every (window, W, hop) of the GPU module's ISTFT and center tests keeps it at 0.25 or more
    in magnitude.  `random` does not everywhere (W = 4096, hop W / 2: 0.026), which is why those tests leave it out."""
    cases = [(n, wl, h) for n in win.ISTFT_WINDOWS for wl, h in win.ISTFT_GEOMETRIES] + [(n, wl, h) for n in win.CENTER_WINDOWS for wl, h in win.CENTER_GEOMETRIES]
    for name, wl, hop in cases:
        g = win.cola_gain(win.window(name, wl), hop)
        assert abs(g) >= win.MIN_COLA, (name, wl, hop, g)
    for name in ("skew", "signed"):
        assert {name} <= set(win.ISTFT_WINDOWS)
    for wl in (2048, 4096, 8192):
        assert 0.88 <= win.cola_gain(win.skew(wl), wl // 2) <= 1.04
    assert abs(win.cola_gain(win.random(4096), 2048)) < win.MIN_COLA


# ---------------------------------------------------------------------------------------------------------------- the mask filter's windows
COLA_TABLE = {"skew": (0.949, 0.925, 0.908, 0.898), "signed": (0.529, 0.536, 0.540, 0.543), "random": (-0.195, -0.438, 0.024, -0.374)}


def test_cola_sums_of_the_mask_filter_cases():
    """The table of tests/windows.py: skew and signed are used at all four lengths, random at W = 512 and 2048 -- at two lengths at least, and
    with a NEGATIVE sum there, which the kernels are handed as `gain`.  A recipe that silently dropped out of the GPU module fails here."""
    lengths = [wl for wl, _ in win.MASKFILTER_GEOMETRIES]
    assert lengths == [256, 512, 1024, 2048] and all(hop == wl // 2 for wl, hop in win.MASKFILTER_GEOMETRIES)
    for name, row in COLA_TABLE.items():
        for (wl, hop), want in zip(win.MASKFILTER_GEOMETRIES, row):
            g = win.cola_gain(win.window(name, wl), hop)
            assert abs(g - want) < 5e-4, (name, wl, g, want)
            assert ((name, wl) in win.MASKFILTER_WINDOWS) == (abs(g) >= win.MIN_COLA), (name, wl, g)
    used = {name: [wl for n, wl in win.MASKFILTER_WINDOWS if n == name] for name in win.NAMES}
    assert used["skew"] == lengths and used["signed"] == lengths and used["random"] == [512, 2048], used
    assert len(used["random"]) >= 2 and all(win.cola_gain(win.random(wl), wl // 2) < -win.MIN_COLA for wl in used["random"])
    assert len(win.MASKFILTER_WINDOWS) == 10
    # the stereo forms ride the same table: both are forms of test_maskfilter's loop, and the gain their model divides by is the table's sum
    import maskfilter_cases as mc
    assert {"stereo1", "stereo2"} <= set(mc.FORMS) and mc.KERNELS["stereo"] == ("k_maskfilter_stereo", "k_maskfilter_stereo_ragged")
    for name, wl in win.MASKFILTER_WINDOWS:
        w32 = mc.window_of(name, wl).astype(np.float32)
        assert abs(float(w32[0] + w32[wl // 2]) - COLA_TABLE[name][[256, 512, 1024, 2048].index(wl)]) < 5e-4, (name, wl)


def _periodic_mirror(w):
    return w[(len(w) - np.arange(len(w))) % len(w)]


@pytest.mark.parametrize("name,wl", win.MASKFILTER_WINDOWS)
def test_a_mirrored_window_moves_the_mask_filter(name, wl):
    """The oracle's mask filter, real and complex masks, under w[::-1] and under the periodic mirror w[(W - n) % W] moves by at least 5 % for
    every (window, W) the GPU module uses; under periodic Hamming the periodic mirror moves it by at most 1e-12 -- the blind spot of every
    mask-filter test before tests/test_gpu_windows.py's, asserted so that it stays documented."""
    import maskfilter_cases as mc
    h = wl // 2
    n = 20 * h + 9
    x = mc.clip(0, n).astype(np.float64)
    xs = mc.stereo_clip(0, n)
    filters = {"real": lambda v: mc.oracle_maskfilter(x, v, mc.masks_for("real", wl, n, 0, "unit")),
               "complex": lambda v: mc.oracle_maskfilter_complex(x, v, mc.masks_for("complex", wl, n, 0, None)),
               "stereo1": lambda v: mc.oracle_maskfilter_stereo(xs, v, mc.masks_for("stereo1", wl, n, 0, "unit")),
               "stereo2": lambda v: mc.oracle_maskfilter_stereo(xs, v, mc.masks_for("stereo2", wl, n, 0, "unit"))}
    w, ham = win.window(name, wl), mc.window_of("hamming", wl)
    for kind, fn in filters.items():
        full, periodic = relerr(fn(w[::-1]), fn(w)), relerr(fn(_periodic_mirror(w)), fn(w))
        blind = relerr(fn(_periodic_mirror(ham)), fn(ham))
        print(f"W={wl} {name} {kind}: mirrored {full:.3f}, periodic mirror {periodic:.3f}; periodic mirror under Hamming {blind:.1e}")
        assert full >= 0.05 and periodic >= 0.05, (name, wl, kind, full, periodic)
        assert blind <= 1e-12, (wl, kind, blind)


@pytest.mark.parametrize("name,wl", win.MASKFILTER_WINDOWS)
def test_a_mirrored_window_in_the_stereo_model_fails_the_gpu_check(name, wl):
    """tests/test_gpu_windows.py::test_maskfilter's check -- mask_error <= TOL_FFT on its own batches, the level over both channels -- applied
    to the float32 model of the stereo packing (maskfilter_cases.stereo_model): sound, it passes every (window, W), `random` with its negative
    gain included; with the window read at (W - n) % W it fails every one, both forms, y and the rest -- and has the sound model's bits
    under periodic Hamming, the only window the stereo and PCM kernels had met."""
    import maskfilter_cases as mc
    n = 20 * (wl // 2) + 9
    for form in sorted(mc.STEREO_DATA):
        assert form in mc.FORMS and mc.family_of(form) == "stereo"
        b, ham = mc.batch(form, wl, n, name, "unit"), mc.batch(form, wl, n, "hamming", "unit")
        for x, m, ref in zip(b["clips"], b["masks"], b["refs"]):
            sound, bad = mc.stereo_model_rows(x, b["w"], m), mc.stereo_model_rows(x, b["w"], m, "window_mirror")
            swapped = mc.stereo_model_rows(x, b["w"], m, "channel_swap")   # (the masks exchanged: seen under any window, by stereo2 alone)
            assert np.array_equal(swapped, sound) == (form == "stereo1"), (name, wl, form)
            for j in range(4):
                level = mc.row_level(ref, x, j, 2)
                assert mc.mask_error(sound[j], ref[j], level) <= mc.TOL_FFT, (name, wl, form, j)
                assert mc.mask_error(bad[j], ref[j], level) >= 1e3 * mc.TOL_FFT, (name, wl, form, j, mc.mask_error(bad[j], ref[j], level))
                assert form == "stereo1" or mc.mask_error(swapped[j], ref[j], level) >= 1e3 * mc.TOL_FFT, (name, wl, j)
        x, m = ham["clips"][0], ham["masks"][0]
        assert np.array_equal(mc.stereo_model_rows(x, ham["w"], m), mc.stereo_model_rows(x, ham["w"], m, "window_mirror"))


# ---------------------------------------------------------------------------------------------------------------- the tolerance yardstick
def mdct_in_float32(x, w):
    """The reference MDCT (zaf.py:1025-1075, as oracle.zaf_oracle.mdct restates it) in float32: scipy.fft on complex64, the same twiddles."""
    wl = len(w)
    hop = wl // 2
    nt = orc.mdct_num_frames(len(x), wl)
    xp = np.zeros((nt + 2) * hop, np.float32)
    xp[hop:hop + len(x)] = x
    w32 = w.astype(np.float32)
    pre = np.exp(-1j * np.pi / wl * np.arange(0, wl)).astype(np.complex64)
    post = np.exp(-1j * np.pi / wl * (wl / 2 + 1) * np.arange(0.5, wl / 2 + 0.5)).astype(np.complex64)
    out = np.zeros((hop, nt), np.float32)
    for j in range(nt):
        seg = scipy.fft.fft((xp[j * hop:j * hop + wl] * w32) * pre)
        assert seg.dtype == np.complex64
        out[:, j] = np.real(seg[:hop] * post)
    return out


@pytest.mark.parametrize("wl", [64, 512, 2048, 4096, 8192])
def test_float32_mdct_is_no_further_from_the_oracle_than_under_kbd(wl):
    """The evidence that the suite's tolerances need no widening for these windows: a plain float32 MDCT sits at 1.2e-7 ... 2.2e-7 of the oracle
    under them, 1.0e-7 ... 2.2e-7 under KBD -- the new windows within 2x the KBD figure of the same W, and all of it a fiftieth of 1e-5."""
    x = synth_clip(33, 0, 8 * wl + 5)
    x64 = x.astype(np.float64)
    kbd = orc.kbd_window(wl).astype(np.float32).astype(np.float64)
    base = relerr(mdct_in_float32(x, kbd), orc.mdct(x64, kbd))
    print(f"W={wl} kbd: {base:.2e}")
    assert 0 < base <= 1e-6
    for name in win.NAMES:
        w = win.window(name, wl)
        e = relerr(mdct_in_float32(x, w), orc.mdct(x64, w))
        print(f"W={wl} {name}: {e:.2e}")
        assert e <= 2.0 * base, (wl, name, e, base)


# ---------------------------------------------------------------------------------------------------------------- the fold table on the CPU
@pytest.fixture(scope="module")
def fold_emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mdct_fold_emu") / "mdct_fold_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-DZAFX_HOST_EMU", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "mdct_fold_emu.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _fold_error(exe, w):
    res = subprocess.run([exe], input=struct.pack("i", len(w)) + np.asarray(w, np.float32).tobytes(), capture_output=True)
    wl, err = res.stdout.decode().split()
    assert int(wl) == len(w)
    return res.returncode, float(err)


@pytest.mark.parametrize("wl", [64, 256])
def test_fold_table_gives_the_direct_mdct(fold_emu, wl):
    """zafx::mdct_fold_window -- the bytes finalize_constant uploads as d_wfold -- with k_mdct_ft32's fold, pack and tap pairing restated in double and a
    naive DFT, against X[k] = sum x[n] w[n] cos(2 pi / W (n + 1/2 + W/4)(k + 1/2)) to 1e-11, for the three recipes.  With components 0 and 3 of the
    quadruples of 2m < W/4 swapped in a scratch copy of the header the program fails on all three (0.019 ... 0.66) and still passes under KBD and
    the sine window (8e-15, 4e-14)."""
    for name in win.NAMES:
        rc, err = _fold_error(fold_emu, win.window(name, wl))
        print(f"W={wl} {name}: {err:.2e}")
        assert rc == 0 and err <= 1e-11, (wl, name, rc, err)
    for sym in SYMMETRIC.values():
        rc, err = _fold_error(fold_emu, sym(wl))
        assert rc == 0 and err <= 1e-11
