"""Deterministic windows that are NOT mirror-symmetric, shared by tests/golden/make_windows_golden.py (which feeds them to the real
reference) and the window tests (tests/test_windows_host.py, tests/test_gpu_windows.py).

KBD and the sine window satisfy w[n] == w[W-1-n] exactly, and the MDCT kernels are built around that mirror: the forward kernels read a
sign-folded table of window quadruples whose components are pairwise mirror images (zafx_wfold.hpp), the inverse unfolds
(u2, -u2_r, -u1_r, -u1) under the window.  Under a symmetric window a tap taken at its mirror position gives the same number; under these
it does not.  Each recipe is f(W) with n = arange(W) and t = (n + 0.5) / W, computed in float64 and rounded through float32 (what both
sides are fed), as tests/signals.py does.
"""
import numpy as np

NAMES = ("skew", "signed", "random")


def _f32_exact(w):
    return w.astype(np.float32).astype(np.float64)


def skew(window_length):
    """sin(pi t^0.6): smooth, positive, its peak left of the centre.  Its COLA sum at hop W / 2 is 0.88 ... 1.04."""
    t = (np.arange(window_length) + 0.5) / window_length
    return _f32_exact(np.sin(np.pi * t ** 0.6))


def signed(window_length):
    """skew with every third tap negated and a ramp 0.25 ... 1 over it: it changes sign, and its two halves have different levels."""
    n = np.arange(window_length)
    t = (n + 0.5) / window_length
    return _f32_exact(np.sin(np.pi * t ** 0.6) * np.where(n % 3 == 0, -1.0, 1.0) * (0.25 + 0.75 * t))


def random(window_length):
    """Seeded Gaussian taps scaled to a peak of 1: no structure at all, so any single misplaced tap moves a frame by about 1 / sqrt(W) of its
    level -- at least 1e-3 at W <= 8192, a hundred times the float32 tolerance."""
    g = np.random.default_rng([7, window_length]).standard_normal(window_length)
    return _f32_exact(g / np.abs(g).max())


RECIPES = {"skew": skew, "signed": signed, "random": random}


def window(name, window_length):
    return RECIPES[name](window_length)


# tests/golden/windows.npz (make_windows_golden.py): (W, hop or None = MDCT / IMDCT only, samples); mel filters and MFCCs per W
FS = 44100
GOLDEN_CASES = ((64, 16, 1000), (256, 128, 1000), (2048, None, 3072))
GOLDEN_MEL = {64: (6, 4), 256: (20, 8)}


def clip(window_length, n):
    """The fixture's input: unit white noise, float32."""
    return np.random.default_rng([2025, window_length]).standard_normal(n).astype(np.float32)


def cola_gain(w, step_length):
    """sum(w[0:W:H]), what zaf.istft divides by (zaf.py:241)."""
    return float(np.sum(np.asarray(w, dtype=np.float64)[0:len(w):step_length]))


# Geometries of tests/test_gpu_windows.py, which tests/test_windows_host.py holds to its three conditions: each recipe discriminates a mirrored
# window there (MDCT_LENGTHS, STFT_GEOMETRIES), and every (window, W, hop) the ISTFT and center tests use has a COLA sum zaf.istft can divide by.
MDCT_LENGTHS = (64, 256, 512, 1000, 1024, 2048, 4096, 8192)
STFT_GEOMETRIES = ((2048, 1024), (4096, 2048), (2048, 512), (1000, 250), (8192, 4096))   # (W, hop)
MEL_WINDOWS = ("skew", "random")
ISTFT_WINDOWS = ("skew", "signed")   # (random at W = 4096, hop W / 2: a COLA sum of 0.026 -- left out, not tested)
ISTFT_GEOMETRIES = ((2048, 1024), (2048, 512), (4096, 2048), (4096, 1024), (8192, 4096), (8192, 2048))
CENTER_WINDOWS = ("skew",)
CENTER_GEOMETRIES = ((2048, 1024), (256, 128))
MIN_COLA = 0.25

# The fused mask-filter kernels (hop W / 2 only).  Periodic Hamming, their tests' only window so far, satisfies w[n] == w[(W - n) % W]: a window
# read at that periodic mirror -- one `& (W - 1)` away from the bin pairing kn = (W - k) & (W - 1) the kernels compute -- is invisible under it.
# A recipe is used at a length only where zaf.istft can divide by its COLA sum: skew 0.949 / 0.925 / 0.908 / 0.898 and signed 0.529 / 0.536 /
# 0.540 / 0.543 at W = 256 / 512 / 1024 / 2048 everywhere, random -0.195 / -0.438 / 0.024 / -0.374 at W = 512 and 2048 -- where its sum is
# NEGATIVE, a gain these kernels had never been handed (tests/test_windows_host.py::test_cola_sums_of_the_mask_filter_cases).
MASKFILTER_GEOMETRIES = ((256, 128), (512, 256), (1024, 512), (2048, 1024))
MASKFILTER_WINDOWS = tuple((name, wl) for wl, hop in MASKFILTER_GEOMETRIES for name in NAMES if abs(cola_gain(window(name, wl), hop)) >= MIN_COLA)
