"""The float64 reference of the mask filter under COMPLEX masks, shared by the host tests (tests/test_maskfilter_complex_host.py) and the GPU
tests (tests/test_gpu_maskfilter_complex.py): zaf.py:185-195 with the mask extended to its Hermitian mirror,

    y = istft(concat(M, conj(M[-2:0:-1])) * stft(x, w, W/2), w, W/2)[0:N],

on the oracle's transforms (zaf.istft keeps the real part of the inverse transform, zaf.py:223 -- so the imaginary parts of rows 0 and W/2,
the two bins that are their own mirror, have no effect).  tests/golden/maskfilter_complex.npz pins the composition to the reference."""
import os

import numpy as np

from maskfilter_oracle import TOL_FFT, mask_error, mask_frames  # noqa: F401  (the bound, the error measure and the frame count of the real kind)

MASK_KINDS = ("disc", "phase", "real", "sparse", "big")


def oracle_maskfilter_complex(x, w, m):
    """The composition above with the oracle's stft / istft, float64 / complex128."""
    from oracle import zaf_oracle as orc
    x, m = np.asarray(x, np.float64), np.asarray(m, np.complex128)
    wl, h = len(w), len(w) // 2
    assert m.shape == (h + 1, mask_frames(len(x), wl)), (m.shape, len(x), wl)
    s = orc.stft(x, w, h)
    return np.real(orc.istft(np.concatenate((m, np.conj(m[-2:0:-1]))) * s, w, h))[:len(x)]


def make_complex_mask(kind, wl, n, seed=0):
    """The seeded test masks, complex64 (W/2 + 1, T): "disc" (radius sqrt(u), uniform phase: uniform in the unit disc, |M| <= 1), "phase"
    (|M| = 1), "real" (a disc mask's real part, imaginary parts zero), "sparse" (2 % of unit modulus, the rest zero), "big" (8 x disc)."""
    shape = (wl // 2 + 1, mask_frames(n, wl))
    g = np.random.default_rng([78, seed, wl, n])
    disc = np.sqrt(g.random(shape)) * np.exp(2j * np.pi * g.random(shape))
    if kind == "disc":
        m = disc
    elif kind == "phase":
        m = np.exp(2j * np.pi * g.random(shape))
    elif kind == "real":
        m = disc.real + 0j
    elif kind == "sparse":
        m = np.where(g.random(shape) < 0.02, np.exp(2j * np.pi * g.random(shape)), 0)
    elif kind == "big":
        m = 8 * disc
    else:
        raise ValueError(kind)
    return m.astype(np.complex64)


def golden_cases():
    """(window_length, N, x float32 (N,), m complex64 (W/2 + 1, T), y float64 (N,)) of tests/golden/maskfilter_complex.npz."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskfilter_complex.npz"))
    for i in range(len([k for k in g.files if k.startswith("w")])):
        wl, n = (int(v) for v in g[f"w{i}"])
        yield wl, n, g[f"x{i}"], g[f"m{i}"], g[f"y{i}"]
