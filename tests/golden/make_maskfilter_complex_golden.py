#!/usr/bin/env python3
"""Generate tests/golden/maskfilter_complex.npz by running the REAL reference: a complex time-frequency mask, extended to its Hermitian
mirror, between zaf.stft and zaf.istft, as zaf.istft's docstring composes them with a real one (zaf.py:185-195).

Run where the reference lies (it never travels to the GPU box), with its directory in ZAF_REFERENCE unless zaf is importable as it is:

    ZAF_REFERENCE=<directory of zaf.py> MPLBACKEND=Agg python tests/golden/make_maskfilter_complex_golden.py

(the committed fixture was made that way, with numpy's default_rng seeds [2026, i]).  Per case i: w{i} = (window_length, number of samples),
x{i} = the float32-exact mono input (N,), m{i} = the complex64 mask (window_length / 2 + 1, T), seeded uniform in the unit disc -- rows 0
and window_length / 2 with NON-ZERO imaginary parts, which zaf.istft's np.real (zaf.py:223) drops: the fixture pins that rule --, y{i} =
the float64 result (N,).  The fixture is DATA; no reference source text is stored.
"""
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
if os.environ.get("ZAF_REFERENCE"):
    sys.path.insert(0, os.environ["ZAF_REFERENCE"])

import numpy as np  # noqa: E402
import scipy.signal.windows  # noqa: E402
import zaf  # noqa: E402  (the reference)

CASES = [(2048, 5000), (1024, 3000), (512, 1500), (256, 1)]


def filtered(x, w, h, m):
    """zaf.py:190-195 with the complex mask and its conjugate mirror handed in, on float64 / complex128 copies of the samples and mask."""
    x, m = x.astype(np.float64), m.astype(np.complex128)
    s = zaf.stft(x, w, h)
    assert s.shape == (len(w), m.shape[1]) and m.shape[0] == len(w) // 2 + 1, (s.shape, m.shape)
    y = zaf.istft(np.multiply(np.concatenate((m, np.conj(m[-2:0:-1, :]))), s), w, h)[0:len(x)]
    assert y.shape == x.shape and np.isrealobj(y) and np.isfinite(y).all()
    return y


def main():
    out = {}
    for i, (wl, n) in enumerate(CASES):
        w = scipy.signal.windows.hamming(wl, sym=False)
        g = np.random.default_rng([2026, i])
        x = g.standard_normal(n).astype(np.float32)
        frames = -(-n // (wl // 2)) + 1
        shape = (wl // 2 + 1, frames)
        m = (np.sqrt(g.random(shape)) * np.exp(2j * np.pi * g.random(shape))).astype(np.complex64)
        assert (m[0].imag != 0).all() and (m[-1].imag != 0).all()
        out[f"w{i}"] = np.array([wl, n], dtype=np.int64)
        out[f"x{i}"] = x
        out[f"m{i}"] = m
        out[f"y{i}"] = filtered(x, w, wl // 2, m)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "maskfilter_complex.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
