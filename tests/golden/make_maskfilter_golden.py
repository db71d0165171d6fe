#!/usr/bin/env python3
"""Generate tests/golden/maskfilter.npz by running the REAL reference: a real time-frequency mask between zaf.stft and zaf.istft, as
zaf.istft's docstring composes them (zaf.py:185-195).

Run where the reference lies (it never travels to the GPU box), with its directory in ZAF_REFERENCE unless zaf is importable as it is:

    ZAF_REFERENCE=<directory of zaf.py> MPLBACKEND=Agg python tests/golden/make_maskfilter_golden.py

Per case i: w{i} = (window_length, number of samples), x{i} = the float32-exact mono input (N,), m{i} = the float32 mask
(window_length / 2 + 1, T), seeded uniform in [0, 1], y{i} = the float64 result (N,).  The fixture is DATA; no reference source text
is stored.
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
    """zaf.py:190-195 with the mask handed in, on float64 copies of the float32 samples and mask."""
    x, m = x.astype(np.float64), m.astype(np.float64)
    s = zaf.stft(x, w, h)
    assert s.shape == (len(w), m.shape[1]) and m.shape[0] == len(w) // 2 + 1, (s.shape, m.shape)
    y = zaf.istft(np.multiply(np.concatenate((m, m[-2:0:-1, :])), s), w, h)[0:len(x)]
    assert y.shape == x.shape and np.isfinite(y).all()
    return y


def main():
    out = {}
    for i, (wl, n) in enumerate(CASES):
        w = scipy.signal.windows.hamming(wl, sym=False)
        g = np.random.default_rng([2025, i])
        x = g.standard_normal(n).astype(np.float32)
        frames = -(-n // (wl // 2)) + 1
        m = g.random((wl // 2 + 1, frames)).astype(np.float32)
        out[f"w{i}"] = np.array([wl, n], dtype=np.int64)
        out[f"x{i}"] = x
        out[f"m{i}"] = m
        out[f"y{i}"] = filtered(x, w, wl // 2, m)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "maskfilter.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
