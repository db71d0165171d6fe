#!/usr/bin/env python3
"""Generate tests/golden/center.npz by running the REAL reference: the center / sides example of zaf.istft's docstring
(zaf.py:155-198) composed from zaf.stft and zaf.istft.

Run where the reference lies (it never travels to the GPU box):

    MPLBACKEND=Agg python tests/golden/make_center_golden.py

Per case i: w{i} = (window_length, number of sample frames), x{i} = the float32-exact stereo input (N, 2), c{i} = the float64
center (N, 2).  Inputs: L = c + 0.5 n1, R = 0.8 c + 0.5 n2 with seeded Gaussian c, n1, n2 -- a common part and an own part per
channel, so that both masks are in play.  The script asserts that no reference bin magnitude is exactly zero (where the
library's mask departs from the reference's 0 / 0) and that no output is NaN.  The fixture is DATA; no reference source
text is stored.
"""
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import scipy.signal.windows  # noqa: E402
import zaf  # noqa: E402  (the reference)

CASES = [(2048, 22050), (1024, 7168), (512, 7000), (256, 1)]


def stereo(seed, n):
    g = np.random.default_rng([2024, seed])
    c, n1, n2 = g.standard_normal(n), g.standard_normal(n), g.standard_normal(n)
    return np.stack([c + 0.5 * n1, 0.8 * c + 0.5 * n2], axis=1).astype(np.float32)


def center_of(x, w, h):
    """zaf.py:176-195, on float64 copies of the float32 samples."""
    x = x.astype(np.float64)
    wl = len(w)
    s_l, s_r = zaf.stft(x[:, 0], w, h), zaf.stft(x[:, 1], w, h)
    a, b = abs(s_l[0:wl // 2 + 1, :]), abs(s_r[0:wl // 2 + 1, :])
    assert a.min() > 0 and b.min() > 0, "a reference bin magnitude is exactly zero"
    m_l, m_r = np.minimum(a, b) / a, np.minimum(a, b) / b
    c_l = np.multiply(np.concatenate((m_l, m_l[-2:0:-1, :])), s_l)
    c_r = np.multiply(np.concatenate((m_r, m_r[-2:0:-1, :])), s_r)
    y_l, y_r = zaf.istft(c_l, w, h), zaf.istft(c_r, w, h)
    c = np.stack((y_l, y_r), axis=1)[0:len(x), :]
    assert c.shape == x.shape and not np.isnan(c).any()
    return c


def main():
    out = {}
    for i, (wl, n) in enumerate(CASES):
        w = scipy.signal.windows.hamming(wl, sym=False)
        x = stereo(i, n)
        out[f"w{i}"] = np.array([wl, n], dtype=np.int64)
        out[f"x{i}"] = x
        out[f"c{i}"] = center_of(x, w, wl // 2)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "center.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
