#!/usr/bin/env python3
"""Generate tests/golden/maskfilter_stereo.npz by running the REAL reference: real time-frequency masks of the caller's between zaf.stft
and zaf.istft on either channel of a stereo clip, as zaf.istft's docstring composes them with its own masks (zaf.py:176-198).

Run where the reference lies (it never travels to the GPU box), with its directory in ZAF_REFERENCE unless zaf is importable as it is:

    ZAF_REFERENCE=<directory of zaf.py> MPLBACKEND=Agg python tests/golden/make_maskfilter_stereo_golden.py

(the committed fixture was made that way, with numpy's default_rng seeds [2027, i]).  Per case i: w{i} = (window_length, number of sample
frames), x{i} = the float32-exact stereo input (N, 2), m{i} = the float32 masks (2, window_length / 2 + 1, T), uniform in [0, 1], y{i} = the
float64 result (N, 2) with mask c on channel c, s{i} = the float64 result (N, 2) with mask 0 on both channels.  The fixture is DATA; no
reference source text is stored.
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
    """zaf.py:190-195 for one channel with the mask handed in, on float64 copies of the samples and the mask."""
    x, m = x.astype(np.float64), m.astype(np.float64)
    s = zaf.stft(x, w, h)
    assert s.shape == (len(w), m.shape[1]) and m.shape[0] == len(w) // 2 + 1, (s.shape, m.shape)
    y = zaf.istft(np.multiply(np.concatenate((m, m[-2:0:-1, :])), s), w, h)[0:len(x)]
    assert y.shape == x.shape and np.isrealobj(y) and np.isfinite(y).all()
    return y


def main():
    out = {}
    for i, (wl, n) in enumerate(CASES):
        w = scipy.signal.windows.hamming(wl, sym=False)
        g = np.random.default_rng([2027, i])
        x = g.standard_normal((n, 2)).astype(np.float32)
        frames = -(-n // (wl // 2)) + 1
        m = g.random((2, wl // 2 + 1, frames)).astype(np.float32)
        out[f"w{i}"] = np.array([wl, n], dtype=np.int64)
        out[f"x{i}"] = x
        out[f"m{i}"] = m
        out[f"y{i}"] = np.stack([filtered(x[:, c], w, wl // 2, m[c]) for c in range(2)], axis=1)
        out[f"s{i}"] = np.stack([filtered(x[:, c], w, wl // 2, m[0]) for c in range(2)], axis=1)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "maskfilter_stereo.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
