#!/usr/bin/env python3
"""Generate tests/golden/windows.npz by running the REAL reference on windows that are not mirror-symmetric (tests/windows.py: skew, signed,
random), so that the oracle the GPU window tests compare against stays pinned to the reference on exactly such windows.

Run where the reference lies (it never travels to the GPU box):

    MPLBACKEND=Agg python tests/golden/make_windows_golden.py

Cases (CASES below): W = 64 with hop 16 and W = 256 with hop 128 on 1000 samples -- zaf.stft (rows 0..W/2; the mirror rows are their
conjugates, checked here), zaf.istft of that spectrum, zaf.melspectrogram and zaf.mfcc (MEL: filters and coefficients per W), zaf.mdct and
zaf.imdct of those coefficients --, and W = 2048 on 3072 samples for zaf.mdct / zaf.imdct.  Keys: {window}_{W}_{function}; x_{W}_{n}_sum /
_abs and {window}_{W}_sum / _abs pin the recipes of the inputs (tests/windows.py: clip, window).  The fixture is DATA; no reference source
text is stored.
"""
import os
import sys

os.environ.setdefault("MPLBACKEND", "Agg")
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import zaf  # noqa: E402  (the reference)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import windows as win  # noqa: E402


def main():
    out = {}
    for wl, hop, n in win.GOLDEN_CASES:
        x = win.clip(wl, n).astype(np.float64)
        out[f"x_{wl}_{n}_sum"], out[f"x_{wl}_{n}_abs"] = np.array(x.sum()), np.array(np.abs(x).sum())
        for name in win.NAMES:
            w = win.window(name, wl)
            tag = f"{name}_{wl}"
            out[f"{tag}_sum"], out[f"{tag}_abs"] = np.array(w.sum()), np.array(np.abs(w).sum())
            m = zaf.mdct(x, w)
            out[f"{tag}_mdct"] = m
            out[f"{tag}_imdct"] = zaf.imdct(m, w)
            if hop is None:
                continue
            s = zaf.stft(x, w, hop)
            assert np.abs(s[wl // 2 + 1:] - np.conj(s[wl // 2 - 1:0:-1])).max() <= 1e-15 * np.abs(s).max()
            out[f"{tag}_stft"] = s[: wl // 2 + 1]
            out[f"{tag}_istft"] = zaf.istft(s, w, hop)
            filters, coefs = win.GOLDEN_MEL[wl]
            fb = zaf.melfilterbank(win.FS, wl, filters)
            out[f"{tag}_mel"] = zaf.melspectrogram(x, w, hop, fb)
            out[f"{tag}_mfcc"] = zaf.mfcc(x, w, hop, fb, coefs)
    assert all(np.isfinite(v).all() for v in out.values())
    path = os.path.join(HERE, "windows.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
