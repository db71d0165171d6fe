"""Child process of tests/test_gpu_maskfilter_complex.py: the complex mask filter of one clip of 60 blocks + 5 samples per window, alone (cut
into segments), as clip 2 of a batch of four and as one clip of a ragged batch, under whatever ZAFX_COMPUTE_UNITS the parent set; the results
go to the .npz named on the command line.

    python tests/maskfilter_complex_probe.py OUT.npz

The clips and masks are probe_case's, so the parent computes the same inputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "zaf-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

WINDOWS = (256, 512, 1024, 2048)
BLOCKS = 60


def probe_case(wl):
    """-> x (4, N) float32 and masks (4, W/2 + 1, T) complex64 in the unit disc, N = 60 blocks + 5 samples; clip 2 is the one the tests follow."""
    from maskfilter_oracle import mask_frames
    n = BLOCKS * (wl // 2) + 5
    g = np.random.default_rng([61, wl])
    shape = (4, wl // 2 + 1, mask_frames(n, wl))
    x = g.standard_normal((4, n)).astype(np.float32)
    return x, (np.sqrt(g.random(shape)) * np.exp(2j * np.pi * g.random(shape))).astype(np.complex64)


def main(path):
    import zafx
    res = {}
    for wl in WINDOWS:
        w = zafx.hamming(wl)
        x, m = probe_case(wl)
        res[f"alone{wl}"] = zafx.maskfilter_complex_batch(x[2:3], w, m[2:3])[0]
        res[f"batch{wl}"] = zafx.maskfilter_complex_batch(x, w, m)[2]
        res[f"ragged{wl}"] = zafx.maskfilter_complex_ragged([x[0, :700], x[2], x[1, :1]], w, [m[0, :, :zafx_frames(700, wl)], m[2], m[1, :, :2]])[1]
        res[f"units{wl}"] = np.array(zafx.maskfilter_plan(w, layout="TF").compute_units)
    np.savez(path, **res)
    print("probe ok")


def zafx_frames(n, wl):
    from maskfilter_oracle import mask_frames
    return mask_frames(n, wl)


if __name__ == "__main__":
    main(sys.argv[1])
