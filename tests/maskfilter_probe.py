"""Child process of tests/test_gpu_maskfilter.py: the mask filter of one 60-block clip, alone (cut into segments) and as clip 2 of a batch of
four, under whatever ZAFX_COMPUTE_UNITS the parent set; the results go to the .npz named on the command line.

    python tests/maskfilter_probe.py OUT.npz

The clips and masks are probe_case's, so the parent computes the same inputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "zaf-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

WINDOWS = (256, 2048)
BLOCKS = 60


def probe_case(wl):
    """-> x (4, N) float32 and masks (4, W/2 + 1, T) float32 in [0, 1], N = 60 blocks less 7 samples; clip 2 is the one the tests follow."""
    from maskfilter_oracle import mask_frames
    n = BLOCKS * (wl // 2) - 7
    g = np.random.default_rng([60, wl])
    return g.standard_normal((4, n)).astype(np.float32), g.random((4, wl // 2 + 1, mask_frames(n, wl))).astype(np.float32)


def main(path):
    import zafx
    res = {}
    for wl in WINDOWS:
        w = zafx.hamming(wl)
        x, m = probe_case(wl)
        res[f"alone{wl}"] = zafx.maskfilter_batch(x[2:3], w, m[2:3])[0]
        res[f"batch{wl}"] = zafx.maskfilter_batch(x, w, m)[2]
        res[f"units{wl}"] = np.array(zafx.maskfilter_plan(w).compute_units)
    np.savez(path, **res)
    print("probe ok")


if __name__ == "__main__":
    main(sys.argv[1])
