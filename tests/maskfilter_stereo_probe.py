"""Child process of tests/test_gpu_maskfilter_stereo.py: the stereo mask filter of one clip of 60 blocks + 5 sample frames per window and
mask_channels, alone (cut into segments), as clip 2 of a batch of four and as one clip of a ragged batch, under whatever
ZAFX_COMPUTE_UNITS the parent set; the results go to the .npz named on the command line.

    python tests/maskfilter_stereo_probe.py OUT.npz

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


def probe_case(wl, channels):
    """-> x (4, N, 2) float32 and masks (4, W/2 + 1, T) (channels == 1) or (4, 2, W/2 + 1, T) float32 in [0, 1], N = 60 blocks + 5 sample
    frames; clip 2 is the one the tests follow."""
    from maskfilter_oracle import mask_frames
    n = BLOCKS * (wl // 2) + 5
    g = np.random.default_rng([62, wl, channels])
    shape = (4,) + ((2,) if channels == 2 else ()) + (wl // 2 + 1, mask_frames(n, wl))
    return g.standard_normal((4, n, 2)).astype(np.float32), g.random(shape).astype(np.float32)


def ragged_of(x, m, wl):
    """The ragged batch around clip 2: clips of 5 and 20 H sample frames beside it, their masks cut from clips 0 and 1's."""
    from maskfilter_oracle import mask_frames
    h = wl // 2
    return [x[0, :5], x[2], x[1, :20 * h]], [m[0][..., :mask_frames(5, wl)], m[2], m[1][..., :mask_frames(20 * h, wl)]]


def main(path):
    import zafx
    res = {}
    for wl in WINDOWS:
        w = zafx.hamming(wl)
        for ch in (1, 2):
            x, m = probe_case(wl, ch)
            res[f"alone{wl}_{ch}"] = zafx.maskfilter_stereo_batch(x[2:3], w, m[2:3])[0]
            res[f"batch{wl}_{ch}"] = zafx.maskfilter_stereo_batch(x, w, m)[2]
            clips, masks = ragged_of(x, m, wl)
            res[f"ragged{wl}_{ch}"] = zafx.maskfilter_stereo_ragged(clips, w, masks)[1]
        res[f"units{wl}"] = np.array(zafx.maskfilter_plan(w, layout="TF").compute_units)
    np.savez(path, **res)
    print("probe ok")


if __name__ == "__main__":
    main(sys.argv[1])
