"""Child process of tests/test_gpu_maskfilter_ragged.py: the two ragged mask-filter batches of its cut-and-deal test -- three clips the cutter
must cut at W = 2048, 600 short clips at W = 256 -- under whatever ZAFX_COMPUTE_UNITS the parent set; the results go to the .npz named on the
command line.

    python tests/maskfilter_ragged_probe.py OUT.npz

The clips and masks are probe_batch's, so the parent computes the same inputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "zaf-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCHES = ("cut", "short")


def probe_lengths(which):
    """-> (window_length, lengths): "cut": 60, 61 and 200 blocks at W = 2048; "short": 600 clips of 1 - 6 blocks at W = 256."""
    if which == "cut":
        return 2048, [60 * 1024, 61 * 1024 - 3, 200 * 1024 - 500]
    g = np.random.default_rng(600)
    return 256, (g.integers(0, 6, 600) * 128 + g.integers(1, 129, 600)).tolist()


def probe_batch(which):
    """-> (window_length, clips, masks): float32 clips and (W/2 + 1, T_i) masks in [0, 1]."""
    from maskfilter_oracle import mask_frames
    wl, lengths = probe_lengths(which)
    g = np.random.default_rng([61, wl])
    clips = [g.standard_normal(n).astype(np.float32) for n in lengths]
    masks = [g.random((wl // 2 + 1, mask_frames(n, wl))).astype(np.float32) for n in lengths]
    return wl, clips, masks


def main(path):
    import zafx
    res = {}
    for which in BATCHES:
        wl, clips, masks = probe_batch(which)
        w = zafx.hamming(wl)
        out = zafx.maskfilter_ragged(clips, w, masks, rest=True)
        res[which] = np.concatenate([np.concatenate(pair) for pair in out])
        res[f"units_{which}"] = np.array(zafx.maskfilter_plan(w, rest=True).compute_units)
    np.savez(path, **res)
    print("probe ok")


if __name__ == "__main__":
    main(sys.argv[1])
