"""Child process of tests/test_gpu_maskfilter_stems.py: the three stems of one 60-block clip, alone (cut into segments) and as clip 2 of a
batch of four, under whatever ZAFX_COMPUTE_UNITS the parent set; the results go to the .npz named on the command line.

    python tests/maskfilter_stems_probe.py OUT.npz

The clips are maskfilter_probe.probe_case's and the masks are stems_case's, so the parent computes the same inputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "zaf-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

WINDOWS = (256, 2048)
STEMS = 3


def stems_case(wl):
    """-> x (4, N) float32 and masks (4, 3, T, W/2 + 1) float32 in [0, 1] ("TF"): probe_case's clips, stem s of clip c under probe_case's mask
    (c + 1 + s) mod 4; clip 2 is the one the tests follow."""
    from maskfilter_probe import probe_case
    x, m = probe_case(wl)
    masks = np.stack([np.stack([m[(c + 1 + s) % 4].T for s in range(STEMS)]) for c in range(4)])
    return x, np.ascontiguousarray(masks, np.float32)


def main(path):
    import zafx
    res = {}
    for wl in WINDOWS:
        w = zafx.hamming(wl)
        x, m = stems_case(wl)
        for rest in (False, True):
            tag = f"{wl}r" if rest else f"{wl}"
            alone = zafx.maskfilter_stems_batch(x[2:3], w, m[2:3], rest=rest, layout="TF")
            batch = zafx.maskfilter_stems_batch(x, w, m, rest=rest, layout="TF")
            res[f"alone{tag}"] = np.concatenate([alone[0][0], alone[1][0][None]]) if rest else alone[0]
            res[f"batch{tag}"] = np.concatenate([batch[0][2], batch[1][2][None]]) if rest else batch[2]
        res[f"units{wl}"] = np.array(zafx.maskfilter_plan(w, layout="TF").compute_units)
    np.savez(path, **res)
    print("probe ok")


if __name__ == "__main__":
    main(sys.argv[1])
