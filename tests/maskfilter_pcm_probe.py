"""Child process of tests/test_gpu_maskfilter_pcm.py: the PCM mask filter (int16 in, int16 out) of one clip of 60 blocks + 5 sample frames per
window and form -- mono, stereo under one mask, stereo under two --, alone (cut into segments), as clip 2 of a batch of four and as one clip
of a ragged batch, under whatever ZAFX_COMPUTE_UNITS the parent set; the results go to the .npz named on the command line.

    python tests/maskfilter_pcm_probe.py OUT.npz

The clips and masks are probe_case's, so the parent computes the same inputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "zaf-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

WINDOWS = (256, 512, 1024, 2048)
FORMS = ((1, 1), (2, 1), (2, 2))   # (n_channels, mask_channels)
BLOCKS = 60


def probe_case(wl, form):
    """-> x (4, N) or (4, N, 2) int16, full range, and masks (4, W/2 + 1, T) or (4, 2, W/2 + 1, T) float32 in [0, 1], N = 60 blocks + 5 sample
    frames; clip 2 is the one the tests follow."""
    from maskfilter_oracle import mask_frames
    ch, mc = form
    n = BLOCKS * (wl // 2) + 5
    g = np.random.default_rng([63, wl, ch, mc])
    shape = (4,) + ((2,) if mc == 2 else ()) + (wl // 2 + 1, mask_frames(n, wl))
    return g.integers(-32768, 32768, (4, n) + ((2,) if ch == 2 else ())).astype(np.int16), g.random(shape).astype(np.float32)


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
        for form in FORMS:
            x, m = probe_case(wl, form)
            tag = f"{wl}_{form[0]}{form[1]}"
            res["alone" + tag] = zafx.maskfilter_pcm_batch(x[2:3], w, m[2:3])[0]
            res["batch" + tag] = zafx.maskfilter_pcm_batch(x, w, m)[2]
            clips, masks = ragged_of(x, m, wl)
            res["ragged" + tag] = zafx.maskfilter_pcm_ragged(clips, w, masks)[1]
        res[f"units{wl}"] = np.array(zafx.maskfilter_plan(w, layout="TF").compute_units)
    np.savez(path, **res)
    print("probe ok")


if __name__ == "__main__":
    main(sys.argv[1])
