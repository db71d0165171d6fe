"""Child process of tests/test_gpu_maskfilter_stems_ragged.py: the two ragged stems batches of its cut and deal tests -- the three clips the
cutter must cut at W = 2048 with three stems, the 600 short clips at W = 256 with two (the lengths of tests/maskfilter_ragged_probe.py) --
under whatever ZAFX_COMPUTE_UNITS the parent set; the results go to the .npz named on the command line.

    python tests/maskfilter_stems_ragged_probe.py OUT.npz [COMPUTE_UNITS]

COMPUTE_UNITS, if given, is what the plans must report.  The clips and masks are probe_batch's, so the parent computes the same inputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "zaf-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCHES = (("cut", 3), ("short", 2))   # (the lengths' name in maskfilter_ragged_probe, stems)


def probe_batch(which, n_stems):
    """-> (window_length, clips, masks): float32 clips and per clip (S, T_i, W/2 + 1) masks, uniform in [0, 1), a seed per (clip, stem)."""
    from maskfilter_oracle import mask_frames
    from maskfilter_ragged_probe import probe_lengths
    wl, lengths = probe_lengths(which)
    clips = [np.random.default_rng([62, wl, i]).standard_normal(n).astype(np.float32) for i, n in enumerate(lengths)]
    masks = [np.stack([np.random.default_rng([63, wl, i, s]).random((mask_frames(n, wl), wl // 2 + 1)).astype(np.float32) for s in range(n_stems)])
             for i, n in enumerate(lengths)]
    return wl, clips, masks


def run_batch(which, n_stems):
    """The batch through maskfilter_stems_ragged with the rest: -> (every clip's (S + 1, N_i) block, flat and back to back; the plan's compute units)."""
    import zafx
    wl, clips, masks = probe_batch(which, n_stems)
    w = zafx.hamming(wl)
    out = zafx.maskfilter_stems_ragged(clips, w, masks, rest=True, layout="TF")
    flat = np.concatenate([np.concatenate([stems.ravel(), rest]) for stems, rest in out])
    return flat, zafx.maskfilter_plan(w, rest=True, layout="TF").compute_units


def main(path, units=None):
    res = {}
    for which, n_stems in BATCHES:
        res[which], cus = run_batch(which, n_stems)
        assert units is None or cus == int(units), (cus, units)
        res[f"units_{which}"] = np.array(cus)
    np.savez(path, **res)
    print("probe ok")


if __name__ == "__main__":
    main(*sys.argv[1:3])
