"""The float64 reference of the stereo mask filter, shared by the host tests (tests/test_maskfilter_stereo_host.py) and the GPU tests
(tests/test_gpu_maskfilter_stereo.py): zaf.py:176-198 with masks of the caller's,

    y[:, c] = istft(concat(m_c, m_c[-2:0:-1]) * stft(x[:, c], w, W/2), w, W/2)[0:N],   c = L, R,

on the oracle's transforms -- the real kind's composition (tests/maskfilter_oracle.py) on either channel.  A mask (W/2 + 1, T) serves both
channels, masks (2, W/2 + 1, T) one each.  tests/golden/maskfilter_stereo.npz pins the composition to the reference."""
import os

import numpy as np

from maskfilter_oracle import TOL_FFT, make_mask, mask_error, mask_frames, oracle_maskfilter  # noqa: F401  (the real kind's bound, masks, error measure)

MASK_KINDS = ("ones", "unit", "sparse", "signed_wide")


def oracle_maskfilter_stereo(x, w, m):
    """The composition above, float64 (N, 2); m: (W/2 + 1, T) for both channels or (2, W/2 + 1, T)."""
    x, m = np.asarray(x, np.float64), np.asarray(m, np.float64)
    assert x.ndim == 2 and x.shape[1] == 2 and m.ndim in (2, 3), (x.shape, m.shape)
    if not len(x):
        return np.zeros((0, 2))
    return np.stack([oracle_maskfilter(x[:, c], w, m if m.ndim == 2 else m[c]) for c in range(2)], axis=1)


def make_stereo_masks(kind, wl, n, channels, seed=0):
    """The real kind's seeded test masks (make_mask) for a stereo clip: float32 (W/2 + 1, T) for channels == 1, (2, W/2 + 1, T) -- two
    different masks of the kind -- for 2."""
    if channels == 1:
        return make_mask(kind, wl, n, seed)
    return np.stack([make_mask(kind, wl, n, 2 * seed + 100), make_mask(kind, wl, n, 2 * seed + 101)])


def stereo_error(y, ref, x):
    """mask_error with the level max(max|ref|, max|x|) taken over both channels."""
    return mask_error(np.asarray(y).reshape(-1), np.asarray(ref).reshape(-1), np.asarray(x).reshape(-1))


def golden_cases():
    """(window_length, N, x float32 (N, 2), m float32 (2, W/2 + 1, T), y float64 (N, 2) with both masks, s float64 (N, 2) with mask 0
    shared) of tests/golden/maskfilter_stereo.npz."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskfilter_stereo.npz"))
    for i in range(len([k for k in g.files if k.startswith("w")])):
        wl, n = (int(v) for v in g[f"w{i}"])
        yield wl, n, g[f"x{i}"], g[f"m{i}"], g[f"y{i}"], g[f"s{i}"]
