"""The float64 reference of the mask filter, shared by the host tests (tests/test_maskfilter_host.py) and the GPU tests
(tests/test_gpu_maskfilter.py): the reference's own composition of zaf.stft and zaf.istft around a real mask (zaf.py:185-195) on the
oracle's transforms, which tests/test_oracle_golden.py pins; tests/golden/maskfilter.npz pins the composition."""
import os

import numpy as np

TOL_FFT = 1e-5   # the project's bound for a float32 transform chain against the float64 reference


def mask_frames(n, wl):
    """Frames zaf.stft gives a clip of n samples at hop W/2 (zaf.py:99-109)."""
    h = wl // 2
    return -(-n // h) + 1


def oracle_maskfilter(x, w, m):
    """y = istft(concat(m, m[-2:0:-1]) * stft(x, w, W/2), w, W/2)[0:N] with the oracle's stft / istft, float64."""
    from oracle import zaf_oracle as orc
    x, m = np.asarray(x, np.float64), np.asarray(m, np.float64)
    wl, h = len(w), len(w) // 2
    assert m.shape == (h + 1, mask_frames(len(x), wl)), (m.shape, len(x), wl)
    s = orc.stft(x, w, h)
    return orc.istft(np.concatenate((m, m[-2:0:-1])) * s, w, h)[:len(x)]


def mask_error(y, ref, x):
    """max|y - ref| / max(max|ref|, max|x|): the level is the larger of the reference's and the input's -- a sparse mask leaves a reference
    far below the input whose rounding error it inherits."""
    y, ref, x = np.asarray(y, np.float64), np.asarray(ref, np.float64), np.asarray(x, np.float64)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    if not ref.size:
        return 0.0
    level = max(float(np.abs(ref).max()), float(np.abs(x).max()))
    return float(np.abs(y - ref).max()) / (level if level > 0 else 1.0)


def make_mask(kind, wl, n, seed=0):
    """The test masks, float32 (W/2 + 1, T): "ones", "uniform" in [0.25, 1], "sparse" (2 % ones, the rest zeros), "unit" (uniform in [0, 1])
    -- all in [0, 1] -- and "signed_wide", uniform in [-2, 2]: both signs and moduli above one."""
    shape = (wl // 2 + 1, mask_frames(n, wl))
    g = np.random.default_rng([77, seed, wl, n])
    if kind == "ones":
        return np.ones(shape, np.float32)
    if kind == "uniform":
        return g.uniform(0.25, 1.0, shape).astype(np.float32)
    if kind == "sparse":
        return (g.random(shape) < 0.02).astype(np.float32)
    if kind == "unit":
        return g.random(shape).astype(np.float32)
    if kind == "signed_wide":
        return g.uniform(-2.0, 2.0, shape).astype(np.float32)
    raise ValueError(kind)


def golden_cases():
    """(window_length, N, x float32 (N,), m float32 (W/2 + 1, T), y float64 (N,)) of tests/golden/maskfilter.npz."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maskfilter.npz"))
    for i in range(len([k for k in g.files if k.startswith("w")])):
        wl, n = (int(v) for v in g[f"w{i}"])
        yield wl, n, g[f"x{i}"], g[f"m{i}"], g[f"y{i}"]
