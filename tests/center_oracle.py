"""The float64 reference of the center / sides extraction, shared by the host tests (tests/test_center_host.py) and the GPU tests
(tests/test_gpu_center.py, tests/test_gpu_arena.py, tests/test_gpu_signals.py): the reference's own composition of zaf.stft and zaf.istft
(zaf.py:176-195) on the oracle's transforms, which tests/test_oracle_golden.py pins; tests/golden/center.npz pins the composition."""
import numpy as np


def oracle_center(x, w):
    """zaf.py:176-195 with the oracle's stft / istft, float64; the mask in the library's comparison form."""
    from oracle import zaf_oracle as orc
    x = np.asarray(x, np.float64)
    wl, h = len(w), len(w) // 2
    s = [orc.stft(x[:, c], w, h) for c in (0, 1)]
    a, b = np.abs(s[0][:wl // 2 + 1]), np.abs(s[1][:wl // 2 + 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        m = [np.where(b < a, b / a, 1.0), np.where(a < b, a / b, 1.0)]
    y = [orc.istft(np.concatenate((m[c], m[c][-2:0:-1])) * s[c], w, h)[:len(x)] for c in (0, 1)]
    return np.stack(y, axis=1)


# ------------------------------------------------------------------------------ the signal contract of the center (tests/signals.py, stereo)
TOL_CENTER = 1e-5      # the project's center bounds: center <= 1e-5 normwise, sides <= 1e-5 max|x| absolute (tests/test_gpu_center.py)
EPS32 = float(np.finfo(np.float32).eps)
C_CENTER = 16.0        # the floor's factor: measured, not chosen -- see center_figures and tests/test_center_host.py


def center_hops(y, h):
    """(N, 2) -> rows of one hop of one channel each (zero-filled at the end): (2 ceil(N / h), h)."""
    y = np.asarray(y)
    n = -(-len(y) // h) * h
    return np.pad(y, ((0, n - len(y)), (0, 0))).T.reshape(-1, h)


def center_figures(center, sides, x, ref, h, c=C_CENTER):
    """The figures the signal contract bounds, of one clip: center (N, 2) (and sides, or None) against ref = oracle_center(x, w), hop h.
      normwise  max|center - ref| / max|ref|; where the reference is identically zero, max|center| / max|x| (held to the input's level)
      sides     max|sides - (x - ref)| / max|x|
      hop       the worst |center - ref| / (10 tol max_hop|ref| + c eps32 max|x|) over hops of h samples per channel: conftest.row_bound with
                the floor on the INPUT's peak -- the center is bounded by the input, and a reference that is zero has no level of its own."""
    from conftest import excess, relerr, row_bound
    center, ref, x64 = np.asarray(center, np.float64), np.asarray(ref, np.float64), np.asarray(x, np.float64)
    peak_x = float(np.abs(x64).max()) if x64.size else 0.0
    if ref.size and np.any(ref):
        normwise = relerr(center, ref)
    elif not center.size:
        normwise = 0.0
    else:   # a reference of zeros: held to the input's level (an input of zeros too: any output at all counts in full)
        normwise = float(np.abs(center).max()) / (peak_x if peak_x > 0 else 1.0)
    e_s = 0.0
    if sides is not None and x64.size:
        e_s = float(np.abs(np.asarray(sides, np.float64) - (x64 - ref)).max()) / (peak_x if peak_x > 0 else 1.0)
    rows = center_hops(ref, h)
    hop = excess(center_hops(center, h), rows, row_bound(rows, TOL_CENTER, c * EPS32 * peak_x))
    return {"normwise": normwise, "sides": e_s, "hop": hop, "peak": peak_x}


def assert_center_contract(tag, center, sides, x, ref, h, report=None):
    """Finite; silence gives exact zeros; the three bounds of center_figures.  The figures go into report[tag] before anything is asserted
    (the key `row_excess` as in tests/test_gpu_signals.py's report).  -> the figures."""
    center = np.asarray(center)
    assert center.shape == np.asarray(x).shape, (tag, center.shape)
    finite = bool(np.isfinite(center).all() and (sides is None or np.isfinite(sides).all()))
    with np.errstate(invalid="ignore"):
        f = center_figures(center, sides, x, ref, h)
    if report is not None:
        report[tag] = {"normwise": f["normwise"], "row_excess": f["hop"], "sides": f["sides"], "peak": f["peak"], "finite": finite}
    assert finite, (tag, "not finite")
    if not np.any(x):
        assert not center.any() and (sides is None or not np.asarray(sides).any()), (tag, "silence must give exact zeros")
    assert f["normwise"] <= TOL_CENTER, (tag, "center normwise", f)
    assert f["sides"] <= TOL_CENTER, (tag, "sides", f)
    assert f["hop"] <= 1.0, (tag, "hop bound", f)
    return f
