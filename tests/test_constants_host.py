"""The host side of tests/test_gpu_constants.py (no GPU): every case of tests/const_probe.py builds, its table of variants is the one the GPU test
is parametrised over, its constants are float32-exact, and the reference under every replacement differs from the reference under constants A
by MIN_CHANGE = 0.1 or more in every clip -- so no GPU case can pass by ignoring an upload."""
import numpy as np
import pytest

import const_probe as cp
import windows as win


@pytest.mark.parametrize("route", list(cp.ROUTES))
def test_every_replacement_changes_the_reference(route):
    case = cp.case(route)
    ref_a = case.refs(None)
    assert len(ref_a) == cp.N_CLIPS and all(np.isfinite(r).all() and np.any(r) for r in ref_a)
    for variant in cp.VARIANTS[route]:
        change = min(case.err(b, a) for a, b in zip(ref_a, case.refs(variant)))
        assert change >= cp.MIN_CHANGE, (route, variant, change)


@pytest.mark.parametrize("route", list(cp.ROUTES))
def test_constants_are_float32_exact(route):
    case = cp.case(route)
    if case.kw.get("f64"):
        return
    for consts in [case.consts] + [dict(steps) for steps in case.variants.values()]:
        for key, value in consts.items():
            if key in ("cqt", "cqt_values"):
                assert np.array_equal(value.data, value.data.astype(np.complex64).astype(np.complex128)), (route, key)
            else:
                assert np.array_equal(value, np.asarray(value).astype(np.float32).astype(np.float64)), (route, key)


def test_every_ragged_replacement_changes_the_reference():
    """The ragged cases of tests/test_gpu_constants.py: the two long clips change by MIN_CHANGE or more (an empty clip has nothing to change, and
    the center of a one-sample clip is x under any window)."""
    import test_gpu_constants as gpu
    for entry, build in gpu.RAGGED.items():
        case = build()
        pairs = list(zip(case.refs(None), case.refs("b")))[2:]
        assert len(pairs) == 2 and min(case.err(b, a) for a, b in pairs) >= cp.MIN_CHANGE, entry


def test_window_b_is_not_symmetric_and_keeps_its_gain():
    """Window B against A: no mirror symmetry (a stale folded window shows), another COLA sum (a stale gain shows), one zaf.istft can divide by."""
    for w, hop, mdct in ((2048, 1024, False), (4096, 2048, False), (8192, 4096, False), (1000, 500, False), (2048, 100, False), (256, 128, False), (2048, 1024, True)):
        a, b = cp.window_a(w, mdct), win.skew(w)
        assert (np.abs(a - a[::-1]) if mdct else np.abs(a[1:] - a[:0:-1])).max() < 1e-6   # (KBD mirrors around its middle, periodic Hamming around W / 2)
        assert np.abs(b - b[::-1]).max() > 0.1
        assert abs(win.cola_gain(b, hop)) >= win.MIN_COLA
        assert abs(win.cola_gain(b, hop) / win.cola_gain(a, hop) - 1.0) > 0.02, (w, hop)
    assert win.cola_gain(cp.window_zero_gain(2048, 1024), 1024) == 0.0


def test_filterbanks_reach_the_paths_they_are_for():
    a, b, c, d = cp.fb_mel(cp.FS, 2048, 128), cp.fb_mel(16000, 2048, 128), cp.fb_empty_block(cp.FS, 2048, 128), cp.fb_dense(2048, 128)
    assert a.shape == b.shape == c.shape == d.shape
    edges = lambda fb: [(int(np.flatnonzero(r)[0]), int(np.flatnonzero(r)[-1])) for r in fb]
    assert edges(a) != edges(b)                                  # other band edges: another step count and split
    assert not c[16:32].any() and c[:16].any() and c[32:].any()  # a 16-row block without non-zeros
    assert (d != 0).all()                                        # every block full width
