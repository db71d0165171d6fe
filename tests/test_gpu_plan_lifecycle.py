"""What a plan owns and how it is built (-m gpu), on the plans of tests/plan_cases.py -- one per family of tables, each at its smallest shape:

* no plan-owned allocation outlives its plan: zafx_plan_live_allocations is above its earlier value while the plan lives (constants set, one
  execute done) and back at it once the plan is destroyed;
* a zafx_plan_create that fails says exactly what it always said and leaves the count alone;
* every plan carries the kernel name, launches the kernel and writes the bytes recorded in tests/golden/plan_routes.json
  (tests/golden/make_plan_golden.py, run twice on the commit before the plan's tables got one owner and creation its named steps: the two
  recordings agreed on every case).  The hash holds the tables no tolerance test would catch to their values."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    return z


@pytest.fixture(scope="module")
def routes():
    with open(os.path.join(GOLDEN, "plan_routes.json")) as f:
        return json.load(f)


def live():
    from zafx import _lib
    n = ctypes.c_int64(-1)
    assert _lib.load().zafx_plan_live_allocations(ctypes.byref(n)) == 0
    return n.value


def case_names():
    import plan_cases
    return list(plan_cases.CASES)


def test_the_recorded_routes_are_the_cases(routes):
    assert list(routes) == case_names()
    assert all(len(r) == 3 and r[0] and r[1] and r[2] and len(r[2]) == 64 for r in routes.values())


@pytest.mark.parametrize("name", case_names())
def test_plan_owns_its_allocations_and_runs_as_recorded(zafx, routes, name):
    import plan_cases
    zafx.clear_plan_cache()
    before = live()
    plan, run = plan_cases.CASES[name]()
    try:
        out = np.ascontiguousarray(run(plan))
        during = live()
        planned, ran = plan.kernel_name, plan.last_kernel
    finally:
        plan.destroy()
        zafx.clear_plan_cache()
    after = live()
    print(name, "live allocations", before, during, after, planned, ran)
    assert during > before
    assert after == before
    assert [planned, ran] == routes[name][:2]
    assert hashlib.sha256(out.tobytes()).hexdigest() == routes[name][2]


# ---------------------------------------------------------------- failed creation: the message, and nothing left behind
STFT, ISTFT, MDCT, IMDCT, MEL, MFCC, CQT, CHROMA, LINEAR, DCT, CENTER = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
F64 = 1
WINDOW_MSG = ("window_length must be a power of two in [64, 8192] or any other length in [33, 8192] "
              "(any length in [2, 2048] with ZAFX_PRECISION_F64)")
MDCT_WINDOW_MSG = ("window_length must be a power of two in [64, 8192] or any even length in [34, 8192] "
                   "(any even length in [4, 2048] with ZAFX_PRECISION_F64)")
CENTER_HOP_MSG = ("center / sides: step_length must be window_length / 2 (zaf.stft pads window_length / 2 and zaf.istft trims window_length - step_length: "
                  "the two agree at no other hop)")
WITH_MEL_MSG = "with_mel (melspectrogram + mfcc in one pass) takes a float32 ZAFX_MFCC plan of window_length 2048, up to 128 filters and up to 32 coefficients"
DCT_LONG_MSG = "dct / dst: lengths above 8192 need N / 2 (types 2-4), N - 1 (dct type 1) or N + 1 (dst type 1) to be a power of two (at most 8192)"

# (kind, fields of zafx_params, device, the message) -- every check of zafx_plan_create ahead of the device, and every refusal of a family's
# geometry.  ("float32 mel/mfcc kernels are built for window_length 64 ... 8192 ..." cannot be reached: the window check before it is narrower.)
REFUSED = [
    (STFT, dict(struct_size=8, window_length=64, step_length=32), 0, "zafx_params.struct_size mismatch"),
    (STFT, dict(window_length=64, step_length=32, layout=2), 0, "bad layout"),
    (STFT, dict(window_length=64, step_length=32, spectrum=4), 0, "bad spectrum"),
    (STFT, dict(window_length=64, step_length=32, spectrum=-1), 0, "bad spectrum"),
    (MDCT, dict(window_length=64, spectrum=1), 0, "spectrum applies to ZAFX_STFT / ZAFX_ISTFT only"),
    (ISTFT, dict(window_length=64, step_length=32, spectrum=2), 0, "magnitude / power spectra are outputs of ZAFX_STFT only"),
    (STFT, dict(window_length=64, step_length=32, precision=2), 0, "bad precision"),
    (LINEAR, dict(window_length=4, n_filters=4, precision=F64), 0, "ZAFX_PRECISION_F64 is not available for ZAFX_LINEAR / ZAFX_DCT"),
    (DCT, dict(window_length=64, transform_type=2, precision=F64), 0, "ZAFX_PRECISION_F64 is not available for ZAFX_LINEAR / ZAFX_DCT"),
    (STFT, dict(window_length=64, step_length=32, row_align=24), 0, "row_align must be 0 or a power of two <= 1024"),
    (STFT, dict(window_length=64, step_length=32, row_align=2048), 0, "row_align must be 0 or a power of two <= 1024"),
    (STFT, dict(window_length=64, step_length=32, row_align=-1), 0, "row_align must be 0 or a power of two <= 1024"),
    (STFT, dict(window_length=64, step_length=32, row_align=16, layout=1), 0, "row_align applies to the 2-D arrays of ZAFX_LAYOUT_FT plans only"),
    (DCT, dict(window_length=64, transform_type=2, row_align=16), 0, "row_align applies to the 2-D arrays of ZAFX_LAYOUT_FT plans only"),
    (CENTER, dict(window_length=256, step_length=128, precision=F64),
     0, "center / sides: precision must be ZAFX_PRECISION_F32 (ZAFX_PRECISION_F64 is not available for these kinds)"),
    (CENTER, dict(window_length=128, step_length=64), 0, "center / sides: window_length must be a power of two in [256, 2048]"),
    (CENTER, dict(window_length=300, step_length=150), 0, "center / sides: window_length must be a power of two in [256, 2048]"),
    (CENTER, dict(window_length=256, step_length=64), 0, CENTER_HOP_MSG),
    (CENTER, dict(window_length=256, step_length=128, layout=1), 0, "center / sides: layout and row_align do not apply (no 2-D array crosses the boundary)"),
    (STFT, dict(window_length=64, step_length=32), 4096, "device index out of range"),
    (STFT, dict(window_length=64, step_length=32), -1, "device index out of range"),
    (STFT, dict(window_length=32, step_length=16), 0, WINDOW_MSG),
    (STFT, dict(window_length=16384, step_length=16), 0, WINDOW_MSG),
    (STFT, dict(window_length=2049, step_length=16, precision=F64), 0, WINDOW_MSG),
    (STFT, dict(window_length=64, step_length=0), 0, "step_length must be >= 1"),
    (ISTFT, dict(window_length=64, step_length=65), 0, "istft: step_length must not exceed window_length"),
    (STFT, dict(window_length=64, step_length=(1 << 20) + 1), 0, "step_length must not exceed 2^20"),
    (MEL, dict(window_length=2048, step_length=1024, n_filters=0), 0, "n_filters must be in [1, 576] (up to window_length / 2 with ZAFX_PRECISION_F64)"),
    (MEL, dict(window_length=2048, step_length=1024, n_filters=577), 0, "n_filters must be in [1, 576] (up to window_length / 2 with ZAFX_PRECISION_F64)"),
    (MEL, dict(window_length=2048, step_length=1024, n_filters=40, with_mel=1), 0, WITH_MEL_MSG),
    (MFCC, dict(window_length=1024, step_length=512, n_filters=40, n_coefs=13, with_mel=1), 0, WITH_MEL_MSG),
    (MFCC, dict(window_length=2048, step_length=1024, n_filters=40, n_coefs=0), 0, "n_coefs must be in [1, n_filters]"),
    (MFCC, dict(window_length=2048, step_length=1024, n_filters=40, n_coefs=41), 0, "n_coefs must be in [1, n_filters]"),
    (MEL, dict(window_length=64, step_length=32, n_filters=33, precision=F64), 0, "n_filters must not exceed window_length / 2"),
    (MDCT, dict(window_length=32), 0, MDCT_WINDOW_MSG),
    (MDCT, dict(window_length=101), 0, MDCT_WINDOW_MSG),
    (IMDCT, dict(window_length=2050, precision=F64), 0, MDCT_WINDOW_MSG),
    (CQT, dict(fft_length=256, step_length=80, n_bins=12, precision=F64), 0, "fft_length must be a power of two in [512, 131072] (ZAFX_PRECISION_F64 plan)"),
    (CQT, dict(fft_length=131072, step_length=80, n_bins=12), 0, "fft_length must be a power of two in [512, 65536] (up to 131072 with ZAFX_PRECISION_F64)"),
    (CQT, dict(fft_length=1000, step_length=80, n_bins=12), 0, "fft_length must be a power of two in [512, 65536] (up to 131072 with ZAFX_PRECISION_F64)"),
    (CQT, dict(fft_length=1024, step_length=0, n_bins=12), 0, "step_length must be >= 1"),
    (CQT, dict(fft_length=1024, step_length=80, n_bins=0), 0, "n_bins must be in [1, 1024]"),
    (CQT, dict(fft_length=1024, step_length=80, n_bins=1025), 0, "n_bins must be in [1, 1024]"),
    (CHROMA, dict(fft_length=1024, step_length=80, n_bins=12, octave_resolution=13), 0, "octave_resolution must be in [1, n_bins]"),
    (CHROMA, dict(fft_length=1024, step_length=80, n_bins=12, octave_resolution=0), 0, "octave_resolution must be in [1, n_bins]"),
    (LINEAR, dict(window_length=0, n_filters=4), 0, "linear map: window_length (columns) and n_filters (rows) must be in [1, 16384]"),
    (LINEAR, dict(window_length=4, n_filters=16385), 0, "linear map: window_length (columns) and n_filters (rows) must be in [1, 16384]"),
    (DCT, dict(window_length=64, transform_type=5), 0, "transform_type must be 1, 2, 3 or 4"),
    (DCT, dict(window_length=64, transform_type=2, transform_sine=2), 0, "transform_sine must be 0 (dct) or 1 (dst)"),
    (DCT, dict(window_length=1, transform_type=2), 0, "dct / dst: window_length must be at least 2"),
    (DCT, dict(window_length=8194, transform_type=2), 0, DCT_LONG_MSG),
    (99, dict(window_length=64, step_length=32), 0, "unknown plan kind"),
]


@pytest.mark.parametrize("kind,fields,device,message", REFUSED)
def test_refused_creation_keeps_its_words_and_leaks_nothing(zafx, kind, fields, device, message):
    from zafx import _lib
    lib = _lib.load()
    prm = _lib.ZafxParams()
    prm.struct_size = ctypes.sizeof(_lib.ZafxParams)
    for k, v in fields.items():
        setattr(prm, k, v)
    before = live()
    handle = ctypes.c_void_p()
    rc = lib.zafx_plan_create(ctypes.byref(handle), device, kind, ctypes.byref(prm))
    assert rc != 0 and not handle.value
    assert lib.zafx_last_error().decode() == message
    assert live() == before


def test_null_arguments_are_refused(zafx):
    from zafx import _lib
    lib = _lib.load()
    before = live()
    assert lib.zafx_plan_create(None, 0, STFT, None) != 0
    assert lib.zafx_last_error().decode() == "null argument"
    assert lib.zafx_plan_live_allocations(None) != 0
    assert lib.zafx_last_error().decode() == "null argument"
    assert lib.zafx_plan_destroy(None) == 0
    assert live() == before
