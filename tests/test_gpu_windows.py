"""Every windowed kernel under windows that are NOT mirror-symmetric (-m gpu): tests/windows.py's skew, signed and random.

The suite's other modules hand the STFT family periodic Hamming (one sample short of symmetric: a fully mirrored window moves a result by 1e-3,
a form that mirrors one percent of its taps by the 1e-5 tolerance) and every mdct / imdct call KBD or the sine window, which satisfy
w[n] == w[W-1-n] exactly.  The MDCT kernels are built around that mirror -- the forward ones read a sign-folded table of window quadruples whose
components are pairwise mirror images (zafx_wfold.hpp), the inverse unfolds (u2, -u2_r, -u1_r, -u1) under the window -- so a tap taken at its
mirror position, in the table, in a kernel's copy of it or in an unfold, passes all of them.  Under these windows it moves the result by 5 % or
more (tests/test_windows_host.py, which also pins the oracle to the real reference on them and shows that a plain float32 MDCT is no further
from the oracle under them than under KBD: the tolerances here are the suite's own, unchanged).

Input: unit white noise (conftest.synth_clip), two clips of different seeds per call.  Reference: the float64 oracle.  Bounds, normwise
(conftest.relerr) per clip: 1e-5 for stft / istft / mdct / imdct, 1e-4 for mel / mfcc, 1e-12 for the float64 kernels; the center under
center_oracle.assert_center_contract as it is.  After each call the kernel that ran is asserted: through tests/test_gpu_signals.py's ROUTES and
assert_route where that table covers the geometry, else against a name read off the dispatch code (zafx_mdct.hip run_mdct / run_mdct_p /
run_imdct, zafx_stft.hip run_stft / run_istft, zafx_bs32.hip, zafx_f64.hip, zafx_mel.hip) and given beside the case.  Kernel forms that share a
name are reached by geometry: the carry instantiation of k_mdct_ft32 by compact rows off the line grid with n % 4 == 0, its 4-byte-load form by
n % 4 != 0, k_stft_ft16's run-time-claim form by rows of whole lines (its static twin: a plan made under ZAFX_STFT_DYNAMIC=0).

Shapes: the smallest that hold a whole tile and an edge tile of the form under test.  ISTFT and center leave out `random`, whose COLA sum
zaf.istft divides by is 0.026 at W = 4096, hop W / 2 (tests/test_windows_host.py::test_cola_sums_of_the_istft_and_center_cases).

The fused mask-filter kernels -- the six mono ones, k_maskfilter_stereo and its ragged twin, the four PCM kernels -- read the window itself, and their blind spot is the PERIODIC mirror: periodic Hamming, their other tests' only
window, satisfies w[n] == w[(W - n) % W].  test_maskfilter runs every form of tests/maskfilter_cases.py under the (window, W) pairs of
windows.MASKFILTER_WINDOWS -- skew and signed at W = 256 ... 2048, random at 512 and 2048, where its COLA sum, the kernels' `gain`, is negative.
A library whose mask-filter kernels read window[(W - n) & (W - 1)] fails all ten cases on the MI355X and passes the 160 accuracy cases, the signal
cases and the ragged, complex and ragged-stems modules, which run under Hamming.

Measured on MI355X, 2026-10-18 (242 tests, 3 s; the maskfilter rows 2026-10-21), worst normwise error per group (the test functions' first argument to held()) and window, over
every form and row padding mode of the group -- f64: the float64 kernels of every group; set ZAFX_WINDOWS_REPORT=path to have a run write its own:
    mdct_2048     random 1.46e-07, signed 1.83e-07, skew 1.72e-07
    mdct_4096     random 1.94e-07, signed 1.63e-07, skew 1.80e-07
    mdct_8192     random 1.92e-07, signed 1.53e-07, skew 1.76e-07
    mdct_small    random 2.32e-07, signed 2.29e-07, skew 2.09e-07
    mdct_ragged   random 1.77e-07, signed 2.05e-07, skew 1.97e-07
    mdct_pcm      random 1.83e-07, signed 2.26e-07, skew 1.92e-07
    imdct         random 1.91e-07, signed 2.22e-07, skew 2.66e-07
    imdct_ragged  random 1.51e-07, signed 1.59e-07, skew 1.96e-07
    f64           random 2.07e-13, signed 2.07e-13, skew 1.75e-13
    stft          random 2.34e-07, signed 2.10e-07, skew 2.25e-07
    stft_ragged   random 1.83e-07, signed 2.03e-07, skew 2.05e-07
    mel           random 3.89e-07, skew 4.82e-07
    istft         signed 3.01e-07, skew 1.91e-07
    istft_ragged  signed 1.34e-07, skew 1.48e-07
    center        skew 4.22e-07, worst hop 0.0045 of its bound
    cache         skew 2.17e-07
    maskfilter    random 1.82e-07, signed 2.15e-07, skew 3.38e-07   (mask_error; the six fused mono kernels, every form: test_maskfilter)
    maskfilter_stereo           random 1.56e-07, signed 1.71e-07, skew 2.02e-07   (k_maskfilter_stereo and _ragged, one mask and two; the level over both channels)
    maskfilter_stereo_vs_mono   random 1.81e-07, signed 1.69e-07, skew 2.00e-07   (two masks: channel c against k_maskfilter on the planar channel c under mask c)
    maskfilter_pcm              no figure of its own: the four PCM kernels' float32 output has the float kernels' BITS under every window, int16 is its quantiser
Every float32 transform sits at 1.3e-7 ... 3.0e-7 -- where the same kernels sit under Hamming and KBD (tests/test_gpu_signals.py) -- and no form
was found with a mirrored tap.  That the module would see one: a library whose fold table has components 0 and 3 swapped (2m < W/4) passes the
MDCT tests of test_gpu_signals.py, test_gpu_mdct_ragged.py and test_gpu_pcm_ragged.py (KBD) on the MI355X and fails 57 of these (test_mdct_2048, _frame_major_and_row_align, test_mdct_4096, the W = 512 /
1024 cases of test_mdct_generic_and_bluestein, test_mdct_ragged, test_mdct_pcm); tests/test_windows_host.py has the same check on the CPU.
"""
import functools
import json
import os

import numpy as np
import pytest

import signals as sig
import windows as win
from center_oracle import assert_center_contract, oracle_center
from conftest import relerr, synth_clip
from oracle import zaf_oracle as orc
from test_gpu_signals import CENTER_SHAPES, ROUTES, assert_route

pytestmark = pytest.mark.gpu

TOL_FFT = 1e-5
TOL_FB = 1e-4
TOL_F64 = 1e-12

_report = {}


@pytest.fixture(scope="module")
def zafx_lib():
    import zafx as z
    assert z.device_count() >= 1
    yield z
    z.set_row_padding("auto")
    z.set_precision("f32")
    path = os.environ.get("ZAFX_WINDOWS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_report, f, indent=1, sort_keys=True)


@pytest.fixture(params=["compact", "auto"])
def zafx_mode(request, zafx_lib):
    zafx_lib.set_row_padding(request.param)
    yield zafx_lib
    zafx_lib.set_row_padding("auto")


@pytest.fixture
def zafx(zafx_lib):
    zafx_lib.set_row_padding("auto")
    return zafx_lib


# ------------------------------------------------------------------------------------------------------------------ inputs and references
def clips(n, seed=40):
    """Two clips of unit noise with different seeds, float32 (2, n)."""
    return np.stack([synth_clip(seed, 0, n), synth_clip(seed + 1, 0, n)])


@functools.lru_cache(maxsize=None)
def ref_mdct(name, wl, n, seed=40):
    w = win.window(name, wl)
    out = tuple(orc.mdct(x.astype(np.float64), w) for x in clips(n, seed))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_imdct(name, wl, n, seed=40):
    w = win.window(name, wl)
    out = tuple(orc.imdct(m, w) for m in ref_mdct(name, wl, n, seed))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_stft(name, wl, hop, n, seed=40):
    w = win.window(name, wl)
    out = tuple(orc.stft(x.astype(np.float64), w, hop) for x in clips(n, seed))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_istft(name, wl, hop, n, seed=40):
    w = win.window(name, wl)
    out = tuple(orc.istft(s, w, hop) for s in ref_stft(name, wl, hop, n, seed))
    for a in out:
        a.setflags(write=False)
    return out


def held(group, name, got, refs, tol, what=""):
    """Every clip of `got` within `tol` of its reference, normwise; the worst goes into the report under group.window before the assertion."""
    assert len(got) == len(refs), (group, name, what)
    worst = 0.0
    for i, (g, r) in enumerate(zip(got, refs)):
        g = np.asarray(g)
        assert g.shape == r.shape, (group, name, what, i, g.shape, r.shape)
        assert np.isfinite(g).all(), (group, name, what, i)
        worst = max(worst, relerr(g, r))
    key = f"{group}.{name}"
    _report[key] = max(_report.get(key, 0.0), worst)
    print(f"{group} {name} {what}: {worst:.3e}")
    assert worst <= tol, (group, name, what, worst, tol)


def ran(plan, want, *what):
    assert plan.last_kernel == want, (what, plan.last_kernel, want)


# ------------------------------------------------------------------------------------------------------------------ forward MDCT, W = 2048
# n: T = 35 with n % 4 != 0 (the 4-byte-load form of k_mdct_ft32), T = 35 with n % 4 == 0 (16-byte buffer loads; compact rows off the line grid:
# the carry instantiation, padded rows: the plain one with the window quadruples in registers), T = 32 (on the grid: the plain form in either mode)
MDCT_2048 = (1024 * 33 + 5, 1024 * 33 + 4, 1024 * 31)


@pytest.mark.parametrize("n", MDCT_2048)
@pytest.mark.parametrize("name", win.NAMES)
def test_mdct_2048(zafx_mode, name, n):
    zafx = zafx_mode
    w, x, refs = win.window(name, 2048), clips(n), ref_mdct(name, 2048, n)
    got = zafx.mdct_batch(x, w)
    assert_route(zafx, 2048, "mdct", refs[0].shape[1], 32, lambda a: zafx.mdct_plan(w, row_align=a), got)
    held("mdct_2048", name, got, refs, TOL_FFT, f"{zafx.get_row_padding()} n={n}")


@pytest.mark.parametrize("name", win.NAMES)
def test_mdct_2048_frame_major_and_row_align(zafx, name):
    """layout "TF" (TFOUT: the wave that transformed a frame stores it) and an explicit row_align=32 on a frame count off the grid."""
    n = MDCT_2048[1]
    w, x, refs = win.window(name, 2048), clips(n), ref_mdct(name, 2048, n)
    got = zafx.mdct_batch(x, w, layout="TF")
    ran(zafx.mdct_plan(w, layout="TF"), "k_mdct_ft32", "TF")   # (mdct_use_persistent: W = 512 ... 2048 in either layout)
    held("mdct_2048", name, got, [r.T for r in refs], TOL_FFT, "TF")
    got = zafx.mdct_batch(x, w, row_align=32)
    ran(zafx.mdct_plan(w, row_align=32), "k_mdct_ft32", "row_align")
    assert got.strides[-2] == 64 * 4   # T = 35 in rows of 64 floats
    held("mdct_2048", name, got, refs, TOL_FFT, "row_align=32")


# ------------------------------------------------------------------------------------------------------------------ forward MDCT, W = 4096 / 8192
@pytest.mark.parametrize("name", win.NAMES)
def test_mdct_4096(zafx_mode, name):
    """n = 2048 * 33 + 4 (T = 35): k_mdct_ft32bc on compact rows, k_mdct_ft32b on rows padded to whole lines (ROUTES).  n = 2048 * 33 + 5: the band
    kernels load 16-byte pieces and take clips of a multiple of four samples only (run_mdct) -- the generic k_mdct at its largest tiled size."""
    zafx = zafx_mode
    w = win.window(name, 4096)
    n = 2048 * 33 + 4
    got = zafx.mdct_batch(clips(n), w)
    assert_route(zafx, 4096, "mdct", 35, 32, lambda a: zafx.mdct_plan(w, row_align=a), got)
    held("mdct_4096", name, got, ref_mdct(name, 4096, n), TOL_FFT, f"{zafx.get_row_padding()} n={n}")
    n = 2048 * 33 + 5
    got = zafx.mdct_batch(clips(n), w)
    ran(zafx.mdct_plan(w, row_align=32 if zafx.get_row_padding() == "auto" else 0), "k_mdct", 4096, n)
    held("mdct_4096", name, got, ref_mdct(name, 4096, n), TOL_FFT, f"{zafx.get_row_padding()} n={n}")


@pytest.mark.parametrize("name", win.NAMES)
def test_mdct_8192(zafx_mode, name):
    """k_mdct_ft32q (T = 48: rows on the line grid in either mode).  It reads the window itself, not the fold table."""
    zafx = zafx_mode
    w, n = win.window(name, 8192), 4096 * 47 - 100
    got = zafx.mdct_batch(clips(n), w)
    assert_route(zafx, 8192, "mdct", 48, 32, lambda a: zafx.mdct_plan(w, row_align=a), got)
    held("mdct_8192", name, got, ref_mdct(name, 8192, n), TOL_FFT, zafx.get_row_padding())


# ------------------------------------------------------------------------------------------------------------------ forward MDCT, generic and Bluestein
# (W, n, kernel): W = 64, 256 on the generic k_mdct (one frame per slot, the window from d_window); W = 512, 1024 on k_mdct_ft32, whose 4-byte-load
# form n % 4 != 0 selects (run_mdct_p); W = 1000 on the float32 Bluestein form
MDCT_SMALL = ((64, 9 * 64 + 3, "k_mdct"), (256, 9 * 256 + 3, "k_mdct"), (512, 9 * 512 + 3, "k_mdct_ft32"), (1024, 9 * 1024 + 3, "k_mdct_ft32"),
              (1000, 20000, "k_mdct_bs32"))


@pytest.mark.parametrize("wl,n,kernel", MDCT_SMALL)
@pytest.mark.parametrize("name", win.NAMES)
def test_mdct_generic_and_bluestein(zafx_mode, name, wl, n, kernel):
    zafx = zafx_mode
    w, refs = win.window(name, wl), ref_mdct(name, wl, n)
    got = zafx.mdct_batch(clips(n), w)
    padded = zafx.get_row_padding() == "auto" and refs[0].shape[1] % 32
    ran(zafx.mdct_plan(w, row_align=32 if padded else 0), kernel, wl, n)
    held("mdct_small", name, got, refs, TOL_FFT, f"W={wl} {zafx.get_row_padding()}")


# ------------------------------------------------------------------------------------------------------------------ ragged and PCM MDCT
L4 = (0, 4, 1020, 2048, 32 * 1024, 32 * 1024 + 4)   # multiples of 4 around one frame and around a 32-frame tile edge: the 16-byte-load form
L_ODD = tuple(n + (1, 2, 3)[i % 3] for i, n in enumerate(L4))   # the same plus 1, 2, 3: the 4-byte-load form


def ragged_clips(lengths, seed=50):
    return [synth_clip(seed + i, 0, n) for i, n in enumerate(lengths)]


@pytest.mark.parametrize("lengths", [L4, L_ODD], ids=["multiples_of_4", "odd"])
@pytest.mark.parametrize("wl", [2048, 512])
@pytest.mark.parametrize("name", win.NAMES)
def test_mdct_ragged(zafx, name, wl, lengths):
    w, xs = win.window(name, wl), ragged_clips(lengths)
    _, in_off, lens = zafx.pack_ragged(xs)
    assert not (in_off % 4).any() and bool((lens % 4).any()) == (lengths is L_ODD)   # (the launcher's condition for the 16-byte form, or not)
    got = zafx.mdct_ragged(xs, w)
    ran(zafx.mdct_plan(w, row_align=32), "k_mdct_ft32_ragged", wl)
    held("mdct_ragged", name, got, [orc.mdct(x.astype(np.float64), w) for x in xs], TOL_FFT, f"W={wl} {'odd' if lengths is L_ODD else 'x4'}")


def pcm_of(x, channels):
    """Unit noise as int16 at a quarter of full scale (clipped at the ends of the range); stereo: the second channel a shifted copy."""
    p = np.clip(np.rint(x.astype(np.float64) * 8192.0), -32768, 32767).astype(np.int16)
    return p if channels == 1 else np.ascontiguousarray(np.stack([p, np.roll(p, 7)], axis=-1))


def host_f32(p):
    """wavread's x / 2^15 and the channel mean in float32 on the host: exact for int16 of one or two channels."""
    x = p.astype(np.float32) / np.float32(32768.0)
    return x if x.ndim == 1 else x.mean(axis=1, dtype=np.float32)


@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("name", win.NAMES)
def test_mdct_pcm(zafx_lib, name, channels):
    """int16 read by the kernel itself (the power of two of the normalisation rides in the window quadruples): mdct_pcm_ragged on L4 and
    mdct_pcm_batch at T = 35, each against the oracle and bit-equal to its float twin on the same samples (tests/test_gpu_pcm_ragged.py)."""
    zafx = zafx_lib
    w = win.window(name, 2048)
    pcm = [pcm_of(x, channels) for x in ragged_clips(L4)]
    got = zafx.mdct_pcm_ragged(pcm, w)
    ran(zafx.mdct_plan(w, row_align=32), "k_mdct_ft32_ragged", "pcm")
    twin = zafx.mdct_ragged([host_f32(p) for p in pcm], w)
    ran(zafx.mdct_plan(w, row_align=32), "k_mdct_ft32_ragged", "float twin")
    held("mdct_pcm", name, got, [orc.mdct(host_f32(p).astype(np.float64), w) for p in pcm], TOL_FFT, f"ragged ch={channels}")
    for i, (g, t) in enumerate(zip(got, twin)):
        assert np.array_equal(g, t), (name, channels, i)
    n = MDCT_2048[1]
    pb = np.stack([pcm_of(x, channels) for x in clips(n)])
    zafx.set_row_padding("compact")   # (the *_pcm_batch functions run on the compact plan: the float twin on the same form)
    try:
        got = zafx.mdct_pcm_batch(pb if channels == 2 else pb[:, :, None], w)
        ran(zafx.mdct_plan(w), "k_mdct_ft32", "pcm batch")
        xf = np.stack([host_f32(p) for p in pb])
        twin = zafx.mdct_batch(xf, w)
        ran(zafx.mdct_plan(w), "k_mdct_ft32", "float twin")
    finally:
        zafx.set_row_padding("auto")
    held("mdct_pcm", name, got, [orc.mdct(x.astype(np.float64), w) for x in xf], TOL_FFT, f"batch ch={channels}")
    assert np.array_equal(got, twin), (name, channels)


# ------------------------------------------------------------------------------------------------------------------ IMDCT
# (W, n of the clips whose oracle coefficients are the input, kind of ROUTES or kernel): k_imdct at W = 64 ... 4096, k_imdct_q, the Bluestein form
IMDCT_CASES = ((64, 9 * 64 + 3, "k_imdct"), (256, 9 * 256 + 3, "k_imdct"), (512, 9 * 512 + 3, "k_imdct"), (1024, 9 * 1024 + 3, "k_imdct"),
               (2048, 1024 * 33 + 5, "k_imdct"), (2048, 1024 * 31, "k_imdct"), (4096, 2048 * 33 + 5, "k_imdct"), (8192, 4096 * 47 - 100, "k_imdct_q"),
               (1000, 20000, "k_imdct_frames_bs32"))


@pytest.mark.parametrize("wl,n,kernel", IMDCT_CASES)
@pytest.mark.parametrize("name", win.NAMES)
def test_imdct(zafx_mode, name, wl, n, kernel):
    """The inverse on its own: the oracle's coefficient blocks in, orc.imdct of them as the reference."""
    zafx = zafx_mode
    w, blocks, refs = win.window(name, wl), np.stack(ref_mdct(name, wl, n)), ref_imdct(name, wl, n)
    t = blocks.shape[2]
    got = zafx.imdct_batch(blocks, w)
    if (wl, "imdct") in ROUTES:
        assert ROUTES[(wl, "imdct")][(zafx.get_row_padding(), "off" if t % 32 else "on")] == kernel
        assert_route(zafx, wl, "imdct", t, 32, lambda a: zafx.mdct_plan(w, inverse=True, row_align=a))
    else:   # (run_imdct: one kernel for every tiled W below 8192, at any pitch)
        ran(zafx.mdct_plan(w, inverse=True, row_align=32 if zafx.get_row_padding() == "auto" and t % 32 else 0), kernel, wl)
    held("imdct", name, got, refs, TOL_FFT, f"W={wl} T={t} {zafx.get_row_padding()}")


@pytest.mark.parametrize("name", win.NAMES)
def test_imdct_2048_frame_major(zafx, name):
    n = MDCT_2048[0]
    w, refs = win.window(name, 2048), ref_imdct(name, 2048, n)
    got = zafx.imdct_batch(np.stack([m.T for m in ref_mdct(name, 2048, n)]), w, layout="TF")
    ran(zafx.mdct_plan(w, layout="TF", inverse=True), "k_imdct", "TF")
    held("imdct", name, got, refs, TOL_FFT, "W=2048 TF")


IMDCT_RAGGED_T = (1, 2, 31, 32, 33, 70)


@pytest.mark.parametrize("wl", [2048, 512])
@pytest.mark.parametrize("name", win.NAMES)
def test_imdct_ragged(zafx, name, wl):
    """k_imdct_ragged: blocks of 1 ... 70 frames (both sides of a 32-frame tile edge) in one launch."""
    w, m = win.window(name, wl), wl // 2
    lengths = [max((t - 1) * m - 5, 0) for t in IMDCT_RAGGED_T]
    blocks = [orc.mdct(x.astype(np.float64), w) for x in ragged_clips(lengths, seed=60)]
    assert tuple(b.shape[1] for b in blocks) == IMDCT_RAGGED_T
    got = zafx.imdct_ragged(blocks, w)
    ran(zafx.mdct_plan(w, inverse=True, row_align=32), "k_imdct_ragged", wl)
    held("imdct_ragged", name, got, [orc.imdct(b, w) for b in blocks], TOL_FFT, f"W={wl}")


# ------------------------------------------------------------------------------------------------------------------ float64 MDCT / IMDCT
@pytest.mark.parametrize("wl,n,fwd,inv", [(2048, 1024 * 17 + 2, "k_mdct_ft16_f64", "k_imdct_ft16_f64"), (256, 3000, "k_mdct_f64", "k_imdct_frames_f64")])
@pytest.mark.parametrize("name", win.NAMES)
def test_mdct_imdct_in_float64(zafx_mode, name, wl, n, fwd, inv):
    zafx = zafx_mode
    w, x, refs = win.window(name, wl), clips(n).astype(np.float64), ref_mdct(name, wl, n)
    t = refs[0].shape[1]
    a = 16 if zafx.get_row_padding() == "auto" and t % 16 else 0   # (a line of float64: 16 elements)
    got = zafx.mdct_batch(x, w, f64=True)
    ran(zafx.mdct_plan(w, f64=True, row_align=a), fwd, wl)
    assert got.dtype == np.float64
    held("f64", name, got, refs, TOL_F64, f"mdct W={wl} {zafx.get_row_padding()}")
    got = zafx.imdct_batch(np.stack(refs), w, f64=True)
    ran(zafx.mdct_plan(w, inverse=True, f64=True, row_align=a), inv, wl)
    held("f64", name, got, ref_imdct(name, wl, n), TOL_F64, f"imdct W={wl} {zafx.get_row_padding()}")


@pytest.mark.parametrize("name", win.NAMES)
def test_drop_ins_in_float64(zafx, name):
    """zafx.mdct / zafx.imdct, the zaf.* signatures, with the device arithmetic set to float64."""
    n = 1024 * 17 + 2
    w, refs = win.window(name, 2048), ref_mdct(name, 2048, n)
    zafx.set_precision("f64")
    try:
        got = zafx.mdct(clips(n)[0].astype(np.float64), w)
        back = zafx.imdct(refs[0], w)
    finally:
        zafx.set_precision("f32")
    held("f64", name, [got], refs[:1], TOL_F64, "zafx.mdct")
    held("f64", name, [back], ref_imdct(name, 2048, n)[:1], TOL_F64, "zafx.imdct")


# ------------------------------------------------------------------------------------------------------------------ STFT
def stft_n(hop):
    return 20 * hop + 300


@pytest.mark.parametrize("wl,hop", win.STFT_GEOMETRIES)
@pytest.mark.parametrize("name", win.NAMES)
def test_stft(zafx_mode, name, wl, hop):
    """Two-sided spectra of 22 frames (W = 1000: 23) -- rows off the line grid: compact, the carry forms k_stft_ft16c / k_stft_ft16bc and, at W = 8192, the
    generic k_stft; padded to whole lines, k_stft_ft16 (tiles claimed at run time) / k_stft_ft16b / k_stft_ft16q; W = 1000: k_stft_bs32 (ROUTES)."""
    zafx = zafx_mode
    n = stft_n(hop)
    w, refs = win.window(name, wl), ref_stft(name, wl, hop, n)
    t = refs[0].shape[1]
    assert t % 16
    got = zafx.stft_batch(clips(n), w, hop)
    assert_route(zafx, wl, "two_sided", t, 16, lambda a: zafx.stft_plan(w, hop, row_align=a), got)
    held("stft", name, got, refs, TOL_FFT, f"W={wl} hop={hop} {zafx.get_row_padding()}")


@pytest.mark.parametrize("name", win.NAMES)
def test_stft_2048_one_sided_and_magnitude(zafx_mode, name):
    zafx = zafx_mode
    hop = 1024
    n = stft_n(hop)
    w, refs = win.window(name, 2048), ref_stft(name, 2048, hop, n)
    t = refs[0].shape[1]
    got = zafx.stft_batch(clips(n), w, hop, onesided=True)
    assert_route(zafx, 2048, "one_sided", t, 16, lambda a: zafx.stft_plan(w, hop, onesided=True, row_align=a), got)
    held("stft", name, got, [r[:1025] for r in refs], TOL_FFT, f"one-sided {zafx.get_row_padding()}")
    got = zafx.stft_batch(clips(n), w, hop, onesided="magnitude")
    assert_route(zafx, 2048, "magnitude", t, 32, lambda a: zafx.stft_plan(w, hop, onesided="magnitude", row_align=a), got)   # k_mel2
    held("stft", name, got, [np.abs(r[:1025]) for r in refs], TOL_FFT, f"magnitude {zafx.get_row_padding()}")


@pytest.mark.parametrize("name", win.NAMES)
def test_stft_claimed_tiles_equal_the_static_split(zafx, name):
    """k_stft_ft16 on rows of whole lines claims its tiles at run time (run_stft_fat; tests/test_gpu_stft_dynamic.py); a plan made under
    ZAFX_STFT_DYNAMIC=0 keeps the static split.  Both read the window the same way: bit-identical, and the claimed one is held to the oracle."""
    from zafx import _lib
    from zafx.core import Plan
    hop = 1024
    n = stft_n(hop)
    w, x, refs = win.window(name, 2048), clips(n), ref_stft(name, 2048, hop, n)
    got = zafx.stft_batch(x, w, hop)
    cached = zafx.stft_plan(w, hop, row_align=16)
    ran(cached, "k_stft_ft16", "claimed")
    assert cached.row_pitch(n) % 16 == 0
    held("stft", name, got, refs, TOL_FFT, "claimed tiles")
    old = os.environ.get("ZAFX_STFT_DYNAMIC")
    os.environ["ZAFX_STFT_DYNAMIC"] = "0"
    try:
        static = Plan(_lib.STFT, 0, window_length=2048, step_length=hop, layout="FT", onesided=False, row_align=16)
        static.set_window(w)
    finally:
        if old is None:
            del os.environ["ZAFX_STFT_DYNAMIC"]
        else:
            os.environ["ZAFX_STFT_DYNAMIC"] = old
    twin = static.run_host(x, n)
    ran(static, "k_stft_ft16", "static")
    static.destroy()
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(twin[..., :got.shape[-1]]).view(np.uint32))


STFT_RAGGED = (0, 1, 3072, 16 * 1024 + 3, 20 * 1024 + 300)


@pytest.mark.parametrize("name", win.NAMES)
def test_stft_ragged(zafx, name):
    """k_stft_ft16_ragged (two-sided) and k_mel2_ragged (|X|) at W = 2048: clips of 0 samples ... 22 frames in one launch."""
    hop = 1024
    w, xs = win.window(name, 2048), ragged_clips(STFT_RAGGED, seed=70)
    specs = [orc.stft(x.astype(np.float64), w, hop) for x in xs]
    got = zafx.stft_ragged(xs, w, hop)
    ran(zafx.stft_plan(w, hop, row_align=16), "k_stft_ft16_ragged")
    held("stft_ragged", name, got, specs, TOL_FFT, "two-sided")
    got = zafx.stft_ragged(xs, w, hop, onesided="magnitude")
    ran(zafx.stft_plan(w, hop, onesided="magnitude", row_align=32), "k_mel2_ragged")
    held("stft_ragged", name, got, [np.abs(s[:1025]) for s in specs], TOL_FFT, "magnitude")


@pytest.mark.parametrize("name", win.NAMES)
def test_stft_in_float64(zafx_mode, name):
    zafx = zafx_mode
    hop = 1024
    n = stft_n(hop)
    w, refs = win.window(name, 2048), ref_stft(name, 2048, hop, n)
    got = zafx.stft_batch(clips(n).astype(np.float64), w, hop, f64=True)
    a = 8 if zafx.get_row_padding() == "auto" and refs[0].shape[1] % 8 else 0   # (a line of complex128: 8 elements)
    ran(zafx.stft_plan(w, hop, f64=True, row_align=a), "k_stft_ft8_f64")
    held("f64", name, got, refs, TOL_F64, f"stft {zafx.get_row_padding()}")


# ------------------------------------------------------------------------------------------------------------------ mel / MFCC
@pytest.mark.parametrize("name", win.MEL_WINDOWS)
def test_mel_mfcc_2048(zafx, name):
    """k_mel2 (mel, mfcc), k_mel2_ragged and k_mel_ft8_f64: W = 2048, hop 1024, 128 bands, 20 coefficients."""
    hop = 1024
    n = stft_n(hop)
    w, x = win.window(name, 2048), clips(n)
    fb = zafx.melfilterbank(sig.FS, 2048, 128)
    x64 = x.astype(np.float64)
    mel = [orc.melspectrogram(c, w, hop, fb) for c in x64]
    cep = [orc.mfcc(c, w, hop, fb, 20) for c in x64]
    got = zafx.melspectrogram_batch(x, w, hop, fb)
    ran(zafx.mel_plan(w, hop, fb), "k_mel2", "mel")
    held("mel", name, got, mel, TOL_FB, "mel W=2048")
    got = zafx.mfcc_batch(x, w, hop, fb, 20)
    ran(zafx.mel_plan(w, hop, fb, 20), "k_mel2", "mfcc")
    held("mel", name, got, cep, TOL_FB, "mfcc W=2048")
    xs = ragged_clips(STFT_RAGGED[2:], seed=70)
    got = zafx.melspectrogram_ragged(xs, w, hop, fb)
    ran(zafx.mel_plan(w, hop, fb, row_align=32), "k_mel2_ragged", "mel")
    held("mel", name, got, [orc.melspectrogram(c.astype(np.float64), w, hop, fb) for c in xs], TOL_FB, "mel ragged")
    got = zafx.mfcc_ragged(xs, w, hop, fb, 20)
    ran(zafx.mel_plan(w, hop, fb, 20, row_align=32), "k_mel2_ragged", "mfcc")
    held("mel", name, got, [orc.mfcc(c.astype(np.float64), w, hop, fb, 20) for c in xs], TOL_FB, "mfcc ragged")
    got = zafx.melspectrogram_batch(x64, w, hop, fb, f64=True)
    ran(zafx.mel_plan(w, hop, fb, f64=True), "k_mel_ft8_f64", "mel")
    held("f64", name, got, mel, TOL_F64, "mel")
    got = zafx.mfcc_batch(x64, w, hop, fb, 20, f64=True)
    ran(zafx.mel_plan(w, hop, fb, 20, f64=True), "k_mel_ft8_f64", "mfcc")
    held("f64", name, got, cep, TOL_F64, "mfcc")


@pytest.mark.parametrize("name", win.MEL_WINDOWS)
def test_mel_mfcc_4096(zafx, name):
    """k_mel_ft16b: W = 4096, hop 2048, 64 bands (mfcc: 20 coefficients)."""
    hop = 2048
    n = stft_n(hop)
    w, x = win.window(name, 4096), clips(n)
    fb = zafx.melfilterbank(sig.FS, 4096, 64)
    x64 = x.astype(np.float64)
    got = zafx.melspectrogram_batch(x, w, hop, fb)
    ran(zafx.mel_plan(w, hop, fb), "k_mel_ft16b", "mel")
    held("mel", name, got, [orc.melspectrogram(c, w, hop, fb) for c in x64], TOL_FB, "mel W=4096")
    got = zafx.mfcc_batch(x, w, hop, fb, 20)
    ran(zafx.mel_plan(w, hop, fb, 20), "k_mel_ft16b", "mfcc")
    held("mel", name, got, [orc.mfcc(c, w, hop, fb, 20) for c in x64], TOL_FB, "mfcc W=4096")


# ------------------------------------------------------------------------------------------------------------------ ISTFT
# the window enters the inverse only through sum(w[0:W:H]) (zaf.py:241).  Kernel per (W, hop), run_istft: hop W / 2 as in ROUTES; hop W / 4:
# W = 2048 stays on k_istft_ft16, W = 4096 takes the band form k_istft_ft16b (a hop that is a multiple of 4, at least 512), W = 8192 the generic
# k_istft (the four-class kernel is for hop W / 2 only)
ISTFT_QUARTER_HOP = {2048: "k_istft_ft16", 4096: "k_istft_ft16b", 8192: "k_istft"}


@pytest.mark.parametrize("wl,hop", win.ISTFT_GEOMETRIES)
@pytest.mark.parametrize("name", win.ISTFT_WINDOWS)
def test_istft(zafx_mode, name, wl, hop):
    zafx = zafx_mode
    n = stft_n(hop)
    w, specs, refs = win.window(name, wl), np.stack(ref_stft(name, wl, hop, n)), ref_istft(name, wl, hop, n)
    t = specs.shape[2]
    assert abs(win.cola_gain(w, hop)) >= win.MIN_COLA
    got = zafx.istft_batch(specs, w, hop)
    if 2 * hop == wl:
        assert_route(zafx, wl, "istft", t, 16, lambda a: zafx.istft_plan(w, hop, row_align=a))
    else:
        ran(zafx.istft_plan(w, hop, row_align=16 if zafx.get_row_padding() == "auto" and t % 16 else 0), ISTFT_QUARTER_HOP[wl], wl, hop)
    held("istft", name, got, refs, TOL_FFT, f"W={wl} hop={hop} {zafx.get_row_padding()}")


ISTFT_RAGGED_T = (1, 2, 15, 16, 17, 40)


@pytest.mark.parametrize("name", win.ISTFT_WINDOWS)
def test_istft_ragged_and_float64(zafx, name):
    """k_istft_ragged: spectra of 1 ... 40 frames (both sides of a 16-frame tile edge) in one launch; k_istft_ft8_f64 on the equal-length batch."""
    wl, hop = 2048, 1024
    w = win.window(name, wl)
    lengths = [max((t - 1) * hop - 5, 0) for t in ISTFT_RAGGED_T]
    specs = [orc.stft(x.astype(np.float64), w, hop) for x in ragged_clips(lengths, seed=80)]
    assert tuple(s.shape[1] for s in specs) == ISTFT_RAGGED_T
    got = zafx.istft_ragged(specs, w, hop)
    ran(zafx.istft_plan(w, hop, row_align=16), "k_istft_ragged")
    held("istft_ragged", name, got, [orc.istft(s, w, hop) for s in specs], TOL_FFT)
    n = stft_n(hop)
    got = zafx.istft_batch(np.stack(ref_stft(name, wl, hop, n)), w, hop, f64=True)
    ran(zafx.istft_plan(w, hop, f64=True, row_align=8), "k_istft_ft8_f64")   # (T = 22 in rows of 24 complex128)
    held("f64", name, got, ref_istft(name, wl, hop, n), TOL_F64, "istft")


# ------------------------------------------------------------------------------------------------------------------ center / sides
@pytest.mark.parametrize("signal", ["pan_tones", "gain"])
@pytest.mark.parametrize("wl,n", CENTER_SHAPES[1:])
def test_center(zafx, wl, n, signal):
    """k_center and k_center_ragged under `skew` (tests/test_center_host.py: the float32 emulation keeps half the bound under it)."""
    w = win.skew(wl)
    assert (wl, wl // 2) in win.CENTER_GEOMETRIES
    x = sig.stereo_signal(signal, n)
    ref = oracle_center(x, w)
    c, s = zafx.centersides_batch(x[None], w)
    ran(zafx.center_plan(w, sides=True), "k_center")
    f = assert_center_contract(f"k_center.skew.{signal}_{wl}", c[0], s[0], x, ref, wl // 2)
    _report["center.skew"] = max(_report.get("center.skew", 0.0), f["normwise"])
    _report["center.skew.hop"] = max(_report.get("center.skew.hop", 0.0), f["hop"])
    lengths = [n, 9 * (wl // 2) + wl // 4, 1]
    xs = [sig.stereo_signal(signal, k) for k in lengths]
    res = zafx.centersides_ragged(xs, w)
    ran(zafx.center_plan(w, sides=True), "k_center_ragged")
    for k, xk, (ck, sk) in zip(lengths, xs, res):
        f = assert_center_contract(f"k_center_ragged.skew.{signal}_{wl}_{k}", ck, sk, xk, oracle_center(xk, w), wl // 2)
        _report["center.skew"] = max(_report["center.skew"], f["normwise"])
        _report["center.skew.hop"] = max(_report["center.skew.hop"], f["hop"])


# ------------------------------------------------------------------------------------------------------------------ the fused mask filters
@pytest.mark.parametrize("name,wl", win.MASKFILTER_WINDOWS)
def test_maskfilter(zafx, name, wl):
    """The six fused mask-filter kernels under a window that is not its own periodic mirror (periodic Hamming is: a window read at
    (W - n) % W passes every other mask-filter test) and, where `random` runs, under a negative COLA gain.  Three clips of 20 H + 9 samples,
    "unit" / "disc" masks, the rest on: every form of tests/maskfilter_cases.py through its equal-length launch and -- with clips of 1, H,
    3 H + 7 and 0 samples between the same three -- through its ragged one, every stem and the rest within TOL_FFT (mask_error) of the float64
    oracle; the ragged launch gives the shared clips the bits of the equal-length one, and each stem has the bits of the one-mask kind.

    The stereo forms (k_maskfilter_stereo, one mask and two) are forms of the same loop, the level of their bound taken over both channels;
    with two different masks channel c must also lie within TOL_FFT of k_maskfilter on the planar channel c under mask c.  The four PCM
    kernels run on the same windows and masks -- mono "TF" and the two stereo forms, the clips rint(16384 x) clipped to int16 --: float32 out
    has the bits of the float kernel on the clip / 32768, int16 out is the quantiser of that output and the rest clip(x - y_q) in integers,
    equal-length and ragged."""
    import maskfilter_cases as mc
    import maskfilter_run as mr
    from test_gpu_maskfilter_pcm import int_rest, numpy_quantise
    assert (wl, wl // 2) in win.MASKFILTER_GEOMETRIES
    n = 20 * (wl // 2) + 9
    worst = {"maskfilter": 0.0, "maskfilter_stereo": 0.0, "maskfilter_stereo_vs_mono": 0.0}
    for form in mc.FORMS:
        family, data, tail = mc.family_of(form), mc.data_of(form), mc.rest_rows(form)
        group = "maskfilter_stereo" if family == "stereo" else "maskfilter"
        b = mc.batch(data, wl, n, name, "unit")
        twin, where = mc.ragged_twin(b, mc.extras(data, wl, name))
        got = mr.run(form, b["w"], b["clips"], b["masks"], True, ragged=False)
        rag = mr.run(form, twin["w"], twin["clips"], twin["masks"], True, ragged=True)
        for k, i in enumerate(where):
            assert np.array_equal(mr.bits(rag[i]), mr.bits(got[k])), (name, wl, form, "ragged clip", i)
        for res, case in ((got, b), (rag, twin)):
            for r, ref, x in zip(res, case["refs"], case["clips"]):
                assert r.shape == ref.shape and np.isfinite(r).all(), (name, wl, form, len(x))
                for j in range(len(r)):
                    err = mc.mask_error(r[j], ref[j], mc.row_level(ref, x, j, tail))
                    worst[group] = max(worst[group], err)
                    assert err <= TOL_FFT, (name, wl, form, len(x), j, err)
        if form == "stems":   # stem s of clip k against the one-mask kind ("TF") under mask s alone
            for s in range(mc.N_STEMS):
                one = mr.run("tf", b["w"], b["clips"], [m[s] for m in b["masks"]], False, ragged=False)
                for k in range(len(one)):
                    assert np.array_equal(mr.bits(got[k][s]), mr.bits(one[k][0])), (name, wl, "stem", s, "clip", k)
        if form == "stereo2":   # channel c against the mono kind on the planar channel c under mask c: within the bound, not bitwise
            assert all(not np.array_equal(m[0], m[1]) for m in b["masks"])
            for c in (0, 1):
                mono = mr.run("tf", b["w"], [np.ascontiguousarray(x[:, c]) for x in b["clips"]], [m[c] for m in b["masks"]], True, ragged=False)
                for k, x in enumerate(b["clips"]):
                    for blk in (0, 1):   # y, the rest
                        level = max(float(np.abs(mono[k][blk]).max()), float(np.abs(x).max()))
                        err = float(np.abs(got[k][2 * blk + c].astype(np.float64) - mono[k][blk]).max()) / level
                        worst["maskfilter_stereo_vs_mono"] = max(worst["maskfilter_stereo_vs_mono"], err)
                        assert err <= TOL_FFT, (name, wl, "channel", c, "clip", k, "block", blk, err)
        if form in mc.PCM_FORMS:
            for ragged, case in ((False, b), (True, twin)):
                pcm = [mc.to_int16(x, 16384) for x in case["clips"]]
                ref32 = mr.run(form, case["w"], [mc.normalised(q) for q in pcm], case["masks"], True, ragged=ragged)
                as32 = mr.run_pcm(form, case["w"], pcm, case["masks"], True, ragged, np.float32)
                as16 = mr.run_pcm(form, case["w"], pcm, case["masks"], True, ragged, np.int16)
                for i, (q, f, p32, p16) in enumerate(zip(pcm, ref32, as32, as16)):
                    what = (name, wl, form, "ragged" if ragged else "equal-length", "clip", i)
                    assert p32.dtype == np.float32 and p32.shape == f.shape and np.array_equal(mr.bits(p32), mr.bits(f)), what
                    assert p16.dtype == np.int16 and np.array_equal(p16[:tail], numpy_quantise(f[:tail])), what
                    planar = q.T if q.ndim == 2 else q[None]   # (channels, N): the rows' order
                    assert np.array_equal(p16[tail:], int_rest(planar, p16[:tail])), what
    for group, err in worst.items():
        key = f"{group}.{name}"
        _report[key] = max(_report.get(key, 0.0), err)
    print(f"maskfilter {name} W={wl}: " + ", ".join(f"{g} {e:.3e}" for g, e in worst.items()))


# ------------------------------------------------------------------------------------------------------------------ the plan cache
def test_plans_of_one_geometry_with_different_windows_are_not_shared(zafx):
    """A window and its mirror image, one geometry: each call runs on a plan of its own window (the cache key hashes the taps)."""
    n = MDCT_2048[1]
    x = clips(n)
    w = win.skew(2048)
    for v in (w, w[::-1].copy(), w):
        got = zafx.mdct_batch(x, v)
        refs = [orc.mdct(c.astype(np.float64), v) for c in x]
        held("cache", "skew", got, refs, TOL_FFT, "mdct")
        back = zafx.imdct_batch(np.stack(refs), v)
        held("cache", "skew", back, [orc.imdct(r, v) for r in refs], TOL_FFT, "imdct")
        hop = 1024
        got = zafx.stft_batch(x[:, :stft_n(hop)], v, hop)
        held("cache", "skew", got, [orc.stft(c[:stft_n(hop)].astype(np.float64), v, hop) for c in x], TOL_FFT, "stft")
    assert zafx.mdct_plan(w, row_align=32) is not zafx.mdct_plan(w[::-1].copy(), row_align=32)
    assert zafx.stft_plan(w, 1024, row_align=16) is not zafx.stft_plan(w[::-1].copy(), 1024, row_align=16)
