"""GPU parity on signals that are not white noise (-m gpu): silence, DC, full-scale tones on and between bins, two tones
100 dB apart, impulses on hop boundaries, a chirp, noise at -90 dBFS, clipped int16 PCM (tests/signals.py), against the
outputs of the REAL reference (tests/golden/signals.npz) and, at a length that reaches the whole-tile kernels, against the
oracle.

Two bounds per output, both written here:
  * the contract's normwise bound per clip, max|out - ref| / max|ref| <= 1e-5 (stft, istft, mdct, imdct) / 1e-4 (mel, mfcc,
    cqt, chroma);
  * a bound per ROW (frequency bin, mel band, coefficient, CQT bin; a hop of samples for the 1-D outputs):
        |out - ref| <= 10 tol max_row|ref| + floor,
    so that a quiet row under a loud one is held to its own level.  `floor` is the float32 floor of the clip,
    C eps32 max|ref| -- what a float32 transform cannot resolve under the loudest value it handles (a tone's far bins are
    differences of partial sums as large as its peak) -- with C = 2 for the 2048-point frames and 8 for the CQT's
    32768-point frames (measured on MI355X, round 5: worst row at 0.37 / 0.66 of these bounds, DC through the CQT).
  * MFCCs (check_mfcc): the floor is the transform's error carried through log and DCT (conftest.mfcc_floor: bins at c eps sqrt(log2 W) of the
    frame's RMS spectrum, independent, root-sum-square through filterbank and DCT; + the pipeline's own roundings).  Where a mel band of the
    reference holds only the float64 transform's own round-off (DC, a tone exactly on a bin: bands at 1e-26 of the peak) the reference's
    coefficients are functions of that round-off and no float32 program reproduces them; the bound is then as wide as
    log(float32 floor / float64 floor), and it is asserted, not skipped.  The normwise 1e-4 is decided FRAME BY FRAME: every frame whose
    floor is below 1e-4 of the clip's peak is held to it (round 5 switched the whole clip off when one frame's floor was above).  Measured,
    float32, 70 frames: DC 0.62 and the tone on a bin 0.45 of the peak (every frame above), the chirp 1.9e-4 (its steepest frames; the others
    hold 1e-4), every other signal below 8e-6; in float64 (test_signal_in_float64_mel_mfcc_cqt) all of them hold 1e-10 but the tone on a
    bin (7e-9).  Silence has floor 0: every output must be exactly zero, and the MFCCs of silence, DCT(log(eps)) (zaf.py:444-446), may
    differ from the reference's 1e-14 by the rounding of a float32 dot product over 128 equal levels.

  * the fused mask filters (test_signal_through_the_mask_filters; tests/maskfilter_cases.py): mask_error <= 1e-5 and, per hop of H samples,
    |y - ref| <= 10 tol max_hop|ref| + 2 eps32 max(max|ref|, max|x|) -- the level with the input's peak, as mask_error takes it; silence and
    masks of zeros exact.  Two frames ride in one transform, so a quiet frame paired with a loud one inherits its rounding ("loud_quiet").
    Measured on MI355X: worst hop 0.20 of its bound (dc, sparse mask, W = 2048), loud_quiet 0.099 (the unpacked float32 chain: 0.003), worst
    normwise 5.2e-7.

Kernel forms.  The STFT / ISTFT / MDCT / IMDCT checks run in both row padding modes: "compact" (fixture `zafx`) keeps the reference's memory
order, so a frame count off the 128-byte line grid (T = 4, 71) runs the kernels' off-grid forms (k_stft_ft16c, the carry k_mdct_ft32, ...);
"auto" (fixture `zafx_padded`, the *_padded twin of each test), the *_batch default and the drop-ins' path, pads such rows to whole lines and
runs the plain forms (k_stft_ft16, ...).  T = 96 (N_GRID, test_signal_on_the_line_grid) is on the grid in both modes.  After every call the
kernel that ran is asserted against ROUTES, a table read off the dispatch code.  Mel / MFCC / CQT / chroma, the PCM entry points and the ragged
calls lay out their own rows whatever the mode is, and run once.
"""
import json
import os

import numpy as np
import pytest

import signals as sig
from center_oracle import assert_center_contract, oracle_center
from conftest import bin_noise, excess, mfcc_floor, relerr, row_bound
from oracle import zaf_oracle as orc

pytestmark = pytest.mark.gpu

TOL_FFT = 1e-5
TOL_FB = 1e-4
EPS32 = float(np.finfo(np.float32).eps)
C_FLOOR = 2.0
C_FLOOR_CQT = 8.0
N_LONG = 1024 * 69 + 300       # 70 frames: whole 16- / 32-frame tiles, an edge tile and rows off the line grid
N_GRID = 1024 * 94 + 300       # T = 96 STFT and MDCT frames: rows of whole 128-byte lines (16 complex64, 32 float32 elements) in either mode

_report = {}


@pytest.fixture(scope="module")
def zafx_lib():
    import zafx as z
    assert z.device_count() >= 1
    yield z
    z.set_row_padding("auto")
    path = os.environ.get("ZAFX_SIGNALS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_report, f, indent=1, sort_keys=True)


def _in_mode(z, mode):
    z.set_row_padding(mode)
    yield z
    z.set_row_padding("auto")


@pytest.fixture
def zafx(zafx_lib):
    """Row padding "compact": the reference's memory order -- the kernels' off-grid forms at T = 4 and 71.  (set_row_padding decides the device
    layout of the STFT / MDCT-family *_batch functions only, core._line_grid; mel / MFCC / CQT / chroma write their own rows, the *_pcm_batch
    functions run Plan.run_host_pcm on the compact plan and the ragged calls always pad to whole lines, core._ragged_grid: those run once.)"""
    yield from _in_mode(zafx_lib, "compact")


@pytest.fixture
def zafx_padded(zafx_lib):
    """Row padding "auto", the *_batch default: rows off the line grid padded to whole lines -- the plain forms."""
    yield from _in_mode(zafx_lib, "auto")


@pytest.fixture(params=["compact", "auto"])
def zafx_mode(request, zafx_lib):
    yield from _in_mode(zafx_lib, request.param)


@pytest.fixture(scope="module")
def consts(zafx_lib):
    zafx = zafx_lib
    ham, kbd = zafx.hamming(sig.W), zafx.kaiser_bessel_derived(sig.W)
    fb = zafx.melfilterbank(sig.FS, sig.W, 128)
    ck = zafx.cqtkernel(sig.FS, 24, 55, 3520)
    return ham, kbd, fb, ck


def full_spectrum(half):
    """Rows 0..W/2 -> the two-sided spectrum the reference returns (mirror rows = conjugates, see make_golden.py)."""
    return np.concatenate([half, np.conj(half[-2:0:-1])], axis=0)


def hops(y, hop=sig.HOP):
    """A 1-D output as rows of one hop each (zero-filled at the end)."""
    n = -(-len(y) // hop) * hop
    return np.pad(y, (0, n - len(y))).reshape(-1, hop)


def _forms(off_grid_compact, whole_lines):
    """{(mode, grid): kernel}: compact rows off the line grid take one form; rows padded to whole lines (mode "auto") or on the grid take the other."""
    return {("compact", "off"): off_grid_compact, ("auto", "off"): whole_lines, ("compact", "on"): whole_lines, ("auto", "on"): whole_lines}


# The kernel each STFT / MDCT-family call of this module runs, read off the dispatch code (zafx_stft.hip run_stft / run_istft, zafx_mel.hip
# launch_spec2, zafx_mdct.hip run_mdct / run_mdct_p / run_imdct, zafx_bs32.hip), not off last_kernel: a routing change must not move a test
# off the form it claims to cover.  (W, kind) -> {(mode, grid): kernel}; grid "on" = T is a whole number of 128-byte lines of the rows
# the kernel writes (forward) or reads (inverse): 16 complex64, 32 float32 elements.
ROUTES = {
    # W = 2048 (1024-point FFT): complex rows whose pitch is not a multiple of 16 on the carry form; whole lines on k_stft_ft16, the 32 x 32
    # radix-32 schedule (twiddle table d_tw_r32) with whole-line streaming stores
    (2048, "two_sided"): _forms("k_stft_ft16c", "k_stft_ft16"),
    (2048, "one_sided"): _forms("k_stft_ft16c", "k_stft_ft16"),
    # |X|, |X|^2: k_mel2 at every pitch; its store takes 4 frames per 16-byte piece at a pitch that is a multiple of 4 (every padded pitch,
    # T = 96), one frame otherwise (compact T = 71) -- zafx_mel.hip, rowv
    (2048, "magnitude"): _forms("k_mel2", "k_mel2"),
    (2048, "power"): _forms("k_mel2", "k_mel2"),
    (2048, "istft"): _forms("k_istft_ft16", "k_istft_ft16"),
    (2048, "istft_one_sided"): _forms("k_istft_ft16", "k_istft_ft16"),
    # k_mdct_ft32 names two forms (run_mdct_p): the carry instantiation when the row pitch is not a multiple of 16 floats (compact T = 4, 22,
    # 71), the plain one when it is (T = 96, every padded pitch)
    (2048, "mdct"): _forms("k_mdct_ft32", "k_mdct_ft32"),
    (2048, "imdct"): _forms("k_imdct", "k_imdct"),
    # W = 4096: complex rows off the grid on the one-band carry form, whole lines on the two-band kernel; |X| on the two-band kernel at any pitch
    (4096, "two_sided"): _forms("k_stft_ft16bc", "k_stft_ft16b"),
    (4096, "magnitude"): _forms("k_stft_ft16b", "k_stft_ft16b"),
    (4096, "istft"): _forms("k_istft_ft16d", "k_istft_ft16d"),   # hop W / 2: the two-class kernel (16-byte pieces of two frames at an even pitch)
    (4096, "mdct"): _forms("k_mdct_ft32bc", "k_mdct_ft32b"),     # a pitch that is not a multiple of 16 floats: the carry form
    (4096, "imdct"): _forms("k_imdct", "k_imdct"),
    # W = 8192: two-sided rows on the four-class kernel only as whole lines (compact off the grid: generic k_stft; the test's T = 48 is on it);
    # k_imdct_q at any pitch that is a multiple of 4 (48 compact, 64 padded)
    (8192, "two_sided"): _forms("k_stft", "k_stft_ft16q"),
    (8192, "magnitude"): _forms("k_stft_ft16q", "k_stft_ft16q"),
    (8192, "istft"): _forms("k_istft_ft8q", "k_istft_ft8q"),
    (8192, "mdct"): _forms("k_mdct_ft32q", "k_mdct_ft32q"),
    (8192, "imdct"): _forms("k_imdct_q", "k_imdct_q"),
    # W = 1000: the float32 Bluestein forms, one frame per workgroup at any pitch
    (1000, "two_sided"): _forms("k_stft_bs32", "k_stft_bs32"),
    (1000, "magnitude"): _forms("k_stft_bs32", "k_stft_bs32"),
    (1000, "istft"): _forms("k_ifft_frames_bs32", "k_ifft_frames_bs32"),
    (1000, "mdct"): _forms("k_mdct_bs32", "k_mdct_bs32"),
    (1000, "imdct"): _forms("k_imdct_frames_bs32", "k_imdct_frames_bs32"),
}
SPEC = {False: "two_sided", True: "one_sided", "magnitude": "magnitude", "power": "power"}


def assert_route(zafx, w, kind, t, line, plan_for, out=None):
    """The call just made on T = t frames ran ROUTES[(w, kind)] in the current mode.  plan_for(row_align) -> that plan family's plan: _line_grid
    takes the one padded to `line` elements in mode "auto" off the grid, else the compact one.  out: the forward result, whose row stride shows
    that the call ran on that plan."""
    mode = zafx.get_row_padding()
    grid = "off" if t % line else "on"
    padded = mode == "auto" and grid == "off"
    ran, want = plan_for(line if padded else 0).last_kernel, ROUTES[(w, kind)][(mode, grid)]
    assert ran == want, (w, kind, mode, grid, ran, want)
    if out is not None:
        pitch = -(-t // line) * line if padded else t
        assert out.strides[-2] == pitch * out.itemsize, (w, kind, mode, out.strides, pitch)


def check(tag, out, ref, tol, floor=None, c=C_FLOOR):
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape, (tag, out.shape, ref.shape)
    peak = float(np.abs(ref).max()) if ref.size else 0.0
    if floor is None:
        floor = c * EPS32 * peak
    g = relerr(out, ref)
    r = excess(out, ref, row_bound(ref, tol, floor))
    _report[tag] = {"normwise": g, "row_excess": r, "peak": peak}
    assert r <= 1.0, (tag, "row bound", r)
    return g


def check_mfcc(tag, out, ref, half, fbd):
    """The MFCC contract (docstring): every coefficient within 10 tol of its row's level + the float32 floor of its frame (conftest.mfcc_floor), and
    -- decided FRAME BY FRAME -- the normwise 1e-4 of the clip's peak in every frame whose floor is below it.  Frames above it are the ones
    float32 cannot hold (a band at the transform's round-off level under a loud one: DC, a tone on a bin, the steep part of a chirp); the
    report says how many there are and how much of its floor the worst coefficient used."""
    fl = mfcc_floor(half, fbd, 20, C_FLOOR, EPS32)
    g = check(tag, out, ref, TOL_FB, fl)
    peak = float(np.abs(ref).max())
    err = np.abs(np.asarray(out, dtype=np.float64) - ref)
    held = fl.max(axis=0) <= TOL_FB * peak          # frames the normwise contract binds
    worst_held = float(err[:, held].max() / peak) if held.any() and peak > 0 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        use = np.where(fl > 0, err / fl, 0.0)
    _report[tag].update({"floor_over_peak": float(fl.max() / max(peak, 1e-300)), "frames_held_to_tol": int(held.sum()), "frames": int(held.size),
                         "normwise_of_held_frames": worst_held, "error_over_floor": float(use.max())})
    if peak > 0:
        assert worst_held <= TOL_FB, (tag, "mfcc: a frame whose float32 floor is below 1e-4 of the peak", worst_held)
    return g


def run_all(zafx, consts, name, x, ref, label):
    """Every STFT / MDCT-family function of the path on one signal, in the current row padding mode, each call's kernel asserted (ROUTES).
    ref: dict of reference outputs (stft = rows 0..W/2)."""
    ham, kbd, fb, ck = consts
    mode = zafx.get_row_padding()
    tag = f"{mode}.{name}{label}"
    half = ref["stft"]
    t, tm = half.shape[1], ref["mdct"].shape[1]

    def stft_for(kind):
        return lambda a: zafx.stft_plan(ham, sig.HOP, onesided=kind, row_align=a)

    spec = zafx.stft_batch(x[None], ham, sig.HOP)[0]
    assert_route(zafx, sig.W, "two_sided", t, 16, stft_for(False), spec)
    assert spec.shape == (sig.W, half.shape[1])
    assert check(f"{tag}.stft", spec[: sig.W // 2 + 1], half, TOL_FFT) <= TOL_FFT
    assert check(f"{tag}.stft_mirror", spec[sig.W // 2 + 1:], np.conj(half[-2:0:-1]), TOL_FFT) <= TOL_FFT
    spec1 = zafx.stft_batch(x[None], ham, sig.HOP, onesided=True)[0]
    assert_route(zafx, sig.W, "one_sided", t, 16, stft_for(True), spec1)
    assert check(f"{tag}.stft_onesided", spec1, half, TOL_FFT) <= TOL_FFT
    for kind, p in (("magnitude", 1), ("power", 2)):
        lvl = np.abs(half) ** p
        # |X|^p of a bin carrying an absolute error nu: p |X|^(p-1) nu + nu^p
        nu = bin_noise(half, C_FLOOR, EPS32)
        fl = nu if p == 1 else 2 * np.abs(half) * nu + nu ** 2
        gotm = zafx.stft_batch(x[None], ham, sig.HOP, onesided=kind)[0]
        assert_route(zafx, sig.W, kind, t, 32, stft_for(kind), gotm)
        assert check(f"{tag}.stft_{kind}", gotm, lvl, TOL_FFT, fl) <= (TOL_FFT if p == 1 else 2 * TOL_FFT)

    y = zafx.istft_batch(full_spectrum(half)[None], ham, sig.HOP)[0]
    assert_route(zafx, sig.W, "istft", t, 16, lambda a: zafx.istft_plan(ham, sig.HOP, row_align=a))
    assert check(f"{tag}.istft", hops(y), hops(ref["istft"]), TOL_FFT) <= TOL_FFT
    assert len(y) == len(ref["istft"])
    y1 = zafx.istft_batch(half[None], ham, sig.HOP, onesided=True)[0]
    assert_route(zafx, sig.W, "istft_one_sided", t, 16, lambda a: zafx.istft_plan(ham, sig.HOP, onesided=True, row_align=a))
    assert len(y1) == len(ref["istft"])
    assert check(f"{tag}.istft_onesided", hops(y1), hops(ref["istft"]), TOL_FFT) <= TOL_FFT

    coefs = zafx.mdct_batch(x[None], kbd)[0]
    assert_route(zafx, sig.W, "mdct", tm, 32, lambda a: zafx.mdct_plan(kbd, row_align=a), coefs)
    assert check(f"{tag}.mdct", coefs, ref["mdct"], TOL_FFT) <= TOL_FFT
    yi = zafx.imdct_batch(ref["mdct"][None], kbd)[0]
    assert_route(zafx, sig.W, "imdct", tm, 32, lambda a: zafx.mdct_plan(kbd, inverse=True, row_align=a))
    assert len(yi) == len(ref["imdct"])
    assert check(f"{tag}.imdct", hops(yi), hops(ref["imdct"]), TOL_FFT) <= TOL_FFT

    if mode == "auto":
        # the drop-ins run *_batch in the default mode and hand back its result -- a view of the padded rows -- cast to complex128 / float64
        assert np.array_equal(zafx.stft(x, ham, sig.HOP), spec.astype(np.complex128))
        assert np.array_equal(zafx.istft(full_spectrum(half), ham, sig.HOP), y.astype(np.float64))
        assert np.array_equal(zafx.mdct(x, kbd), coefs.astype(np.float64))
        assert np.array_equal(zafx.imdct(ref["mdct"], kbd), yi.astype(np.float64))


def run_filterbanks(zafx, consts, name, x, xq, ref, label):
    """Mel / MFCC (and with xq, CQT / chroma) on one signal: outputs whose rows the row padding mode does not lay out."""
    ham, kbd, fb, ck = consts
    fbd = fb.toarray()
    tag = f"{name}{label}"
    half = ref["stft"]
    # mel bands: FB |X| with every bin off by at most nu
    nu = bin_noise(half, C_FLOOR, EPS32)
    mel_floor = fbd @ np.broadcast_to(nu, (fbd.shape[1], nu.shape[1])) + C_FLOOR * EPS32 * np.abs(ref["mel"])
    got = zafx.melspectrogram_batch(x[None], ham, sig.HOP, fb)[0]
    assert check(f"{tag}.mel", got, ref["mel"], TOL_FB, mel_floor) <= TOL_FB
    got = zafx.mfcc_batch(x[None], ham, sig.HOP, fb, 20)[0]
    check_mfcc(f"{tag}.mfcc", got, ref["mfcc"], half, fbd)

    if xq is not None:
        got = zafx.cqtspectrogram_batch(xq[None], sig.FS, 25, ck)[0]
        assert check(f"{tag}.cqt", got, ref["cqt"], TOL_FB, c=C_FLOOR_CQT) <= TOL_FB
        got = zafx.cqtchromagram_batch(xq[None], sig.FS, 25, 24, ck)[0]
        assert check(f"{tag}.chroma", got, ref["chroma"], TOL_FB, c=C_FLOOR_CQT) <= TOL_FB


def golden_refs(golden, name):
    g = golden["signals"]
    x, xq = sig.signal(name, sig.N_FRAMES), sig.signal(name, sig.N_CQT)
    assert float(x.astype(np.float64).sum()) == g[f"{name}_x_sum"] and float(np.abs(xq.astype(np.float64)).sum()) == g[f"{name}_xq_abs"]
    return x, xq, {k: g[f"{name}_{k}"] for k in ("stft", "istft", "mel", "mfcc", "mdct", "imdct", "cqt", "chroma")}


@pytest.mark.parametrize("name", sig.NAMES)
def test_signal_against_the_reference(zafx, consts, golden, name):
    """n = 3072 / 17640 samples: the reference's own outputs."""
    x, xq, ref = golden_refs(golden, name)
    run_all(zafx, consts, name, x, ref, "")
    run_filterbanks(zafx, consts, name, x, xq, ref, "")


@pytest.mark.parametrize("name", sig.NAMES)
def test_signal_against_the_reference_padded(zafx_padded, consts, golden, name):
    """n = 3072 samples (T = 4) on rows padded to whole lines: the reference's own outputs."""
    x, xq, ref = golden_refs(golden, name)
    run_all(zafx_padded, consts, name, x, ref, "")


def oracle_refs(consts, x):
    ham, kbd, fb, ck = consts
    x64 = x.astype(np.float64)
    s = orc.stft(x64, ham, sig.HOP)
    m = orc.mdct(x64, kbd)
    return {"stft": s[: sig.W // 2 + 1], "istft": orc.istft(s, ham, sig.HOP), "mel": orc.melspectrogram(x64, ham, sig.HOP, fb),
            "mfcc": orc.mfcc(x64, ham, sig.HOP, fb, 20), "mdct": m, "imdct": orc.imdct(m, kbd)}


@pytest.mark.parametrize("name", sig.NAMES)
def test_signal_on_the_whole_tile_kernels(zafx, consts, name):
    """70 frames (the tiled kernels' interior path, an edge tile, rows off the line grid) against the oracle, which
    tests/test_oracle_golden.py holds to the reference on these very signals."""
    x = sig.signal(name, N_LONG)
    ref = oracle_refs(consts, x)
    run_all(zafx, consts, name, x, ref, "_long")
    run_filterbanks(zafx, consts, name, x, None, ref, "_long")


@pytest.mark.parametrize("name", sig.NAMES)
def test_signal_on_the_whole_tile_kernels_padded(zafx_padded, consts, name):
    """The same 70 frames on rows padded to whole lines (k_stft_ft16, the plain k_mdct_ft32, k_mel2 at 4 frames per store)."""
    x = sig.signal(name, N_LONG)
    run_all(zafx_padded, consts, name, x, oracle_refs(consts, x), "_long")


@pytest.mark.parametrize("name", sig.NAMES)
def test_signal_on_the_line_grid(zafx_mode, consts, name):
    """96 frames: rows of whole lines without padding -- the plain forms in compact mode too."""
    x = sig.signal(name, N_GRID)
    run_all(zafx_mode, consts, name, x, oracle_refs(consts, x), "_grid")


def test_silence_is_exact(zafx, consts):
    """Digital silence: every linear output is exactly zero (no denormal dust, no -0.0 that a log would turn into nan)."""
    silence_is_exact(zafx, consts)


def test_silence_is_exact_padded(zafx_padded, consts):
    silence_is_exact(zafx_padded, consts)


def silence_is_exact(zafx, consts):
    ham, kbd, fb, ck = consts
    x = np.zeros((2, N_LONG), dtype=np.float32)
    assert not np.any(zafx.stft_batch(x, ham, sig.HOP))
    assert not np.any(zafx.stft_batch(x, ham, sig.HOP, onesided="power"))
    assert not np.any(zafx.melspectrogram_batch(x, ham, sig.HOP, fb))
    assert not np.any(zafx.mdct_batch(x, kbd))
    assert not np.any(zafx.cqtspectrogram_batch(x[:, :40000], sig.FS, 25, ck))
    c = zafx.mfcc_batch(x, ham, sig.HOP, fb, 20)
    assert np.all(np.isfinite(c))
    # DCT rows 1..20 of 128 equal levels log(eps) = -36.04: zero up to the rounding of a float32 dot product
    assert np.abs(c).max() <= 8.0 * EPS32 * 36.05 * np.sqrt(128.0)


@pytest.mark.parametrize("channels", [1, 2])
def test_clipped_pcm_through_the_pcm_entry_points(zafx, consts, golden, channels):
    """Full-scale clipped int16 (zaf.py:1202 scales by 2**15, :65 averages the channels) straight into the *_pcm_batch forms."""
    ham, kbd, fb, ck = consts
    g = golden["signals"]
    pcm = sig.clipped_pcm16(sig.N_FRAMES)
    assert pcm.min() == -32768 and pcm.max() == 32767
    p = pcm[None, :, None] if channels == 1 else np.stack([pcm, pcm], axis=-1)[None]
    p = np.ascontiguousarray(p)
    half = g["clipped_pcm_stft"]
    got = zafx.stft_pcm_batch(p, ham, sig.HOP)[0]
    assert check(f"pcm{channels}.stft", got[: sig.W // 2 + 1], half, TOL_FFT) <= TOL_FFT
    assert check(f"pcm{channels}.mel", zafx.melspectrogram_pcm_batch(p, ham, sig.HOP, fb)[0], g["clipped_pcm_mel"], TOL_FB) <= TOL_FB
    check_mfcc(f"pcm{channels}.mfcc", zafx.mfcc_pcm_batch(p, ham, sig.HOP, fb, 20)[0], g["clipped_pcm_mfcc"], half, fb.toarray())
    assert check(f"pcm{channels}.mdct", zafx.mdct_pcm_batch(p, kbd)[0], g["clipped_pcm_mdct"], TOL_FFT) <= TOL_FFT
    pq = sig.clipped_pcm16(sig.N_CQT)
    pq = np.ascontiguousarray(pq[None, :, None] if channels == 1 else np.stack([pq, pq], axis=-1)[None])
    assert check(f"pcm{channels}.cqt", zafx.cqtspectrogram_pcm_batch(pq, sig.FS, 25, ck)[0], g["clipped_pcm_cqt"], TOL_FB, c=C_FLOOR_CQT) <= TOL_FB


@pytest.mark.parametrize("name", sig.NAMES)
@pytest.mark.parametrize("wl,hop", [(4096, 2048), (2048, 512), (1000, 250), (8192, 4096)])
def test_signal_on_the_other_kernels(zafx, name, wl, hop):
    """The same signals through the kernels the W = 2048 / hop 1024 cases do not reach -- the two-band forms of W = 4096 (k_stft_ft16b / bc,
    k_istft_ft16d, k_mdct_ft32b / bc, k_mel_ft16b), 75 % overlap, a window that is not a power of two (the Bluestein forms), the four-class
    forms of W = 8192 (k_stft_ft16q, k_mdct_ft32q and, round 6, their inverses k_istft_ft8q, k_imdct_q; 48 frames: rows on the line grid) -- against the
    oracle with the same two bounds, each call's kernel asserted (ROUTES)."""
    other_kernels(zafx, name, wl, hop)


@pytest.mark.parametrize("name", sig.NAMES)
@pytest.mark.parametrize("wl,hop", [(4096, 2048), (2048, 512), (1000, 250), (8192, 4096)])
def test_signal_on_the_other_kernels_padded(zafx_padded, name, wl, hop):
    """The same on rows padded to whole lines (k_stft_ft16b, k_mdct_ft32b, k_stft_ft16, ...)."""
    other_kernels(zafx_padded, name, wl, hop)


def other_kernels(zafx, name, wl, hop):
    n = 40 * hop + 300 if wl != 8192 else 47 * hop - 100
    x = sig.signal(name, n)
    x64 = x.astype(np.float64)
    ham = zafx.hamming(wl)
    s = orc.stft(x64, ham, hop)
    half = s[: wl // 2 + 1]
    t = s.shape[1]
    tag = f"{zafx.get_row_padding()}.{name}_{wl}_{hop}"
    got = zafx.stft_batch(x[None], ham, hop)[0]
    assert_route(zafx, wl, "two_sided", t, 16, lambda a: zafx.stft_plan(ham, hop, row_align=a), got)
    assert check(f"{tag}.stft", got, s, TOL_FFT) <= TOL_FFT
    y = zafx.istft_batch(s[None], ham, hop)[0]
    assert_route(zafx, wl, "istft", t, 16, lambda a: zafx.istft_plan(ham, hop, row_align=a))
    yref = orc.istft(s, ham, hop)
    assert len(y) == len(yref) and relerr(y, yref) <= TOL_FFT
    assert check(f"{tag}.istft", hops(y, hop), hops(yref, hop), TOL_FFT) <= TOL_FFT
    nu = bin_noise(half, C_FLOOR, EPS32)
    gotm = zafx.stft_batch(x[None], ham, hop, onesided="magnitude")[0]
    assert_route(zafx, wl, "magnitude", t, 32, lambda a: zafx.stft_plan(ham, hop, onesided="magnitude", row_align=a), gotm)
    assert check(f"{tag}.magnitude", gotm, np.abs(half), TOL_FFT, nu) <= TOL_FFT
    if wl % 2 == 0:
        kbd = zafx.kaiser_bessel_derived(wl) if wl & (wl - 1) == 0 else zafx.sine(wl)
        m = orc.mdct(x64, kbd)
        coefs = zafx.mdct_batch(x[None], kbd)[0]
        assert_route(zafx, wl, "mdct", m.shape[1], 32, lambda a: zafx.mdct_plan(kbd, row_align=a), coefs)
        assert check(f"{tag}.mdct", coefs, m, TOL_FFT) <= TOL_FFT
        yi, yiref = zafx.imdct_batch(m[None], kbd)[0], orc.imdct(m, kbd)
        assert_route(zafx, wl, "imdct", m.shape[1], 32, lambda a: zafx.mdct_plan(kbd, inverse=True, row_align=a))
        assert len(yi) == len(yiref) and relerr(yi, yiref) <= TOL_FFT
        assert check(f"{tag}.imdct", hops(yi, wl // 2), hops(yiref, wl // 2), TOL_FFT) <= TOL_FFT
    fb = zafx.melfilterbank(sig.FS, wl, 64)
    fbd = fb.toarray()
    mel_floor = fbd @ np.broadcast_to(nu, (fbd.shape[1], nu.shape[1])) + C_FLOOR * EPS32 * np.abs(orc.melspectrogram(x64, ham, hop, fb))
    assert check(f"{tag}.mel", zafx.melspectrogram_batch(x[None], ham, hop, fb)[0], orc.melspectrogram(x64, ham, hop, fb), TOL_FB, mel_floor) <= TOL_FB


@pytest.mark.parametrize("name", sig.NAMES)
def test_signal_in_float64(zafx, consts, name):
    """The float64 mode (the reference's own dtype) on the same signals: 1e-12 normwise on the tiled kernels of W = 2048
    (k_stft_ft8_f64, k_mdct_ft16_f64) and on the inverse transforms; silence stays exactly zero.  (The padded twin: rows of whole lines of 8
    complex128 / 16 float64 elements.)"""
    signal_in_float64(zafx, consts, name)


@pytest.mark.parametrize("name", sig.NAMES)
def test_signal_in_float64_padded(zafx_padded, consts, name):
    signal_in_float64(zafx_padded, consts, name)


def signal_in_float64(zafx, consts, name):
    ham, kbd, fb, ck = consts
    x64 = sig.signal(name, N_LONG).astype(np.float64)
    s = orc.stft(x64, ham, sig.HOP)
    got = zafx.stft_batch(x64[None], ham, sig.HOP, f64=True)[0]
    m = orc.mdct(x64, kbd)
    gotm = zafx.mdct_batch(x64[None], kbd, f64=True)[0]
    if name == "silence":
        assert not np.any(got) and not np.any(gotm)
        return
    assert relerr(got, s) <= 1e-12 and relerr(gotm, m) <= 1e-12
    # per row: a row above 1e-9 of the peak is held to 1e-9 of its own level
    rows = np.abs(s).max(axis=1)
    live = rows > 1e-9 * rows.max()
    assert np.all(np.abs(got - s).max(axis=1)[live] <= 1e-9 * rows[live])
    assert relerr(zafx.istft_batch(s[None], ham, sig.HOP, f64=True)[0], orc.istft(s, ham, sig.HOP)) <= 1e-12
    assert relerr(zafx.imdct_batch(m[None], kbd, f64=True)[0], orc.imdct(m, kbd)) <= 1e-12


@pytest.mark.parametrize("name", sig.NAMES)
def test_signal_in_float64_mel_mfcc_cqt(zafx, consts, name):
    """melspectrogram / mfcc / cqtspectrogram / cqtchromagram in float64 (k_mel_ft8_f64, k_cqt_ft_f64) on the same signals: 1e-12 normwise for the
    linear outputs, and the MFCCs -- the outputs float32 cannot hold on tonal material (module docstring; the chirp: 1.9e-4) -- to 1e-10 with NO
    floor (measured: chirp 2.8e-13, DC 1.5e-14, every other signal below 1.1e-14) wherever the reference's own coefficients are reproducible at
    all.  They are not for a full-scale tone exactly on a bin: its far bands, at 1e-26 of the peak, hold nothing but the round-off of the
    reference's own transform -- any second float64 program (NumPy's FFT called on the whole batch instead of frame by frame is one) moves those
    coefficients by some 1e-9 (measured here: 7.1e-9) --, so that one signal is held to the same interval arithmetic as in float32 with
    float64's epsilon, asserted."""
    ham, kbd, fb, ck = consts
    x64 = sig.signal(name, N_LONG).astype(np.float64)
    xq64 = sig.signal(name, sig.N_CQT * 3).astype(np.float64)
    mel = zafx.melspectrogram_batch(x64[None], ham, sig.HOP, fb, f64=True)[0]
    assert zafx.mel_plan(ham, sig.HOP, fb, f64=True).last_kernel == "k_mel_ft8_f64"
    cep = zafx.mfcc_batch(x64[None], ham, sig.HOP, fb, 20, f64=True)[0]
    cq = zafx.cqtspectrogram_batch(xq64[None], sig.FS, 25, ck, f64=True)[0]
    assert zafx.cqt_plan(sig.FS, 25, ck, f64=True).last_kernel == "k_cqt_ft_f64"
    ch = zafx.cqtchromagram_batch(xq64[None], sig.FS, 25, 24, ck, f64=True)[0]
    if name == "silence":
        assert not np.any(mel) and not np.any(cq) and not np.any(ch)
        assert np.abs(cep).max() <= 64 * np.finfo(float).eps * 36.05 * np.sqrt(128.0)   # DCT rows 1..20 of 128 equal levels log(eps)
        return
    ref_mel, ref_cep = orc.melspectrogram(x64, ham, sig.HOP, fb), orc.mfcc(x64, ham, sig.HOP, fb, 20)
    ref_cq, ref_ch = orc.cqtspectrogram(xq64, sig.FS, 25, ck), orc.cqtchromagram(xq64, sig.FS, 25, 24, ck)
    assert relerr(mel, ref_mel) <= 1e-12 and relerr(cq, ref_cq) <= 1e-12 and relerr(ch, ref_ch) <= 1e-12
    g = relerr(cep, ref_cep)
    _report[f"{name}_f64.mfcc"] = {"normwise": g}
    if name == "sine_bin":
        half = orc.stft(x64, ham, sig.HOP)[: sig.W // 2 + 1]
        fl = mfcc_floor(half, fb.toarray(), 20, C_FLOOR, float(np.finfo(float).eps))
        assert excess(cep, ref_cep, fl) <= 1.0, (name, g)
    else:
        assert g <= 1e-10, (name, g)


# the nine signals as one ragged batch, every clip of its own length (0 and 1 samples, T = 4, 71 and 96 at W = 2048); silence and the
# -90 dBFS noise each sit between two full-scale clips, so that a tile reading past its clip, or taking a neighbour's base, shows
RAGGED = (("dc", 0), ("clipped_pcm", N_LONG), ("silence", N_GRID), ("sine_bin", 44100), ("noise_m90", sig.N_FRAMES), ("two_tones", 2 * sig.W + 1),
          ("impulse", 1), ("chirp", 1024 * 40 + 7), ("sine_half", 16 * sig.HOP + 3))
KINDS = [False, True, "magnitude", "power"]
ZERO_MFCC = 8.0 * EPS32 * 36.05 * np.sqrt(128.0)   # (test_silence_is_exact: DCT rows 1..20 of 128 equal levels log(eps))


def ragged_clips():
    assert len({n for _, n in RAGGED}) == len(RAGGED) and {name for name, _ in RAGGED} == set(sig.NAMES)
    return [sig.signal(name, n) for name, n in RAGGED]


@pytest.mark.parametrize("wl,hop", [(2048, 1024), (1024, 256)])
def test_signals_in_one_ragged_batch(zafx_lib, wl, hop):
    """stft_ragged of the nine signals, every spectrum kind (k_stft_ft16_ragged; |X| / |X|^2 at W = 2048: k_mel2_ragged; W = 1024 two-sided, where
    the equal-length path runs the carry form) against the oracle clip by clip with run_all's bounds; a clip of zeros comes out exactly zero."""
    zafx = zafx_lib
    clips = ragged_clips()
    ham = zafx.hamming(wl)
    specs = [orc.stft(c.astype(np.float64), ham, hop) for c in clips]
    for kind in KINDS:
        got = zafx.stft_ragged(clips, ham, hop, onesided=kind)
        line = 16 if kind in (False, True) else 32
        want = "k_mel2_ragged" if wl == 2048 and kind in ("magnitude", "power") else "k_stft_ft16_ragged"
        assert zafx.stft_plan(ham, hop, onesided=kind, row_align=line).last_kernel == want, kind
        assert len(got) == len(clips)
        for (name, n), x, g, s in zip(RAGGED, clips, got, specs):
            tag = f"ragged.{name}_{n}_{wl}_{hop}.stft_{SPEC[kind]}"
            half = s[: wl // 2 + 1]
            if not np.any(x):
                assert g.shape == (s.shape[0] if kind is False else half.shape[0], s.shape[1]) and not np.any(g), tag
            if kind is False:
                assert check(tag, g, s, TOL_FFT) <= TOL_FFT
            elif kind is True:
                assert check(tag, g, half, TOL_FFT) <= TOL_FFT
            else:
                p = 1 if kind == "magnitude" else 2
                nu = bin_noise(half, C_FLOOR, EPS32)
                fl = nu if p == 1 else 2 * np.abs(half) * nu + nu ** 2
                assert check(tag, g, np.abs(half) ** p, TOL_FFT, fl) <= p * TOL_FFT


def test_signals_in_one_ragged_batch_mel_mfcc(zafx_lib, consts):
    """melspectrogram_ragged / mfcc_ragged / mel_mfcc_ragged (k_mel2_ragged) of the nine signals at W = 2048 against the oracle clip by clip with
    run_all's bounds; the mel bands of a clip of zeros are exactly zero, its MFCCs those of test_silence_is_exact."""
    zafx = zafx_lib
    ham, kbd, fb, ck = consts
    fbd = fb.toarray()
    clips = ragged_clips()
    mel = zafx.melspectrogram_ragged(clips, ham, sig.HOP, fb)
    assert zafx.mel_plan(ham, sig.HOP, fb, row_align=32).last_kernel == "k_mel2_ragged"
    cep = zafx.mfcc_ragged(clips, ham, sig.HOP, fb, 20)
    assert zafx.mel_plan(ham, sig.HOP, fb, 20, row_align=32).last_kernel == "k_mel2_ragged"
    both_mel, both_cep = zafx.mel_mfcc_ragged(clips, ham, sig.HOP, fb, 20)
    assert zafx.mel_plan(ham, sig.HOP, fb, 20, row_align=32, also_mel=True).last_kernel == "k_mel2_ragged"
    for i, ((name, n), x) in enumerate(zip(RAGGED, clips)):
        x64 = x.astype(np.float64)
        half = orc.stft(x64, ham, sig.HOP)[: sig.W // 2 + 1]
        ref_mel, ref_cep = orc.melspectrogram(x64, ham, sig.HOP, fb), orc.mfcc(x64, ham, sig.HOP, fb, 20)
        nu = bin_noise(half, C_FLOOR, EPS32)
        mel_floor = fbd @ np.broadcast_to(nu, (fbd.shape[1], nu.shape[1])) + C_FLOOR * EPS32 * np.abs(ref_mel)
        for form, m, c in (("", mel[i], cep[i]), ("_one_pass", both_mel[i], both_cep[i])):
            tag = f"ragged.{name}_{n}{form}"
            if not np.any(x):
                assert m.shape == ref_mel.shape and not np.any(m), tag
                assert np.all(np.isfinite(c)) and np.abs(c).max() <= ZERO_MFCC, tag
            assert check(f"{tag}.mel", m, ref_mel, TOL_FB, mel_floor) <= TOL_FB
            check_mfcc(f"{tag}.mfcc", c, ref_cep, half, fbd)


# ------------------------------------------------------------------------------------------------ center / sides and the ragged MDCT / IMDCT launches
TOL_ROUND_TRIP = 1e-5   # |imdct(mdct(x)) - x| on unit-variance noise, absolute (tests/test_gpu_mdct_ragged.py)
CENTER_SHAPES = [(2048, sig.N_FRAMES), (2048, N_LONG), (256, 128 * 69 + 37)]   # (W, N): 4 frames; several 4-frame tiles, a carry and an edge tile; 8-frame tiles


def center_last_kernel(zafx, w, sides):
    return zafx.center_plan(w, sides=sides).last_kernel


@pytest.mark.parametrize("name", sig.STEREO_NAMES)
@pytest.mark.parametrize("wl,n", CENTER_SHAPES)
def test_stereo_signal_through_k_center(zafx_lib, wl, n, name):
    """The center mask -- the library's most non-linear arithmetic: squared magnitudes, one v_rcp_f32 and one v_sqrt_f32 per bin, a clamp at the
    smallest normal number, a departure from the reference at 0 / 0 (zafx_center.hpp) -- on the eleven stereo signals of tests/signals.py, both
    kinds (ZAFX_CENTER_SIDES and ZAFX_CENTER) of k_center, against center_oracle.oracle_center.  Bounds (center_oracle.assert_center_contract):
    finite; silence exactly zero; center <= 1e-5 normwise (left_only, whose reference is identically zero: max|center| <= 1e-5 max|x|); sides
    <= 1e-5 max|x|; per hop of H samples per channel |out - ref| <= 10 * 1e-5 max_hop|ref| + C eps32 max|x| with C = 16 -- the smallest
    power of two that leaves the float32 host emulation at or below half the bound (tests/test_center_host.py: its worst hop is left_only at
    W = 2048, 0.353 of the bound; the other half is the device's 1-ulp rcp and sqrt).
    Measured on MI355X (66 results): worst normwise 9.88e-07 (pan_tones_2048_70956.center), worst hop 0.360 of its bound (left_only_2048_70956.center),
    worst sides 9.88e-07 of max|x| (pan_tones_2048_70956.sides)."""
    zafx = zafx_lib
    w = zafx.hamming(wl)
    x = sig.stereo_signal(name, n)
    ref = oracle_center(x, w)
    c, s = zafx.centersides_batch(x[None], w)
    assert center_last_kernel(zafx, w, True) == "k_center"
    assert_center_contract(f"k_center.{name}_{wl}_{n}.sides", c[0], s[0], x, ref, wl // 2, _report)
    only = zafx.centersides_batch(x[None], w, sides=False)
    assert center_last_kernel(zafx, w, False) == "k_center"
    assert_center_contract(f"k_center.{name}_{wl}_{n}.center", only[0], None, x, ref, wl // 2, _report)
    assert np.array_equal(only[0].view(np.uint32), c[0].view(np.uint32))


@pytest.mark.parametrize("wl", [2048, 256])
def test_center_below_the_smallest_normal(zafx_lib, wl):
    """The clamp in center_ratio (zafx_center.hpp), which none of the eleven signals reaches -- it takes |X| < 1e-19 --: the `gain` signal at 1e-23,
    whose squared magnitudes are all denormal.  v_rcp_f32 takes a denormal for zero, so without the clamp the mask is lo * inf.  With it the
    mask is only too small (lo / FLT_MIN < 1 for lo < hi < FLT_MIN), the right channel's mask stays 1, and the result is finite and no larger
    than the input's peak.  The normwise bound does not apply: below the smallest normal number the mask's value is not the reference's."""
    zafx = zafx_lib
    w = zafx.hamming(wl)
    x = sig.stereo_signal("gain", 128 * 69 + 37) * np.float32(1e-23)
    peak = float(np.abs(x).max())
    assert peak > 1e-24 and (peak * wl) ** 2 < np.finfo(np.float32).tiny
    c, s = zafx.centersides_batch(x[None], w)
    assert center_last_kernel(zafx, w, True) == "k_center"
    _report[f"k_center.gain_1e-23_{wl}"] = {"finite": bool(np.isfinite(c).all()), "max_over_peak": float(np.nanmax(np.abs(c))) / peak}
    assert np.isfinite(c).all() and np.isfinite(s).all()
    assert float(np.abs(c).max()) <= peak


def stereo_ragged_lengths(h, f):
    """One length per stereo signal, 1 sample frame ... 70 hops: a clip of 1, one that ends a tile exactly (2 f h), the others around hops."""
    hopsof = {"silence": 3 * h + 7, "dc": 1, "pan_tones": 70 * h - 5, "gain": 2 * f * h, "anti": 9 * h + h // 2, "tones_chirp": 33 * h, "impulse": 5 * h - 1,
              "noise_m90": 17 * h + 1, "clipped": 48 * h + 3, "loud_quiet": 64 * h + 300, "left_only": 25 * h + 11}
    assert set(hopsof) == set(sig.STEREO_NAMES) and len(set(hopsof.values())) == 11 and max(hopsof.values()) <= 70 * h
    return [hopsof[name] for name in sig.STEREO_NAMES]


@pytest.mark.parametrize("sides", [True, False], ids=["center_sides", "center"])
@pytest.mark.parametrize("wl", [2048, 256])
def test_stereo_signals_in_one_ragged_batch(zafx_lib, wl, sides):
    """k_center_ragged: the eleven stereo signals in ONE centersides_ragged call, each of its own length (1 sample frame ... 70 hops, one ending a
    tile exactly), packed back to back -- silence beside DC, the -90 dBFS noise between the impulses and the clipped sine -- clip by clip under
    test_stereo_signal_through_k_center's bounds.
    Measured on MI355X (44 results): worst normwise 9.85e-07 (pan_tones_2048_71675.center), worst hop 0.361 of its bound (left_only_2048_25611.center),
    worst sides 9.88e-07 of max|x| (pan_tones_2048_71675.sides)."""
    zafx = zafx_lib
    w, h = zafx.hamming(wl), wl // 2
    lengths = stereo_ragged_lengths(h, zafx.center_tile_frames(wl))
    clips = [sig.stereo_signal(name, n) for name, n in zip(sig.STEREO_NAMES, lengths)]
    res = zafx.centersides_ragged(clips, w, sides=sides)
    assert center_last_kernel(zafx, w, sides) == "k_center_ragged"
    assert len(res) == len(clips)
    for name, n, x, r in zip(sig.STEREO_NAMES, lengths, clips, res):
        c, s = r if sides else (r, None)
        assert_center_contract(f"k_center_ragged.{name}_{wl}_{n}.{'sides' if sides else 'center'}", c, s, x, oracle_center(x, w), h, _report)


# one length per mono signal, every one a multiple of 4 (mdct_ragged packs the clips on 128-byte lines: the 16-byte-load form); `odd` adds 1, 2
# or 3 samples (the 4-byte form).  T = ceil(n / M) + 1: one tile, tile edges (31 M, 33 M) and several tiles at M = 1024 and at M = 256.
MDCT_RAGGED = (("silence", 4100), ("dc", 20), ("sine_bin", 1024 * 40), ("sine_half", 16 * 1024 + 4), ("two_tones", 2 * sig.W + 8), ("impulse", 3 * 1024 + 4),
               ("chirp", 1024 * 31), ("noise_m90", sig.N_FRAMES), ("clipped_pcm", 1024 * 33 + 12))


def mdct_ragged_clips(odd):
    assert tuple(name for name, _ in MDCT_RAGGED) == sig.NAMES and not any(n % 4 for _, n in MDCT_RAGGED)
    lengths = [n + (1, 2, 3)[i % 3] * odd for i, (_, n) in enumerate(MDCT_RAGGED)]
    assert all(n % 4 for n in lengths) if odd else True
    return lengths, [sig.signal(name, n) for (name, _), n in zip(MDCT_RAGGED, lengths)]


@pytest.mark.parametrize("lengths_are", ["multiples_of_4", "odd"])
@pytest.mark.parametrize("wl", [2048, 512])
def test_signals_in_one_ragged_mdct_batch(zafx_lib, wl, lengths_are):
    """k_mdct_ft32_ragged (both load forms) on the nine mono signals in one mdct_ragged call at KBD 2048 and KBD 512, every clip against orc.mdct
    with the per-row bound and C_FLOOR, exactly as the equal-length run_all; a clip of zeros comes out exactly zero.  Both forms report the one
    kernel name: which one runs follows from the launcher's rule (zafx_execute_ragged: 16-byte loads when d_in is on 16 bytes and every offset
    and length is a multiple of 4) and from how mdct_ragged packs -- a fresh allocation, every clip on a 32-element slot (asserted on
    pack_ragged below).  This is a test of VALUES: the packing pads with zeros, so a read past a clip's end is invisible here; that is
    tests/test_gpu_arena.py::test_mdct_ragged's, where NaNs lie between the clips.
    Measured on MI355X (36 results): worst normwise 2.05e-07 (multiples_of_4.chirp_31744_2048.mdct), worst row 0.238 of its bound
    (multiples_of_4.clipped_pcm_33804_2048.mdct)."""
    zafx = zafx_lib
    kbd = zafx.kaiser_bessel_derived(wl)
    lengths, clips = mdct_ragged_clips(lengths_are == "odd")
    _, in_off, lens = zafx.pack_ragged(clips)
    assert not (in_off % 4).any() and bool((lens % 4).any()) == (lengths_are == "odd")   # (the launcher's condition for the 16-byte form, or not)
    got = zafx.mdct_ragged(clips, kbd)
    assert zafx.mdct_plan(kbd, row_align=32).last_kernel == "k_mdct_ft32_ragged"
    assert len(got) == len(clips)
    for (name, _), n, x, g in zip(MDCT_RAGGED, lengths, clips, got):
        ref = orc.mdct(x.astype(np.float64), kbd)
        if not np.any(x):
            assert g.shape == ref.shape and not np.any(g), name
        assert check(f"k_mdct_ft32_ragged.{lengths_are}.{name}_{n}_{wl}.mdct", g, ref, TOL_FFT) <= TOL_FFT


@pytest.mark.parametrize("wl", [2048, 512])
def test_signals_in_one_ragged_imdct_batch(zafx_lib, wl):
    """k_imdct_ragged: the oracle's MDCT blocks of the nine signals in one imdct_ragged call, against orc.imdct per hop of W / 2 samples with the
    per-row bound (run_all's imdct check); then the round trip mdct_ragged -> imdct_ragged of each signal, the views fed as they lie, within
    TOL_ROUND_TRIP absolute -- for noise_m90 scaled by that signal's level, 10^(-90/20): the bound is DESIGN 1's for unit-variance noise, the
    other signals are at full scale.
    Measured on MI355X (18 results): worst normwise 5.36e-07 (clipped_pcm_33807_512.imdct), worst hop 0.234 of its bound (impulse_3079_2048.imdct).  Round
    trip: worst 2.91e-11 against 3.16e-10 (noise_m90_3074_2048.round_trip)."""
    zafx = zafx_lib
    kbd, m = zafx.kaiser_bessel_derived(wl), wl // 2
    lengths, clips = mdct_ragged_clips(True)
    blocks = [orc.mdct(x.astype(np.float64), kbd) for x in clips]
    got = zafx.imdct_ragged(blocks, kbd)
    inverse = zafx.mdct_plan(kbd, inverse=True, row_align=32)
    assert inverse.last_kernel == "k_imdct_ragged"
    for (name, _), n, b, y in zip(MDCT_RAGGED, lengths, blocks, got):
        ref = orc.imdct(b, kbd)
        assert len(y) == len(ref)
        if not np.any(b):
            assert not np.any(y), name
        assert check(f"k_imdct_ragged.{name}_{n}_{wl}.imdct", hops(y, m), hops(ref, m), TOL_FFT) <= TOL_FFT
    spectra = zafx.mdct_ragged(clips, kbd)
    assert zafx.mdct_plan(kbd, row_align=32).last_kernel == "k_mdct_ft32_ragged"
    keep = [min(n, max(m * (s.shape[1] - 1) - 1, 0)) for n, s in zip(lengths, spectra)]
    assert keep == lengths   # (no length is a whole number of hops: every sample comes back)
    back = zafx.imdct_ragged(spectra, kbd, lengths=keep)
    assert inverse.last_kernel == "k_imdct_ragged"
    for (name, _), n, x, y in zip(MDCT_RAGGED, lengths, clips, back):
        assert y.shape == x.shape
        err = float(np.max(np.abs(y.astype(np.float64) - x)))
        bound = TOL_ROUND_TRIP * (10.0 ** (-90.0 / 20.0) if name == "noise_m90" else 1.0)   # (the one signal far below unit level: held to its own)
        _report[f"k_imdct_ragged.{name}_{n}_{wl}.round_trip"] = {"max_abs": err, "bound": bound}
        assert err <= bound, (name, n, err, bound)


# ------------------------------------------------------------------------------------------------------------------ the fused mask filters
def maskfilter_rows(tag, res, case, h):
    """Every stem and the rest of every clip: mask_error <= TOL_FFT and the per-hop bound of tests/maskfilter_cases.hop_share, whose level takes
    max|x| as mask_error's does.  The figures go into the report before they are asserted."""
    import maskfilter_cases as mc
    for i, (r, ref, x) in enumerate(zip(res, case["refs"], case["clips"])):
        assert r.shape == ref.shape and np.isfinite(r).all(), (tag, i)
        for j in range(len(r)):
            g, share = mc.mask_error(r[j], ref[j], x), mc.hop_share(r[j], ref[j], x, h)
            _report[f"maskfilter/{tag}.clip{i}.row{j}"] = {"normwise": g, "hop_share": share, "peak": float(np.abs(ref[j]).max())}
            assert g <= TOL_FFT, (tag, i, j, "normwise", g)
            assert share <= 1.0, (tag, i, j, "hop bound", share)
        if not np.any(x):
            assert not np.any(r), (tag, i, "silence must give exact zeros, the rest included")


@pytest.mark.parametrize("name", sig.NAMES + ("loud_quiet",))
@pytest.mark.parametrize("wl", [2048, 256])
def test_signal_through_the_mask_filters(zafx_lib, wl, name):
    """k_maskfilter ("TF" and "FT" compact), k_maskfilter_stems (S = 2: "uniform" and "sparse"), k_maskfilter_complex ("disc") and the ragged twin
    of each, the rest on, on a clip of 20 H + 9 samples of every signal and on "loud_quiet" -- unit noise in front of noise at -90 dB, where the
    frame pair across the step rides in ONE transform and the quiet frame inherits the loud one's rounding.  Bounds: mask_error <= TOL_FFT and,
    per hop of H samples, |y - ref| <= 10 TOL_FFT max_hop|ref| + C_FLOOR eps32 max(max|ref|, max|x|) (tests/test_accuracy_host.py holds the
    unpacked float32 chain to half of it on the same inputs); silence gives exact zeros.  The ragged launch gives the full-length clips the
    bits of the equal-length one."""
    import maskfilter_cases as mc
    import maskfilter_run as mr
    assert name in mc.SIGNAL_NAMES and wl in mc.SIGNAL_WINDOWS and mc.C_FLOOR == C_FLOOR and mc.TOL_FFT == TOL_FFT
    case = mc.signal_case(name, wl)
    for form in mc.SIGNAL_FORMS:
        c = case[mc.family_of(form)]
        same = {k: [c[k][i] for i in c["equal"]] for k in ("clips", "masks", "refs")}
        got = mr.run(form, case["w"], same["clips"], same["masks"], True, ragged=False)
        rag = mr.run(form, case["w"], c["clips"], c["masks"], True, ragged=True)
        for k, i in enumerate(c["equal"]):
            assert np.array_equal(mr.bits(rag[i]), mr.bits(got[k])), (name, wl, form, "ragged clip", i)
        maskfilter_rows(f"{form}.{name}_{wl}", got, same, wl // 2)
        maskfilter_rows(f"{form}_ragged.{name}_{wl}", rag, c, wl // 2)


@pytest.mark.parametrize("wl", [2048, 256])
def test_stems_of_zero_masks(zafx_lib, wl):
    """Masks of zeros in every stem: every stem is exact zeros and the rest has the bits of x -- equal-length and ragged (the one-mask kinds:
    tests/test_gpu_maskfilter.py::test_zeros, tests/test_gpu_maskfilter_complex.py::test_fixed_values)."""
    import maskfilter_cases as mc
    import maskfilter_run as mr
    h = wl // 2
    w = mc.window_of("hamming", wl)
    clips = [mc.clip(k, n) for k, n in enumerate((20 * h + 9, 7 * h + 3, 20 * h + 9))]
    masks = [np.zeros((mc.N_STEMS, h + 1, mc.mask_frames(len(x), wl)), np.float32) for x in clips]
    for res, xs in ((mr.run("stems", w, clips[::2], masks[::2], True, ragged=False), clips[::2]), (mr.run("stems", w, clips, masks, True, ragged=True), clips)):
        for r, x in zip(res, xs):
            assert r.shape == (mc.N_STEMS + 1, len(x)) and not r[:mc.N_STEMS].any(), (wl, len(x))
            assert np.array_equal(mr.bits(r[mc.N_STEMS]), mr.bits(x)), (wl, len(x), "rest")


def stereo_maskfilter_rows(tag, res, case, h):
    """Every channel of y and of the rest of every stereo clip: mask_error <= TOL_FFT, the level over both channels, and the per-hop bound of
    tests/maskfilter_cases.hop_share_stereo -- max_hop|ref| per channel, the floor's level over both.  The figures go into the report before
    they are asserted; silence gives exact zeros."""
    import maskfilter_cases as mc
    for i, (r, ref, x) in enumerate(zip(res, case["refs"], case["clips"])):
        assert r.shape == ref.shape == (4, len(x)) and np.isfinite(r).all(), (tag, i)
        figures = []
        for j in (0, 2):
            shares = mc.hop_share_stereo(r[j:j + 2], ref[j:j + 2], x, h)
            for c in (0, 1):
                g = mc.mask_error(r[j + c], ref[j + c], mc.row_level(ref, x, j + c, 2))
                talk = float(np.abs(r[j + c].astype(np.float64) - ref[j + c]).max()) / max(float(np.abs(x).max()), 1e-300)
                _report[f"maskfilter/{tag}.clip{i}.row{j + c}"] = {"normwise": g, "hop_share": shares[c], "peak": float(np.abs(ref[j + c]).max()),
                                                                  "error_of_the_loud_level": talk}
                figures.append((j + c, g, shares[c]))
        for row, g, share in figures:
            assert g <= TOL_FFT, (tag, i, row, "normwise", g)
            assert share <= 1.0, (tag, i, row, "hop bound", share)
        if not np.any(x):
            assert not np.any(r), (tag, i, "silence must give exact zeros, the rest included")


@pytest.mark.parametrize("name", sig.STEREO_NAMES)
@pytest.mark.parametrize("wl", [2048, 256])
def test_stereo_signal_through_the_mask_filters(zafx_lib, wl, name):
    """k_maskfilter_stereo under one mask ("uniform") and under one per channel ("uniform" on L, "sparse" on R) and its ragged twin, the rest
    on, on every stereo signal at 20 H + 9 sample frames and its first 7 H + 3: left_only -- a silent channel in the same transform as a loud
    one, whose every figure is reported --, loud_quiet, tones, DC, an impulse.  Bounds: mask_error <= TOL_FFT and hop_share_stereo <= 1
    (tests/test_accuracy_host.py holds the unpacked chain to half of it and a float32 model of the packing to it on the same inputs);
    silence gives exact zeros.  The ragged launch gives the full-length clip the bits of the equal-length one.

    The same signals through the PCM kernels, quantised to rint(16384 x) -- half of full scale, so that the reference alone stays inside the
    int16 range under masks in [0, 1], asserted on the host before the launch: float32 out has the bits of the float kernel on the clip / 32768,
    int16 out is held to |y_q - 32768 ref| <= 0.5 + 32768 (the per-hop bound)."""
    import maskfilter_cases as mc
    import maskfilter_run as mr
    assert wl in mc.SIGNAL_WINDOWS and mc.C_FLOOR == C_FLOOR and mc.TOL_FFT == TOL_FFT
    h = wl // 2
    case = mc.stereo_signal_case(name, wl)
    for form in mc.STEREO_SIGNAL_FORMS:
        c = case[form]
        same = {k: [c[k][i] for i in c["equal"]] for k in ("clips", "masks", "refs")}
        got = mr.run(form, case["w"], same["clips"], same["masks"], True, ragged=False)
        rag = mr.run(form, case["w"], c["clips"], c["masks"], True, ragged=True)
        for k, i in enumerate(c["equal"]):
            assert np.array_equal(mr.bits(rag[i]), mr.bits(got[k])), (name, wl, form, "ragged clip", i)
        stereo_maskfilter_rows(f"{form}.{name}_{wl}", got, same, h)
        stereo_maskfilter_rows(f"{form}_ragged.{name}_{wl}", rag, c, h)
        # int16 PCM: the references of the quantised clips, in range before anything is launched
        pcm = [mc.to_int16(x, 16384) for x in c["clips"]]
        norm = [mc.normalised(q) for q in pcm]
        refs = [mc.reference(form, xn, case["w"], m) for xn, m in zip(norm, c["masks"])]
        bounds = [mc.int16_bound(ref[:2], xn, h) for xn, ref in zip(norm, refs)]
        for ref, bound in zip(refs, bounds):
            assert (np.abs(32768.0 * ref[:2]) + bound < 32767).all(), (name, wl, form, "the reference leaves the int16 range")
        for ragged in (False, True):
            pick = list(c["equal"]) if not ragged else list(range(len(pcm)))
            sel = lambda v: [v[i] for i in pick]   # noqa: E731
            f32 = mr.run(form, case["w"], sel(norm), sel(c["masks"]), True, ragged=ragged)
            p32 = mr.run_pcm(form, case["w"], sel(pcm), sel(c["masks"]), True, ragged, np.float32)
            p16 = mr.run_pcm(form, case["w"], sel(pcm), sel(c["masks"]), True, ragged, np.int16)
            for i, a, b, q in zip(pick, f32, p32, p16):
                tag = f"{form}_pcm{'_ragged' if ragged else ''}.{name}_{wl}.clip{i}"
                assert np.array_equal(mr.bits(a), mr.bits(b)), (tag, "float32 out against the float kernel")
                share = excess(q[:2].astype(np.float64), 32768.0 * refs[i][:2], bounds[i])
                _report[f"maskfilter/{tag}"] = {"int16_share": share}
                assert share <= 1.0, (tag, "int16 out against the oracle", share)
                if not np.any(pcm[i]):
                    assert not np.any(q) and not np.any(b), (tag, "silence")
