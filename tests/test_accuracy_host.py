"""The yardstick, the reference and the checker of tests/test_gpu_accuracy.py, held to account on the CPU (no GPU, no library):

  * tests/plain.py at float64 restates the pinned oracle (<= 1e-12) for every operation at every geometry of the two catalogues and of the
    cases added in tests/accuracy_cases.py; at long double it does too, and lies 1e-16 ... 1e-15 (rms) from its float64 run -- it is a
    wider computation, and not a wrong one;
  * the float32 yardstick is a single-precision computation (its error grows with the length; np.fft's does not: it computes in double);
  * the checker (tests/accuracy.py) fails two doctored results that the 1e-5 contract passes;
  * the FFT core of zafx_fft.hpp, emulated on the host (tests/host_emu/fft_emu.cpp), is within K_RMS of the yardstick at every size;
  * the fused mask filters (tests/maskfilter_cases.py): plain.maskfilter* restates the oracle's composition; the unpacked float32 chain keeps
    half the per-hop bound of tests/test_gpu_signals.py on every signal it is asked of; a NumPy float32 model of the kernels' packed
    arithmetic stays inside the family factors, and with one defect at a time -- the window read at its periodic mirror, bin H's mask taken
    from bin H - 1, the packed spectrum rounded to 16 mantissa bits -- it is caught by the new checks where the 1e-5 bound cannot see it."""
import os
import subprocess

import numpy as np
import pytest
import scipy.fft

import accuracy as acc
import accuracy_cases as ac
import const_probe as cp
import maskfilter_cases as mc
import plain
import route_cases as rc
import signals as sig
from conftest import relerr
from oracle import zaf_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
WIDER = (1e-16, 1e-15)   # e_rms of the long-double run against the float64 run: a transform's own rounding


def mfcc_condition(x, consts, hop):
    """The MFCC's rows 1 .. n are orthogonal to the constant, so the common level of the log-mel values (about 14 for unit noise, log(eps) =
    -36 in an empty band) drops out of the coefficients -- while every product and every partial sum of D @ logs is rounded at the level of
    |D| @ |logs|.  The textbook bound of an inner product, |fl(d . l) - d . l| <= gamma_n |d| . |l|, makes || |D| @ |logs| || / || D @ logs ||
    the factor by which a correct float64 MFCC may lie further from the exact one than a transform does (whose own factor is 1: unitary).
    Computed from the long-double run alone; the upper end of WIDER is held times this factor, the lower end and TOL as they are."""
    logs = plain.logmel(x, consts["window"], hop, consts["fb"], np.longdouble)
    d = np.asarray(consts["dct"], np.longdouble)
    return max(float(np.sqrt((np.matmul(np.abs(d), np.abs(logs)) ** 2).sum() / (np.matmul(d, logs) ** 2).sum())), 1.0)


def rms(a, b):
    return acc.measure(a, b, hop=1)["e_rms"]


def held(f64, wide, oracle, tag, condition=1.0):
    """f64, wide, oracle: the clips' results by plain at float64, at long double, and by the oracle."""
    assert len(f64) == len(wide) == len(oracle)
    worst = max(max(relerr(np.asarray(a, b.dtype), b), relerr(np.asarray(w, b.dtype), b)) for a, w, b in zip(f64, wide, oracle))
    flat = lambda v: [np.asarray(a).reshape(-1) for a in v]
    apart = rms(flat(f64), flat(wide))
    print(f"{tag}: float64 and long double within {worst:.3g} of the oracle, {apart:.3g} apart (rms); condition {condition:.3g}")
    assert all(np.asarray(w).dtype in (np.longdouble, np.complex256) for w in wide)
    assert worst <= TOL, (tag, worst)
    assert WIDER[0] <= apart <= WIDER[1] * condition, (tag, apart, condition)


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("route", ac.PROBE_ROUTES + sorted(ac.ADDED_PROBES))
def test_plain_restates_the_oracle_on_the_constants_catalogue(route):
    case = cp.case(route) if route in cp.ROUTES else ac.ADDED_PROBES[route]()
    cond = mfcc_condition(case.data, case.consts, case.kw["step_length"]) if case.kind == "MFCC" and not case.kw["with_mel"] else 1.0
    held(ac.probe_plain(case, np.float64), ac.probe_plain(case, np.longdouble), case.refs(None), route, cond)


def route_geometries():
    """The distinct transforms of tests/route_cases.py (the addresses, row pitches and layouts of its 92 calls do not reach the arithmetic)."""
    seen = {}
    for name, c in rc.CASES.items():
        key = (c["family"], c["W"], c["hop"], c["spectrum"], c["frames"], c["short"], c["filters"], c["ncoef"], c["pcm"])
        seen.setdefault(key, name)
    return sorted(seen.values())


@pytest.mark.parametrize("name", route_geometries())
def test_plain_restates_the_oracle_on_the_call_catalogue(name):
    c = dict(rc.CASES[name], layout="FT", row_align=0)
    n_in = c["frames"] if rc.is_inverse(c) else rc.samples(c)
    if c["pcm"]:
        x = rc.noise(7, (rc.N_CLIPS, n_in), np.int16)
    elif rc.is_inverse(c):
        rows = c["W"] // 2 if c["family"] == "imdct" else c["W"] // 2 + 1 if c["spectrum"] else c["W"]
        x = rc.noise(7, (rc.N_CLIPS * rows * n_in,), np.float32 if c["family"] == "imdct" else np.complex64)
    else:
        x = rc.noise(7, (rc.N_CLIPS * n_in,), np.float32)
    x = ac.route_input(c, x, n_in)
    consts = ac.route_consts(c)
    cond = mfcc_condition(x, consts, c["hop"]) if c["family"] == "mfcc" else 1.0
    held(ac.route_plain(c, x, np.float64, consts), ac.route_plain(c, x, np.longdouble, consts), ac.route_reference(c, x, consts), name, cond)


@pytest.mark.parametrize("n", ac.DCT_LENGTHS)
def test_plain_restates_the_oracle_dct_and_dst(n):
    x = ac.dct_input(n)
    for sine in (False, True):
        for t in (1, 2, 3, 4):
            held(ac.dct_plain(x, t, sine, np.float64), ac.dct_plain(x, t, sine, np.longdouble), ac.dct_reference(x, t, sine), f"{'dst' if sine else 'dct'}{t}_{n}")


def test_the_roots_do_not_come_from_a_double_pi():
    """exp(-2 pi i k / n) at long double against the exact octant symmetries (which a double pi breaks at 1e-16) and against float64."""
    n = 4096
    z = plain.roots(np.arange(n), n, np.longdouble)
    assert z.dtype == np.complex256
    eps = float(np.finfo(np.longdouble).eps)
    assert float(np.abs(np.abs(z) - 1).max()) < 4 * eps
    assert float(np.abs(z[n // 8].real + z[n // 8].imag).max()) < 2 * eps            # cos(pi / 4) == sin(pi / 4)
    assert float(np.abs(z[n // 2] + 1)) < 2 * eps and float(np.abs(z[n // 4] + 1j)) < 2 * eps
    assert float(np.abs(plain.roots(np.arange(n), n, np.float64) - z).max()) < 1.2e-16   # one rounding of each part
    z32 = plain.roots(np.arange(n), n, np.float32)
    assert z32.dtype == np.complex64 and np.array_equal(z32, plain.roots(np.arange(n), n, np.float64).astype(np.complex64))
    # a large numerator is reduced in integers: no angle is ever above 2 pi
    assert np.array_equal(plain.roots(np.arange(n) + 1000 * n, n, np.longdouble), z)


# ------------------------------------------------------------------------------------------------ the yardstick is single precision
def fft_error(transform, n, frames=16):
    g = np.random.default_rng([31, n])
    x = (g.standard_normal((frames, n)) + 1j * g.standard_normal((frames, n))).astype(np.complex64)
    ref = scipy.fft.fft(x.astype(np.complex256), axis=-1)
    return rms([np.asarray(transform(x)).reshape(-1)], [ref.reshape(-1)])


def test_the_yardstick_is_single_precision():
    short, long_ = fft_error(plain.fft, 256, 64), fft_error(plain.fft, 16384, 4)
    numpy_short, numpy_long = fft_error(np.fft.fft, 256, 64), fft_error(np.fft.fft, 16384, 4)
    print(f"scipy.fft complex64: {short:.3g} at 256, {long_:.3g} at 16384; np.fft.fft (cast back to complex64): "
          f"{fft_error(lambda a: np.fft.fft(a).astype(np.complex64), 256, 64):.3g}, {fft_error(lambda a: np.fft.fft(a).astype(np.complex64), 16384, 4):.3g}"
          f"; np.fft.fft as returned: {numpy_short:.3g}, {numpy_long:.3g}")
    assert plain.fft(np.zeros(8, np.complex64)).dtype == np.complex64
    assert long_ > short > 5e-8
    # and the wider ones are what they say: float64 at 2e-16 ... 3e-16 of the long-double result
    g = np.random.default_rng(32)
    x = g.standard_normal((4, 2048)) + 1j * g.standard_normal((4, 2048))
    wide = plain.fft(x.astype(np.complex256))
    assert wide.dtype == np.complex256
    assert 1e-16 < rms([plain.fft(x).reshape(-1)], [wide.reshape(-1)]) < 5e-16


# ------------------------------------------------------------------------------------------------ the checker
@pytest.fixture(scope="module")
def stft_pair():
    """W = 2048, 2 clips x 33 frames: the oracle and a plain float32 result."""
    w, hop = 2048, 1024
    x = cp.clips_of(55, 32 * hop - 3)
    window = cp.window_a(w)
    ref = list(orc.stft_batch(x.astype(np.float64), window, hop))
    yard = list(plain.stft(x, window, hop, np.float32))
    assert ref[0].shape == (w, 33)
    return ref, yard


def test_the_checker_passes_a_second_plain_result(stft_pair):
    ref, yard = stft_pair
    same = acc.measure(yard, ref)
    assert acc.over(same, same, acc.factors()) == []
    assert 5e-8 < same["e_rms"] < 3e-7


def test_the_checker_fails_one_scaled_row(stft_pair):
    ref, yard = stft_pair
    bad = [y.copy() for y in yard]
    for b in bad:
        b[700] *= np.float32(1 + 3e-6)
    k, y = acc.measure(bad, ref), acc.measure(yard, ref)
    print(acc.line("one row times 1 + 3e-6", "-", k, y))
    assert max(relerr(b.astype(np.complex128), r) for b, r in zip(bad, ref)) < 1e-5
    assert "e_row" in acc.over(k, y, acc.factors())
    assert "e_row" in acc.over(k, y, acc.factors(bluestein=True))


def test_the_checker_fails_noise_on_every_element(stft_pair):
    ref, yard = stft_pair
    g = np.random.default_rng(77)
    bad = [(y * (1 + 1e-6 * g.standard_normal(y.shape))).astype(np.complex64) for y in yard]
    k, y = acc.measure(bad, ref), acc.measure(yard, ref)
    print(acc.line("relative noise 1e-6", "-", k, y))
    assert max(relerr(b.astype(np.complex128), r) for b, r in zip(bad, ref)) < 1e-5
    assert "e_rms" in acc.over(k, y, acc.factors())
    assert "e_rms" in acc.over(k, y, acc.factors(bluestein=True))


def test_the_metrics_on_a_one_dimensional_result():
    """Rows are the positions n mod hop, columns the hop-long blocks: an error in one block shows in e_col, one at a position in e_row."""
    g = np.random.default_rng(5)
    ref = [g.standard_normal(1000), g.standard_normal(1000)]
    block = [r.copy() for r in ref]
    block[1][300:400] *= 1.01
    m = acc.measure(block, ref, hop=100)
    assert abs(m["e_col"] - 0.01) < 1e-12 and m["e_row"] < 0.01 and m["e_rms"] < 0.01
    pos = [r.copy() for r in ref]
    for p in pos:
        p[7::100] *= 1.01
    m = acc.measure(pos, ref, hop=100)
    assert abs(m["e_row"] - 0.01) < 1e-12 and m["e_col"] < 0.01
    assert acc.measure(ref, ref, hop=100) == dict.fromkeys(acc.METRICS, 0.0)
    assert acc.factors(bluestein=True) == {"e_max": 6.0, "e_rms": 4.0, "e_row": 6.0, "e_col": 6.0}
    assert all(1 < f <= acc.MAX_FACTOR and cause for f, cause in ac.OWN_FACTORS.values())


# ------------------------------------------------------------------------------------------------ the FFT core
@pytest.fixture(scope="module")
def fft_emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fft_emu") / "fft_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-DZAFX_HOST_EMU", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "fft_emu.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_fft_core_is_as_accurate_as_a_plain_transform(fft_emu, tmp_path):
    """Every (log2n, log2e) tests/host_emu/fft_emu.cpp lists: the emulated core on >= 32768 points of complex64 noise against scipy.fft on the
    same frames, both measured against the long-double transform.  (Measured: 0.99 ... 1.07.)"""
    sizes = [tuple(map(int, ln.split())) for ln in subprocess.run([fft_emu, "--sizes"], capture_output=True, text=True, check=True).stdout.split("\n") if ln]
    assert len(sizes) >= 12 and (11, 4) in sizes and (14, 4) in sizes
    worst = 0.0
    for log2n, log2e in sizes:
        n = 1 << log2n
        frames = max(32768 // n, 4)
        g = np.random.default_rng([41, log2n, log2e])
        x = (g.standard_normal((frames, n)) + 1j * g.standard_normal((frames, n))).astype(np.complex64)
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        x.tofile(src)
        subprocess.run([fft_emu, str(log2n), str(log2e), str(src), str(dst)], check=True, capture_output=True)
        got = np.fromfile(dst, np.complex64).reshape(frames, n)
        ref = scipy.fft.fft(x.astype(np.complex256), axis=-1)
        core, yard = rms([got.reshape(-1)], [ref.reshape(-1)]), rms([plain.fft(x).reshape(-1)], [ref.reshape(-1)])
        print(f"log2n={log2n} log2e={log2e}: core {core:.3g}, yardstick {yard:.3g}, ratio {core / yard:.2f}")
        assert yard > 5e-8
        assert core <= acc.K_RMS * yard, (log2n, log2e, core, yard)
        worst = max(worst, core / yard)
    print(f"worst ratio {worst:.2f}")


CHAIN_CAUSE = "const/chroma_8192"   # (the case whose own factor stands for this core in tests/accuracy_cases.OWN_FACTORS)


def test_chained_core_loses_what_its_cases_are_granted(fft_emu, tmp_path):
    """k_cqt's transforms below 32768 points take every twiddle from a two-level root table and a product tree (pass_write_chain:
    w^r = w^(r / 2) w^(r - r / 2), r < 16): w^r carries r times the rounding of w, where a pass table holds one rounded root.  That is the cause
    named for the CQT cases' own factor; here the core alone, emulated, is held to that factor (measured 1.26 / 1.72 / 2.56 / 4.28 at 256 /
    512 / 2048 / 4096 points, the tabled core 1.00), and it must be a real loss: above K_RMS at 4096 points, or the factor has no cause."""
    sizes = [tuple(map(int, ln.split())) for ln in subprocess.run([fft_emu, "--chain-sizes"], capture_output=True, text=True, check=True).stdout.split("\n") if ln]
    assert (12, 4) in sizes
    own = ac.OWN_FACTORS[CHAIN_CAUSE][0]
    seen = {}
    for log2n, log2e in sizes:
        n = 1 << log2n
        frames = max(32768 // n, 4)
        g = np.random.default_rng([41, log2n, log2e])
        x = (g.standard_normal((frames, n)) + 1j * g.standard_normal((frames, n))).astype(np.complex64)
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        x.tofile(src)
        subprocess.run([fft_emu, "chain", str(log2n), str(log2e), str(src), str(dst)], check=True, capture_output=True)
        got = np.fromfile(dst, np.complex64).reshape(frames, n)
        ref = scipy.fft.fft(x.astype(np.complex256), axis=-1)
        k, y = acc.measure([got.T], [ref.T]), acc.measure([plain.fft(x).T], [ref.T])
        print(acc.line(f"chained core {n}", "-", k, y))
        assert acc.over(k, y, acc.factors(own=own)) == [], (log2n, acc.ratios(k, y))
        seen[log2n] = acc.ratios(k, y)["e_rms"]
    assert seen[12] > acc.K_RMS, seen


# ------------------------------------------------------------------------------------------------ the fused mask filters
@pytest.mark.parametrize("wl", mc.WINDOWS)
def test_plain_restates_the_oracle_mask_filter(wl):
    """plain.maskfilter / _complex / _stems at float64 and at long double against the oracle's composition, real, stems and complex masks."""
    n = 9 * (wl // 2) + 5
    for family in ("real", "stems", "complex"):
        x, w = mc.clip(3, n), mc.window_of("hamming", wl)
        m = mc.masks_for(family, wl, n, 3, "signed_wide")
        ref = mc.reference(family, x, w, m)
        runs = {}
        for dtype in (np.float64, np.longdouble):
            if family == "complex":
                y = plain.maskfilter_complex(x, w, m, dtype)
                runs[dtype] = np.stack([y, x.astype(dtype) - y])
            else:
                runs[dtype] = plain.maskfilter_stems(x, w, m if family == "stems" else m[None], dtype, rest=True)
        assert runs[np.float64].shape == ref.shape and runs[np.longdouble].dtype == np.longdouble
        held(list(runs[np.float64]), list(runs[np.longdouble]), list(ref), f"maskfilter {family} W={wl}")


def test_the_mask_filter_yardstick_keeps_half_the_hop_bound():
    """The per-hop bound of tests/test_gpu_signals.py::test_signal_through_the_mask_filters is a condition on the kernels, so its inputs are
    held here first: the unpacked float32 chain stays within 0.5 of it on every (signal, mask, W) used -- a failure on the GPU then points at
    the kernel, not at the input.  (Measured: worst 0.16, sine_bin under the sparse mask at W = 2048; the packed model 0.27, dc, sparse,
    W = 256; on loud_quiet 0.003 unpacked and 0.11 packed: the quiet frame paired with a loud one inherits its rounding.)"""
    worst, packed = (-1.0, ()), (-1.0, ())
    for wl in mc.SIGNAL_WINDOWS:
        h = wl // 2
        for name in mc.SIGNAL_NAMES:
            case = mc.signal_case(name, wl)
            for family in ("real", "stems", "complex"):
                c = case[family]
                for i, (yard, ref, x) in enumerate(zip(c["yard"], c["refs"], c["clips"])):
                    for j in range(len(ref)):
                        share = mc.hop_share(yard[j], ref[j], x, h)
                        worst = max(worst, (share, (name, wl, family, i, j)))
                        assert share <= 0.5 and mc.mask_error(yard[j], ref[j], x) <= mc.TOL_FFT, (name, wl, family, i, j, share)
                    if not np.any(x):
                        assert not np.any(yard), (name, wl, family)
            c = case["real"]
            for i, (m, ref, x) in enumerate(zip(c["masks"], c["refs"], c["clips"])):
                share = mc.hop_share(mc.packed_model(x, case["w"], m), ref[0], x, h)
                packed = max(packed, (share, (name, wl, i)))
                assert share <= 1.0, (name, wl, i, share)
    print(f"worst share of the hop bound: unpacked {worst[0]:.3f} {worst[1]}, packed model {packed[0]:.3f} {packed[1]}")


def _model_batch(b, defect):
    return [mc.packed_model(x, b["w"], m, defect)[None] for x, m in zip(b["clips"], b["masks"])]


def _model_errors(b, got):
    return max(mc.mask_error(g[0], r[0], x) for g, r, x in zip(got, b["refs"], b["clips"]))


def _model_judged(b, got, h):
    k = acc.measure(mc.all_rows(got), mc.rows_of(b["refs"], False), h)
    y = acc.measure(mc.rows_of(b["yard"], False), mc.rows_of(b["refs"], False), h)
    return k, y


@pytest.mark.parametrize("wl", mc.WINDOWS)
def test_the_packed_model_is_within_the_family_factors(wl):
    """Two frames in one transform, the split and the re-pack, in NumPy float32: within the family's factors of the unpacked yardstick on the
    catalogue's own batches (measured 0.79 ... 1.21 in the four metrics) -- the factors leave room for the packing and for nothing else."""
    for blocks in mc.BLOCKS:
        b = mc.batch("real", wl, blocks * (wl // 2) + 5, rotate=mc.WINDOWS.index(wl) + mc.BLOCKS.index(blocks))
        k, y = _model_judged(b, _model_batch(b, None), wl // 2)
        print(acc.line(f"packed model W={wl} T={blocks + 2}", "-", k, y))
        assert acc.over(k, y, acc.factors()) == [], acc.ratios(k, y)


@pytest.mark.parametrize("wl", [256, 2048])
def test_the_new_checks_see_what_the_old_bound_cannot(wl):
    """One defect at a time in the packed model, through the checks of the GPU modules:
      * the window read at (W - n) % W: past TOL_FFT under `skew` (tests/test_gpu_windows.py::test_maskfilter) -- and, under periodic Hamming,
        the bits of the sound model: no earlier mask-filter test could see it;
      * bin H's mask taken from bin H - 1: past TOL_FFT;
      * Z rounded to 16 mantissa bits before the split: inside TOL_FFT, outside the accuracy factors (tests/test_gpu_accuracy.py)."""
    h = wl // 2
    ham, skew = mc.batch("real", wl, 20 * h + 9, "hamming", "unit"), mc.batch("real", wl, 20 * h + 9, "skew", "unit")
    sound = _model_batch(ham, None)
    assert _model_errors(ham, sound) <= mc.TOL_FFT and _model_errors(skew, _model_batch(skew, None)) <= mc.TOL_FFT
    mirrored = _model_batch(ham, "window_mirror")
    assert all(np.array_equal(a, b) for a, b in zip(mirrored, sound))
    assert _model_errors(skew, _model_batch(skew, "window_mirror")) >= 0.05
    assert _model_errors(ham, _model_batch(ham, "bin_h")) > mc.TOL_FFT
    b = mc.batch("real", wl, 61 * h + 5, rotate=0)
    rounded = _model_batch(b, "round16")
    k, y = _model_judged(b, rounded, h)
    print(acc.line(f"Z at 16 mantissa bits, W={wl}", "-", k, y))
    assert _model_errors(b, rounded) <= mc.TOL_FFT
    assert set(acc.over(k, y, acc.factors())) == set(acc.METRICS), acc.ratios(k, y)
    assert acc.over(*_model_judged(b, _model_batch(b, None), h), acc.factors()) == []


# ------------------------------------------------------------------------------------------------ the stereo mask filter
def _stereo_batch(form, b, defect):
    return [mc.stereo_model_rows(x, b["w"], m, defect) for x, m in zip(b["clips"], b["masks"])]


def _stereo_errors(b, got):
    """The worst mask_error of y_L and y_R, the level over both channels (tests/test_gpu_accuracy.py's bound on top)."""
    return max(mc.mask_error(g[j], r[j], mc.row_level(r, x, j, 2)) for g, r, x in zip(got, b["refs"], b["clips"]) for j in (0, 1))


def _stereo_judged(b, got, h, rest=True):
    rows = lambda v: mc.rows_of(v, rest, 2)   # noqa: E731
    return acc.measure(rows(got), rows(b["refs"]), h), acc.measure(rows(b["yard"]), rows(b["refs"]), h)


@pytest.mark.parametrize("form", sorted(mc.STEREO_DATA))
@pytest.mark.parametrize("wl", mc.WINDOWS)
def test_the_stereo_model_is_within_the_family_factors(wl, form):
    """Two channels in one transform, the per-channel form's split and re-pack and the shared form's none, in NumPy float32: within the
    family's factors of the unpacked yardstick on the catalogue's own batches and on their ragged extras, the rest included."""
    for blocks in mc.BLOCKS:
        b, e = mc.accuracy_batch(f"{form}_{wl}_{blocks}_rest")
        twin, _ = mc.ragged_twin(b, e)
        k, y = _stereo_judged(twin, _stereo_batch(form, twin, None), wl // 2)
        print(acc.line(f"stereo model {form} W={wl} T={blocks + 2}", "-", k, y))
        assert acc.over(k, y, acc.factors()) == [], acc.ratios(k, y)
        assert _stereo_errors(twin, _stereo_batch(form, twin, None)) <= mc.TOL_FFT


def test_the_stereo_model_and_yardstick_keep_the_hop_bound():
    """hop_share_stereo is a condition on k_maskfilter_stereo (tests/test_gpu_signals.py::test_stereo_signal_through_the_mask_filters), so it is
    held here first: on all eleven stereo signals, W = 2048 and 256, both forms, both clips, y and the rest, the unpacked float32 chain stays
    within 0.5 of it and the model of the packing within 1 -- a failure on the GPU then points at the kernel.  The silent channel of
    left_only is where the model comes closest: it inherits the loud channel's rounding and has nothing but the floor to be held to."""
    worst, packed = (-1.0, ()), (-1.0, ())
    assert len(sig.STEREO_NAMES) == 11 and mc.SIGNAL_WINDOWS == (2048, 256)
    for wl in mc.SIGNAL_WINDOWS:
        h = wl // 2
        for name in sig.STEREO_NAMES:
            case = mc.stereo_signal_case(name, wl)
            for form in mc.STEREO_SIGNAL_FORMS:
                c = case[form]
                for i, (yard, ref, x, m) in enumerate(zip(c["yard"], c["refs"], c["clips"], c["masks"])):
                    model = mc.stereo_model_rows(x, case["w"], m)
                    for j in (0, 2):   # the pair y_L, y_R and the pair rest_L, rest_R
                        for ch, (s_yard, s_model) in enumerate(zip(mc.hop_share_stereo(yard[j:j + 2], ref[j:j + 2], x, h),
                                                                   mc.hop_share_stereo(model[j:j + 2], ref[j:j + 2], x, h))):
                            at = (name, wl, form, i, j + ch)
                            worst, packed = max(worst, (s_yard, at)), max(packed, (s_model, at))
                            assert s_yard <= 0.5 and s_model <= 1.0, (at, s_yard, s_model)
                    if not np.any(x):
                        assert not np.any(yard) and not np.any(model), (name, wl, form)
    print(f"worst share of the stereo hop bound: unpacked {worst[0]:.3f} {worst[1]}, stereo model {packed[0]:.3f} {packed[1]}")


@pytest.mark.parametrize("wl", [256, 2048])
def test_the_stereo_checks_see_each_defect(wl):
    """One defect at a time in the stereo model, through the checks of the GPU modules:
      * the window read at (W - n) % W: past TOL_FFT under `skew`, both forms -- and, under periodic Hamming, the bits of the sound model;
      * m_0 and m_1 exchanged: past TOL_FFT in stereo2, under either window; stereo1 has one mask and keeps the sound model's bits;
      * bin H's mask taken from bin H - 1: past TOL_FFT and outside the accuracy factors;
      * Z rounded to 16 mantissa bits before the masks: inside TOL_FFT, outside the accuracy factors in every metric."""
    h = wl // 2
    for form in sorted(mc.STEREO_DATA):
        ham, skew = mc.batch(form, wl, 20 * h + 9, "hamming", "unit"), mc.batch(form, wl, 20 * h + 9, "skew", "unit")
        sound = _stereo_batch(form, ham, None)
        assert _stereo_errors(ham, sound) <= mc.TOL_FFT and _stereo_errors(skew, _stereo_batch(form, skew, None)) <= mc.TOL_FFT
        mirrored = _stereo_batch(form, ham, "window_mirror")
        assert all(np.array_equal(a, b) for a, b in zip(mirrored, sound))
        assert _stereo_errors(skew, _stereo_batch(form, skew, "window_mirror")) >= 0.05
        for b in (ham, skew):
            swapped = _stereo_batch(form, b, "channel_swap")
            if form == "stereo2":
                assert _stereo_errors(b, swapped) >= 0.05, (wl, _stereo_errors(b, swapped))
            else:
                assert all(np.array_equal(a, c) for a, c in zip(swapped, _stereo_batch(form, b, None)))
        assert _stereo_errors(ham, _stereo_batch(form, ham, "bin_h")) > mc.TOL_FFT
        b = mc.batch(form, wl, 61 * h + 5, rotate=0)
        assert acc.over(*_stereo_judged(b, _stereo_batch(form, b, None), h), acc.factors()) == []
        k, y = _stereo_judged(b, _stereo_batch(form, b, "bin_h"), h)
        assert acc.over(k, y, acc.factors()) != [], acc.ratios(k, y)
        rounded = _stereo_batch(form, b, "round16")
        k, y = _stereo_judged(b, rounded, h, rest=False)
        print(acc.line(f"{form}: Z at 16 mantissa bits, W={wl}", "-", k, y))
        assert _stereo_errors(b, rounded) <= mc.TOL_FFT
        assert set(acc.over(k, y, acc.factors())) == set(acc.METRICS), acc.ratios(k, y)
