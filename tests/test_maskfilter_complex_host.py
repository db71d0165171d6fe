"""The mask filter under complex masks (zafx_execute_masked_complex, zafx_execute_masked_complex_ragged) without a GPU: the kernel's
algorithm -- two frames of a clip in one complex transform, split, the caller's COMPLEX mask, re-pack, inverse, overlap-add
(maskfilter_pair_c of zafx_maskfilter.hpp + the FFT core, compiled by g++) -- against the reference's own composition
(tests/golden/maskfilter_complex.npz, made by tests/golden/make_maskfilter_complex_golden.py) and against the float64 oracle; the refusal
predicates of zafx_routes.hpp from both sides of the 2^27 bound; the header's text, the ctypes signatures, the null-plan calls and the
argument checks of the Python layer."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from maskfilter_complex_oracle import MASK_KINDS, TOL_FFT, golden_cases, make_complex_mask, mask_error, mask_frames, oracle_maskfilter_complex

CSRC = os.path.join(ROOT, "zaf-python_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "host_emu")
EMU_SRC = os.path.join(EMU, "maskfilter_complex_emu.cpp")
WINDOWS = (256, 512, 1024, 2048)


def test_fixture_cases_pin_the_discard_rule():
    got = {(wl, n) for wl, n, _, _, _ in golden_cases()}
    assert got == {(2048, 5000), (1024, 3000), (512, 1500), (256, 1)}
    for wl, n, x, m, y in golden_cases():
        assert x.dtype == np.float32 and x.shape == (n,)
        assert m.dtype == np.complex64 and m.shape == (wl // 2 + 1, mask_frames(n, wl)) and np.abs(m).max() <= 1 + 1e-6
        assert (m[0].imag != 0).all() and (m[-1].imag != 0).all()   # rows 0 and W/2 carry imaginary parts the reference drops
        assert y.dtype == np.float64 and y.shape == (n,) and np.isfinite(y).all()


def test_the_oracle_composition_matches_the_reference():
    import zafx
    for wl, n, x, m, y in golden_cases():
        ref = oracle_maskfilter_complex(x, zafx.hamming(wl), m)
        assert np.abs(ref - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0), (wl, n)
        m0 = m.copy()
        m0[0].imag = 0
        m0[-1].imag = 0
        assert np.abs(oracle_maskfilter_complex(x, zafx.hamming(wl), m0) - y).max() <= 1e-12 * max(np.abs(y).max(), 1.0), (wl, n, "rows 0 and W/2")


def test_the_oracle_agrees_with_the_real_kind():
    """Under a mask without imaginary parts the composition is the real kind's; a mask of ones returns the clip (Hamming at H = W/2 is COLA)."""
    import zafx
    from maskfilter_oracle import oracle_maskfilter
    wl, n = 512, 3001
    w = zafx.hamming(wl)
    x = np.random.default_rng(4).standard_normal(n)
    m = make_complex_mask("real", wl, n)
    assert np.abs(oracle_maskfilter_complex(x, w, m) - oracle_maskfilter(x, w, m.real)).max() <= 1e-13
    ident = oracle_maskfilter_complex(x, w, np.ones((wl // 2 + 1, mask_frames(n, wl)), np.complex64))
    assert np.abs(ident - x).max() <= 1e-13


# ------------------------------------------------------------------------------------------------------------------ the emulation
def _build(tmp_path_factory, name, flags, src=EMU_SRC):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-DZAFX_HOST_EMU", "-I", CSRC, *flags, src, "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def complex_emu(tmp_path_factory):
    return _build(tmp_path_factory, "maskfilter_complex_emu", ["-O2"])


def _payload(x, w, m):
    x, m = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(m, np.complex64)
    assert m.shape == (len(w) // 2 + 1, mask_frames(len(x), len(w)))
    return struct.pack("ii", len(w), len(x)) + np.asarray(w, np.float32).tobytes() + x.tobytes() + m.tobytes()


def _emulate(exe, x, w, m):
    res = subprocess.run([exe], input=_payload(x, w, m), capture_output=True, check=True)
    return np.frombuffer(res.stdout, np.float32)


def test_host_emulation_matches_the_reference(complex_emu):
    import zafx
    for wl, n, x, m, y in golden_cases():
        err = mask_error(_emulate(complex_emu, x, zafx.hamming(wl), m), y, x)
        print(f"W={wl} N={n}: error {err:.3e} of the level")
        assert err <= TOL_FFT, (wl, n, err)


def edge_lengths(wl):
    h = wl // 2
    return [1, h - 1, h, h + 1, wl, 3 * h + 7, 20 * h]


@pytest.mark.parametrize("wl", WINDOWS)
def test_host_emulation_against_the_oracle(complex_emu, wl):
    import zafx
    w = zafx.hamming(wl)
    worst = 0.0
    for n in edge_lengths(wl):
        x = np.random.default_rng([12, wl, n]).standard_normal(n).astype(np.float32)
        for kind in MASK_KINDS:
            m = make_complex_mask(kind, wl, n)
            got = _emulate(complex_emu, x, w, m)
            err = mask_error(got, oracle_maskfilter_complex(x, w, m), x)
            worst = max(worst, err)
            assert got.shape == (n,) and err <= TOL_FFT, (wl, n, kind, err)
    print(f"W={wl}: worst error {worst:.3e} of the level")


def test_host_emulation_fixed_values(complex_emu):
    """A mask of zeros gives no non-zero output; silence under the "big" mask gives none; NaN in Im M of rows 0 and W/2 gives the bytes that
    zeros there give."""
    import zafx
    wl, n = 512, 3001
    w = zafx.hamming(wl)
    x = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    assert not _emulate(complex_emu, x, w, np.zeros((wl // 2 + 1, mask_frames(n, wl)), np.complex64)).any()
    assert not _emulate(complex_emu, np.zeros(n, np.float32), w, make_complex_mask("big", wl, n)).any()
    m = make_complex_mask("disc", wl, n)
    zeros, nans = m.copy(), m.copy()
    for a, v in ((zeros, 0.0), (nans, np.nan)):
        a[0].imag = v
        a[-1].imag = v
    assert np.isnan(nans[0].imag).all() and np.isnan(nans[-1].imag).all() and np.isfinite(nans[1:-1]).all()
    got = _emulate(complex_emu, x, w, nans)
    assert np.isfinite(got).all() and got.tobytes() == _emulate(complex_emu, x, w, zeros).tobytes()
    assert mask_error(got, oracle_maskfilter_complex(x, w, m), x) <= TOL_FFT


def test_host_emulation_under_the_sanitizers(tmp_path_factory):
    """The emulation as a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, run as such on the shortest clip
    and on an odd length: a clean exit and the oracle's values within the bound."""
    import zafx
    exe = _build(tmp_path_factory, "maskfilter_complex_emu_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                                  "-fno-omit-frame-pointer"])
    for wl, n in ((256, 1), (2048, 3 * 1024 + 7)):
        w = zafx.hamming(wl)
        x = np.random.default_rng([13, wl, n]).standard_normal(n).astype(np.float32)
        m = make_complex_mask("disc", wl, n)
        res = subprocess.run([exe], input=_payload(x, w, m), capture_output=True)
        assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
        assert mask_error(np.frombuffer(res.stdout, np.float32), oracle_maskfilter_complex(x, w, m), x) <= TOL_FFT


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_the_refusal_predicates_from_both_sides(tmp_path_factory):
    from zafx import _lib
    exe = _build(tmp_path_factory, "maskfilter_complex_routes_emu", ["-O2", "-Wall", "-Wno-unknown-pragmas"], os.path.join(EMU, "maskfilter_complex_routes_emu.cpp"))
    mf, mfr, stft, tf, ft, top = _lib.MASKFILTER, _lib.MASKFILTER_REST, _lib.STFT, _lib.LAYOUT_TF, _lib.LAYOUT_FT, 1 << 27
    cases = [
        ("e", mf, tf, [top - 1]), ("e", mfr, tf, [0]), ("r", mf, tf, [1]), ("r", mfr, tf, [top - 1, 0, 5]), ("r", mf, tf, []),      # taken
        ("e", mf, tf, [top]), ("e", mfr, tf, [top + 1]),                                                                                # the length
        ("e", mf, ft, [10]), ("e", mfr, ft, [top]), ("r", mf, ft, [10]), ("r", mfr, ft, []),                                          # the layout, named before a length
        ("e", stft, tf, [10]), ("e", _lib.CENTER, ft, [top]), ("r", stft, tf, [10]), ("r", _lib.ISTFT, ft, [top]),                    # the kind, named first of all
        ("r", mf, tf, [top]), ("r", mfr, tf, [5, 0, top - 1, top + 1, top]),                                                           # a clip's length, with its index
    ]
    text = "".join(f"{form} {k} {lay} " + (f"{ls[0]}" if form == "e" else f"{len(ls)} {' '.join(str(v) for v in ls)}") + "\n" for form, k, lay, ls in cases)
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    head, *rest = res.stdout.strip().split("\n")
    assert head == f"{mf} {mfr} {top}"
    for line, wl in zip(rest[:4], WINDOWS):   # the offset arithmetic at the bound: the kernel's descriptor, (T)(H + 1) 8 bytes
        w_, below, above = (int(v) for v in line.split())
        assert w_ == wl and below == mask_frames(top - 1, wl) * (wl // 2 + 1) * 8 < 1 << 31 and above >= 1 << 31, line
    out = rest[4:]
    assert len(out) == len(cases) and out[:5] == ["taken"] * 5
    for line in out[5:7]:
        assert line.startswith("refused -1:") and "2^27" in line, line
    for line in out[7:11]:
        assert line.startswith("refused -1:") and "ZAFX_LAYOUT_TF" in line, line
    for line in out[11:15]:
        assert line.startswith("refused -1:") and "ZAFX_MASKFILTER" in line and "plans only" in line, line
    assert out[15].startswith("refused 0:") and "2^27" in out[15]
    assert out[16].startswith("refused 3:") and "2^27" in out[16]


# ------------------------------------------------------------------------------------------------------------------ header, binding, Python layer
def test_header_text_and_binding():
    from zafx import _lib
    import zafx
    header = open(os.path.join(ROOT, "include", "zafx.h")).read()
    assert re.search(r"#define ZAFX_VERSION 101\b", header)
    assert "zafx_execute_masked_complex" in header.split("#ifndef ZAFX_H")[0]
    text = re.sub(r"\s*\n \*\s*", " ", header)
    assert "The imaginary parts of mask rows 0 and W/2 have no effect" in text and "NaN included" in text
    assert "2^27" in text and "-ffp-contract=fast" in text and "zafx_plan_ragged_layout gives a one-sided complex ZAFX_LAYOUT_TF STFT plan" in text
    assert '"k_maskfilter_complex"' in text and '"k_maskfilter_complex_ragged"' in text
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+zafx_execute_masked_complex\s*\(\s*zafx_plan\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*void\s*\*\s*\w+,\s*int64_t\s+\w+,\s*int64_t\s+\w+\)", code)
    assert re.search(r"int\s+zafx_execute_masked_complex_ragged\s*\(\s*zafx_plan\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,"
                     r"\s*const void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*int64_t\s+\w+\)", code)
    res, args = _lib.SYMBOLS["zafx_execute_masked_complex"]
    assert res is ctypes.c_int and args == _lib.SYMBOLS["zafx_execute_masked"][1] and len(args) == 6
    res, args = _lib.SYMBOLS["zafx_execute_masked_complex_ragged"]
    assert res is ctypes.c_int and args == _lib.SYMBOLS["zafx_execute_masked_ragged"][1] and len(args) == 9
    for name in ("execute_masked_complex", "execute_masked_complex_ragged"):
        assert callable(getattr(zafx.Plan, name))
    for name in ("maskfilter_complex", "maskfilter_complex_batch", "maskfilter_complex_ragged", "pack_ragged_complex_masks"):
        assert callable(getattr(zafx, name))
    routes = open(os.path.join(CSRC, "zafx_routes.hpp")).read()
    assert 'kMaskfilterComplexKernel = "k_maskfilter_complex"' in routes and 'kMaskfilterComplexRaggedKernel = "k_maskfilter_complex_ragged"' in routes


def test_null_plan_is_an_error_with_text(built_library):
    from zafx import _lib
    lib = _lib.load()
    assert lib.zafx_execute_masked_complex(None, None, None, None, 1, 1000) != 0
    assert b"null" in lib.zafx_last_error()
    one = (ctypes.c_int64 * 1)(0)
    assert lib.zafx_execute_masked_complex_ragged(None, None, one, one, None, one, None, one, 1) != 0
    assert b"null" in lib.zafx_last_error()


def test_argument_validation_before_the_library_is_loaded(monkeypatch):
    import zafx
    from zafx import _lib

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    w = zafx.hamming(1024)
    n = 4000
    t = mask_frames(n, 1024)
    x, m = np.zeros((3, n), np.float32), np.ones((3, 513, t), np.complex64)
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_complex_batch(x, w, m[:, :, :-1])             # a frame short
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_complex_batch(x, w, m[:, :-1])                # a row short
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_complex_batch(x, w, m[:2])                    # a clip short
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_complex_batch(x, w, m, layout="TF")           # the other layout's shape
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_complex_batch(x, w, m.transpose(0, 2, 1))     # ... and the reverse
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_complex_batch(x[:, :-1000], w, m)             # the mask of a longer clip
    with pytest.raises(ValueError, match="real"):
        zafx.maskfilter_complex_batch(x.astype(np.complex64), w, m)
    with pytest.raises(ValueError, match="dtype"):
        zafx.maskfilter_complex_batch(x, w, np.full(m.shape, "1"))    # strings
    with pytest.raises(ValueError, match="step_length"):
        zafx.maskfilter_complex_batch(x, w, m, step_length=256)
    with pytest.raises(ValueError, match="window_length"):
        zafx.maskfilter_complex_batch(np.zeros((1, 9000), np.float32), zafx.hamming(4096), np.ones((1, 2049, 6), np.complex64))
    with pytest.raises(ValueError):
        zafx.maskfilter_complex_batch(np.zeros((3, n, 2), np.float32), w, m)
    for bad in (np.empty((3, n), np.float64), np.empty((3, 2, n), np.float32), np.empty((2, n), np.float32), np.empty((3, n + 1), np.float32)):
        with pytest.raises(ValueError, match="out must be"):
            zafx.maskfilter_complex_batch(x, w, m, out=bad)
    with pytest.raises(ValueError, match="out must be"):
        zafx.maskfilter_complex_batch(x, w, m, rest=True, out=np.empty((3, n), np.float32))
    with pytest.raises(ValueError, match="step_length"):
        zafx.maskfilter_complex(np.zeros(n), w, 256, m[0])
    with pytest.raises(ValueError):
        zafx.maskfilter_complex(np.zeros((n, 2)), w, 512, m[0])
    with pytest.raises(ValueError):
        zafx.maskfilter_complex(np.zeros(n), w, 512, m)
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_complex(np.zeros(n), w, 512, m[0, :, 1:])
    # ragged: list lengths, shapes with the clip's index, dtypes
    clips = [np.zeros(700, np.float32), np.zeros(1, np.float32)]
    masks = [np.ones((513, mask_frames(700, 1024)), np.complex64), np.ones((513, 2), np.complex64)]
    with pytest.raises(ValueError, match="one entry per clip"):
        zafx.maskfilter_complex_ragged(clips, w, masks[:1])
    with pytest.raises(ValueError, match="mask 1 must have shape"):
        zafx.maskfilter_complex_ragged(clips, w, [masks[0], masks[1][:, :1]])
    with pytest.raises(ValueError, match="mask 0 must have shape"):
        zafx.maskfilter_complex_ragged(clips, w, masks, layout="TF")
    with pytest.raises(ValueError, match="mask 1 .* must be numeric"):
        zafx.maskfilter_complex_ragged(clips, w, [masks[0], np.full((513, 2), "x")])
    with pytest.raises(ValueError, match="must be real"):
        zafx.maskfilter_complex_ragged([clips[0].astype(np.complex64), clips[1]], w, masks)
    with pytest.raises(ValueError, match="sequence"):
        zafx.pack_ragged_complex_masks(masks[0], [700], 1024)
    # the real kinds keep refusing complex masks
    with pytest.raises(ValueError, match="real"):
        zafx.maskfilter_batch(x, w, m)
    with pytest.raises(ValueError, match="real"):
        zafx.maskfilter_ragged(clips, w, masks)
    # an empty batch of REAL masks is taken, and needs no device
    got = zafx.maskfilter_complex_batch(np.zeros((0, n), np.float32), w, np.ones((0, 513, t), np.float32))
    assert got.shape == (0, n) and got.dtype == np.float32


@pytest.mark.parametrize("layout", ["FT", "TF"])
def test_pack_ragged_complex_masks(layout):
    """The packed array holds every mask as (T_i, W/2 + 1) complex64 at the compact offsets -- the arithmetic of zafx_plan_mask_ragged_layout for
    a TF plan, computed here --, whichever layout the masks came in; real masks are accepted and become complex64."""
    import zafx
    wl, h = 512, 256
    lengths = [0, 1, h, 3 * h + 7, 5000]
    frames = [mask_frames(n, wl) for n in lengths]
    g = np.random.default_rng(9)
    masks = [(g.standard_normal((h + 1, t)) + 1j * g.standard_normal((h + 1, t))).astype(np.complex64) for t in frames]
    masks[2] = masks[2].real.astype(np.float64)   # a real one among them
    given = masks if layout == "FT" else [m.T for m in masks]
    packed, offs = zafx.pack_ragged_complex_masks(given, lengths, wl, layout)
    want = np.concatenate(([0], np.cumsum([t * (h + 1) for t in frames])))
    assert packed.dtype == np.complex64 and packed.ndim == 1 and offs.dtype == np.int64 and np.array_equal(offs, want) and len(packed) == want[-1]
    for m, o, t in zip(masks, offs.tolist(), frames):
        assert np.array_equal(packed[o:o + t * (h + 1)].reshape(t, h + 1), m.T.astype(np.complex64))
    empty, offs0 = zafx.pack_ragged_complex_masks([], [], wl, layout)
    assert empty.dtype == np.complex64 and np.array_equal(offs0, [0])
