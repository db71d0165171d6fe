"""The stereo mask filter (zafx_execute_masked_stereo, zafx_execute_masked_stereo_ragged) without a GPU: the kernel's algorithm -- both
channels of a frame in one complex transform, the caller's mask(s) on the pairs (k, W-k), inverse, overlap-add (the pair functions of
zafx_maskfilter_stereo.hpp + the FFT core, compiled by g++) -- against the reference's own composition (tests/golden/maskfilter_stereo.npz,
made by tests/golden/make_maskfilter_stereo_golden.py) and against the float64 oracle; the refusal predicates of zafx_routes.hpp from both
sides of the 2^28 / 2^27 bounds; the cut of a ragged batch into units; the header's text, the ctypes signatures, the null-plan calls and the
argument checks of the Python layer."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from maskfilter_stereo_oracle import MASK_KINDS, TOL_FFT, golden_cases, make_stereo_masks, mask_frames, oracle_maskfilter_stereo, stereo_error

CSRC = os.path.join(ROOT, "zaf-python_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "host_emu")
EMU_SRC = os.path.join(EMU, "maskfilter_stereo_emu.cpp")
ROUTES_SRC = os.path.join(EMU, "maskfilter_stereo_routes_emu.cpp")
WINDOWS = (256, 512, 1024, 2048)
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_fixture_cases():
    got = {(wl, n) for wl, n, *_ in golden_cases()}
    assert got == {(2048, 5000), (1024, 3000), (512, 1500), (256, 1)}
    for wl, n, x, m, y, s in golden_cases():
        assert x.dtype == np.float32 and x.shape == (n, 2)
        assert m.dtype == np.float32 and m.shape == (2, wl // 2 + 1, mask_frames(n, wl)) and 0 <= m.min() and m.max() <= 1
        assert not np.array_equal(m[0], m[1])
        for r in (y, s):
            assert r.dtype == np.float64 and r.shape == (n, 2) and np.isfinite(r).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "maskfilter_stereo.npz")) < 1 << 20


def test_the_oracle_composition_matches_the_reference():
    import zafx
    for wl, n, x, m, y, s in golden_cases():
        w = zafx.hamming(wl)
        for ref, masks in ((y, m), (s, m[0])):
            assert np.abs(oracle_maskfilter_stereo(x, w, masks) - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0), (wl, n, masks.ndim)


# ------------------------------------------------------------------------------------------------------------------ the emulation
def _build(tmp_path_factory, name, flags, src=EMU_SRC):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-DZAFX_HOST_EMU", "-I", CSRC, *flags, src, "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def stereo_emu(tmp_path_factory):
    return _build(tmp_path_factory, "maskfilter_stereo_emu", ["-O2"])


@pytest.fixture(scope="module")
def routes_emu(tmp_path_factory):
    return _build(tmp_path_factory, "maskfilter_stereo_routes_emu", ["-O2", "-Wall", "-Wno-unknown-pragmas"], ROUTES_SRC)


def _payload(x, w, m):
    x, m = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(m, np.float32)
    mc = 1 if m.ndim == 2 else 2
    assert x.ndim == 2 and x.shape[1] == 2 and m.shape[-2:] == (len(w) // 2 + 1, mask_frames(len(x), len(w))) and (m.ndim == 2 or m.shape[0] == 2)
    return struct.pack("iii", len(w), len(x), mc) + np.asarray(w, np.float32).tobytes() + x.tobytes() + m.tobytes()


def _emulate(exe, x, w, m):
    res = subprocess.run([exe], input=_payload(x, w, m), capture_output=True, check=True)
    return np.frombuffer(res.stdout, np.float32).reshape(-1, 2)


def test_host_emulation_matches_the_reference(stereo_emu):
    import zafx
    for wl, n, x, m, y, s in golden_cases():
        for ref, masks in ((y, m), (s, m[0])):
            err = stereo_error(_emulate(stereo_emu, x, zafx.hamming(wl), masks), ref, x)
            print(f"W={wl} N={n} mask_channels={masks.ndim - 1}: error {err:.3e} of the level")
            assert err <= TOL_FFT, (wl, n, masks.ndim, err)


def edge_lengths(wl):
    h = wl // 2
    return [1, h - 1, h, h + 1, wl, 3 * h + 7, 20 * h]


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("wl", WINDOWS)
def test_host_emulation_against_the_oracle(stereo_emu, wl, channels):
    import zafx
    w = zafx.hamming(wl)
    worst = 0.0
    for n in edge_lengths(wl):
        x = np.random.default_rng([14, wl, n]).standard_normal((n, 2)).astype(np.float32)
        for kind in MASK_KINDS:
            m = make_stereo_masks(kind, wl, n, channels)
            got = _emulate(stereo_emu, x, w, m)
            err = stereo_error(got, oracle_maskfilter_stereo(x, w, m), x)
            worst = max(worst, err)
            assert got.shape == (n, 2) and err <= TOL_FFT, (wl, n, kind, channels, err)
    print(f"W={wl} mask_channels={channels}: worst error {worst:.3e} of the level")


def test_host_emulation_fixed_values(stereo_emu):
    """A mask of zeros gives exact zeros; silence on both channels gives zeros under any finite mask; the shared form under a mask of ones
    returns the input within the bound (Hamming at H = W/2 is COLA)."""
    import zafx
    wl, n = 512, 3001
    w = zafx.hamming(wl)
    x = np.random.default_rng(6).standard_normal((n, 2)).astype(np.float32)
    shape = (wl // 2 + 1, mask_frames(n, wl))
    for channels in (1, 2):
        zeros = np.zeros(shape if channels == 1 else (2,) + shape, np.float32)
        assert not _emulate(stereo_emu, x, w, zeros).any()
        assert not _emulate(stereo_emu, np.zeros((n, 2), np.float32), w, make_stereo_masks("signed_wide", wl, n, channels)).any()
    ident = _emulate(stereo_emu, x, w, np.ones(shape, np.float32))
    assert stereo_error(ident, x, x) <= TOL_FFT


def test_host_emulation_under_the_sanitizers(tmp_path_factory):
    """The emulations as stand-alone programs built with AddressSanitizer and UndefinedBehaviorSanitizer, run as such: the kernel's model on
    the shortest clip and on an odd length, both forms -- a clean exit and the oracle's values within the bound --, and the routes program
    on a refusal and a cut."""
    import zafx
    from zafx import _lib
    exe = _build(tmp_path_factory, "maskfilter_stereo_emu_san", SANITIZE)
    for wl, n in ((256, 1), (2048, 3 * 1024 + 7)):
        w = zafx.hamming(wl)
        x = np.random.default_rng([15, wl, n]).standard_normal((n, 2)).astype(np.float32)
        for channels in (1, 2):
            m = make_stereo_masks("unit", wl, n, channels)
            res = subprocess.run([exe], input=_payload(x, w, m), capture_output=True)
            assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
            assert stereo_error(np.frombuffer(res.stdout, np.float32).reshape(-1, 2), oracle_maskfilter_stereo(x, w, m), x) <= TOL_FFT
    routes = _build(tmp_path_factory, "maskfilter_stereo_routes_emu_san", SANITIZE, ROUTES_SRC)
    text = f"r {_lib.MASKFILTER} {_lib.LAYOUT_TF} 2 3 5 {1 << 27} 0\nc 256 8 4 12 5 0 1 128 391 7685\n"
    res = subprocess.run([routes], input=text, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    assert "refused 1:" in res.stdout and "units " in res.stdout


# ------------------------------------------------------------------------------------------------------------------ the refusals
def test_the_refusal_predicates_from_both_sides(routes_emu):
    from zafx import _lib
    mf, mfr, stft, tf, ft = _lib.MASKFILTER, _lib.MASKFILTER_REST, _lib.STFT, _lib.LAYOUT_TF, _lib.LAYOUT_FT
    top = {1: 1 << 28, 2: 1 << 27}
    cases = []
    for mc in (1, 2):
        t = top[mc]
        cases += [("e", mf, tf, mc, [t - 1]), ("e", mfr, tf, mc, [0]), ("r", mf, tf, mc, [1]), ("r", mfr, tf, mc, [t - 1, 0, 5]), ("r", mf, tf, mc, []),   # taken
                  ("e", mf, tf, mc, [t]), ("e", mfr, tf, mc, [t + 1]),                                                                                       # the length
                  ("r", mf, tf, mc, [t]), ("r", mfr, tf, mc, [5, 0, t - 1, t + 1, t])]                                                                       # a clip's length, with its index
    other = [("e", mf, ft, 1, [10]), ("e", mfr, ft, 2, [1 << 28]), ("r", mf, ft, 2, [10]), ("r", mfr, ft, 1, []),                       # the layout, named before a length
             ("e", stft, tf, 1, [10]), ("e", _lib.CENTER, ft, 2, [1 << 28]), ("r", stft, tf, 2, [10]), ("r", _lib.ISTFT, ft, 1, [1 << 28]),   # the kind, named first of all
             ("e", mf, tf, 0, [10]), ("e", mfr, tf, 3, [10]), ("r", mf, tf, 0, [10]), ("r", mfr, tf, 3, []), ("e", mf, tf, -1, [1 << 28])]   # mask_channels, before a length
    cases += other
    text = "".join(f"{form} {k} {lay} {mc} " + (f"{ls[0]}" if form == "e" else f"{len(ls)} {' '.join(str(v) for v in ls)}") + "\n" for form, k, lay, mc, ls in cases)
    res = subprocess.run([routes_emu], input=text, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    head, *rest = res.stdout.strip().split("\n")
    assert head == f"{mf} {mfr} {1 << 28} {1 << 27}"
    for line, wl in zip(rest[:4], WINDOWS):   # the offset arithmetic at the bounds: the kernel's descriptor, T mask_channels (H + 1) 4 bytes
        w_, below1, below2, above1, above2 = (int(v) for v in line.split())
        assert w_ == wl and below1 == mask_frames(top[1] - 1, wl) * (wl // 2 + 1) * 4 < 1 << 31, line
        assert below2 == mask_frames(top[2] - 1, wl) * 2 * (wl // 2 + 1) * 4 < 1 << 31 and above1 >= 1 << 31 and above2 >= 1 << 31, line
    out = rest[4:]
    assert len(out) == len(cases)
    for i, mc in enumerate((1, 2)):
        o = out[9 * i:9 * i + 9]
        bound = "2^28" if mc == 1 else "2^27"
        assert o[:5] == ["taken"] * 5, o
        for line in o[5:7]:
            assert line.startswith("refused -1:") and bound in line and "sample frames" in line, line
        assert o[7].startswith("refused 0:") and bound in o[7]
        assert o[8].startswith("refused 3:") and bound in o[8]
    o = out[18:]
    for line in o[0:4]:
        assert line.startswith("refused -1:") and "ZAFX_LAYOUT_TF" in line, line
    for line in o[4:8]:
        assert line.startswith("refused -1:") and "ZAFX_MASKFILTER" in line and "plans only" in line, line
    for line in o[8:13]:
        assert line.startswith("refused -1:") and "mask_channels" in line, line


@pytest.mark.parametrize("wl,tile", [(256, 8), (2048, 4)])
@pytest.mark.parametrize("slots,per_slot", [(1, 1), (4, 12), (1024, 12)])
def test_the_unit_cut(routes_emu, wl, tile, slots, per_slot):
    """Every block of every clip lies in exactly one unit, no unit is empty or reaches past its clip, the records carry the clip's offsets --
    mask_off among them -- and the units come ordered by descending size."""
    h = wl // 2
    lengths = [0, 1, h, 3 * h + 7, 60 * h + 5]
    res = subprocess.run([routes_emu], input=f"c {wl} {tile} {slots} {per_slot} {len(lengths)} {' '.join(map(str, lengths))}\n", capture_output=True, text=True,
                         timeout=60, check=True)
    lines = res.stdout.strip().split("\n")[5:]
    assert lines[0].startswith("units ")
    units = [tuple(int(v) for v in line.split()) for line in lines[1:]]
    assert len(units) == int(lines[0].split()[1])
    covered = {i: [] for i in range(len(lengths))}
    for in_off, n, out_off, mask_off, b0, b1, pitch in units:
        i = (in_off - 1) // 1000
        assert (in_off, n, out_off, mask_off, pitch) == (1000 * i + 1, lengths[i], 2000 * i + 2, 3000 * i + 3, 0)
        assert 0 <= b0 < b1 <= -(-n // h)
        covered[i] += list(range(b0, b1))
    for i, n in enumerate(lengths):
        assert sorted(covered[i]) == list(range(-(-n // h))), (i, n)
    sizes = [u[5] - u[4] for u in units]
    assert sizes == sorted(sizes, reverse=True)
    if slots == 1 and per_slot == 1:   # one segment length for the batch: everything whole
        assert len(units) == 4
    if slots == 1024:   # the floor 4 F - 3 cuts the long clip, and every piece of it keeps 2 F - 1 blocks
        long_units = [u for u in units if u[1] == lengths[-1]]
        assert len(long_units) > 1 and all(4 * tile - 3 >= u[5] - u[4] >= 2 * tile - 1 for u in long_units)


# ------------------------------------------------------------------------------------------------------------------ header, binding, Python layer
def test_header_text_and_binding():
    from zafx import _lib
    import zafx
    header = open(os.path.join(ROOT, "include", "zafx.h")).read()
    assert "zafx_execute_masked_stereo" in header.split("#ifndef ZAFX_H")[0]
    text = re.sub(r"\s*\n \*\s*", " ", header)
    assert "2^28 sample frames" in text and "2^27 with mask_channels == 2" in text and "NOT promised: that two equal per-channel masks give the bits of the shared form" in text
    assert '"k_maskfilter_stereo"' in text and '"k_maskfilter_stereo_ragged"' in text
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+zafx_execute_masked_stereo\s*\(\s*zafx_plan\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*void\s*\*\s*\w+,\s*int64_t\s+\w+,\s*int64_t\s+\w+,"
                     r"\s*int32_t\s+\w+\)", code)
    assert re.search(r"int\s+zafx_execute_masked_stereo_ragged\s*\(\s*zafx_plan\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,"
                     r"\s*const void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*int64_t\s+\w+,\s*int32_t\s+\w+\)", code)
    assert re.search(r"int\s+zafx_plan_stereo_ragged_layout\s*\(\s*const zafx_plan\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*int64_t\s+\w+,\s*int32_t\s+\w+,\s*int64_t\s*\*\s*\w+,"
                     r"\s*int64_t\s*\*\s*\w+\)", code)
    assert _lib.SYMBOLS["zafx_execute_masked_stereo"] == _lib.SYMBOLS["zafx_execute_masked_stems"]
    assert _lib.SYMBOLS["zafx_execute_masked_stereo_ragged"] == _lib.SYMBOLS["zafx_execute_masked_stems_ragged"]
    assert _lib.SYMBOLS["zafx_plan_stereo_ragged_layout"] == _lib.SYMBOLS["zafx_plan_stems_ragged_layout"]
    for name in ("execute_masked_stereo", "execute_masked_stereo_ragged", "stereo_mask_shape", "stereo_out_shape", "stereo_ragged_layout"):
        assert callable(getattr(zafx.Plan, name))
    for name in ("maskfilter_stereo", "maskfilter_stereo_batch", "maskfilter_stereo_ragged", "pack_ragged_stereo_masks"):
        assert callable(getattr(zafx, name))
    routes = open(os.path.join(CSRC, "zafx_routes.hpp")).read()
    assert 'kMaskfilterStereoKernel = "k_maskfilter_stereo"' in routes and 'kMaskfilterStereoRaggedKernel = "k_maskfilter_stereo_ragged"' in routes
    assert "zafx_maskfilter_stereo.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_null_plan_is_an_error_with_text(built_library):
    from zafx import _lib
    lib = _lib.load()
    assert lib.zafx_execute_masked_stereo(None, None, None, None, 1, 1000, 1) != 0
    assert b"null" in lib.zafx_last_error()
    one = (ctypes.c_int64 * 2)(0, 0)
    assert lib.zafx_execute_masked_stereo_ragged(None, None, one, one, None, one, None, one, 1, 2) != 0
    assert b"null" in lib.zafx_last_error()
    assert lib.zafx_plan_stereo_ragged_layout(None, one, 1, 1, one, one) != 0
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
    x, m1, m2 = np.zeros((3, n, 2), np.float32), np.ones((3, 513, t), np.float32), np.ones((3, 2, 513, t), np.float32)
    for m in (m1, m2):
        with pytest.raises(ValueError, match="shape"):
            zafx.maskfilter_stereo_batch(x, w, m[..., :-1])                # a frame short
        with pytest.raises(ValueError, match="shape"):
            zafx.maskfilter_stereo_batch(x, w, m[:2])                      # a clip short
        with pytest.raises(ValueError, match="shape"):
            zafx.maskfilter_stereo_batch(x, w, m, layout="TF")             # the other layout's shape
        with pytest.raises(ValueError, match="shape"):
            zafx.maskfilter_stereo_batch(x[:, :-1000], w, m)               # the masks of a longer clip
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stereo_batch(x, w, np.ones((3, 3, 513, t), np.float32))   # three channels
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stereo_batch(x, w, m2.transpose(0, 3, 1, 2))       # "TF" masks handed in as "FT"
    with pytest.raises(ValueError, match="3-D .* or 4-D"):
        zafx.maskfilter_stereo_batch(x, w, m1[0])
    with pytest.raises(ValueError, match="real"):
        zafx.maskfilter_stereo_batch(x, w, m1.astype(np.complex64))
    with pytest.raises(ValueError, match="dtype"):
        zafx.maskfilter_stereo_batch(x, w, np.full(m1.shape, "1"))
    with pytest.raises(ValueError, match="stereo"):
        zafx.maskfilter_stereo_batch(x[..., 0], w, m1)
    with pytest.raises(ValueError, match="step_length"):
        zafx.maskfilter_stereo_batch(x, w, m1, step_length=256)
    with pytest.raises(ValueError, match="window_length"):
        zafx.maskfilter_stereo_batch(np.zeros((1, 9000, 2), np.float32), zafx.hamming(4096), np.ones((1, 2049, 6), np.float32))
    for bad in (np.empty((3, n, 2), np.float64), np.empty((3, 2, n, 2), np.float32), np.empty((2, n, 2), np.float32), np.empty((3, n), np.float32)):
        with pytest.raises(ValueError, match="out must be"):
            zafx.maskfilter_stereo_batch(x, w, m1, out=bad)
    with pytest.raises(ValueError, match="out must be"):
        zafx.maskfilter_stereo_batch(x, w, m2, rest=True, out=np.empty((3, n, 2), np.float32))
    with pytest.raises(ValueError, match="step_length"):
        zafx.maskfilter_stereo(x[0], w, 256, m1[0])
    with pytest.raises(ValueError, match="stereo"):
        zafx.maskfilter_stereo(np.zeros(n), w, 512, m1[0])
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        zafx.maskfilter_stereo(x[0], w, 512, m2)
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stereo(x[0], w, 512, m2[0, :, :, 1:])
    # ragged: list lengths, shapes with the clip's index, one kind of mask for the batch
    clips = [np.zeros((700, 2), np.float32), np.zeros((1, 2), np.float32)]
    masks = [np.ones((513, mask_frames(700, 1024)), np.float32), np.ones((513, 2), np.float32)]
    with pytest.raises(ValueError, match="one entry per clip"):
        zafx.maskfilter_stereo_ragged(clips, w, masks[:1])
    with pytest.raises(ValueError, match="mask 1 must have shape"):
        zafx.maskfilter_stereo_ragged(clips, w, [masks[0], masks[1][:, :1]])
    with pytest.raises(ValueError, match="mask 0 must have shape"):
        zafx.maskfilter_stereo_ragged(clips, w, masks, layout="TF")
    with pytest.raises(ValueError, match="mask 1 .* must be 2-D"):
        zafx.maskfilter_stereo_ragged(clips, w, [masks[0], np.stack([masks[1]] * 2)])
    with pytest.raises(ValueError, match="must be stereo"):
        zafx.maskfilter_stereo_ragged([clips[0][:, :1], clips[1]], w, masks)
    with pytest.raises(ValueError, match="sequence"):
        zafx.pack_ragged_stereo_masks(masks[0], [700], 1024)
    # an empty batch is taken, and needs no device
    got = zafx.maskfilter_stereo_batch(np.zeros((0, n, 2), np.float32), w, np.ones((0, 513, t), np.float32))
    assert got.shape == (0, n, 2) and got.dtype == np.float32


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("layout", ["FT", "TF"])
def test_pack_ragged_stereo_masks(layout, channels):
    """The packed array holds every clip's masks as (T_i, mask_channels, W/2 + 1) float32 at the compact offsets -- the arithmetic of
    zafx_plan_stereo_ragged_layout, computed here --, whichever layout the masks came in."""
    import zafx
    wl, h = 512, 256
    lengths = [0, 1, h, 3 * h + 7, 5000]
    frames = [mask_frames(n, wl) for n in lengths]
    g = np.random.default_rng(10)
    masks = [g.standard_normal((h + 1, t) if channels == 1 else (2, h + 1, t)).astype(np.float32) for t in frames]
    masks[2] = masks[2].astype(np.float64)
    given = masks if layout == "FT" else [m.T if channels == 1 else m.transpose(2, 0, 1) for m in masks]
    packed, offs, mc = zafx.pack_ragged_stereo_masks(given, lengths, wl, layout)
    want = np.concatenate(([0], np.cumsum([channels * t * (h + 1) for t in frames])))
    assert mc == channels and packed.dtype == np.float32 and packed.ndim == 1 and offs.dtype == np.int64 and np.array_equal(offs, want) and len(packed) == want[-1]
    for m, o, t in zip(masks, offs.tolist(), frames):
        block = packed[o:o + channels * t * (h + 1)].reshape(t, channels, h + 1)
        for c in range(channels):
            assert np.array_equal(block[:, c], (m if channels == 1 else m[c]).T.astype(np.float32))
    empty, offs0, mc0 = zafx.pack_ragged_stereo_masks([], [], wl, layout)
    assert empty.dtype == np.float32 and np.array_equal(offs0, [0]) and mc0 == 1
