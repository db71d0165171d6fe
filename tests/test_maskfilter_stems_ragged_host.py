"""Ragged mask filter stems (zafx_execute_masked_stems_ragged, zafx_plan_stems_ragged_layout, k_maskfilter_stems' RAGGED form) without a GPU: the
two entry points in the header, the binding and the library, the refusal predicate at its edges, the packing and the validation that run
before any device call, the cutter under the stems' workgroup slots, and a CPU model of the RAGGED walk
(tests/host_emu/maskfilter_stems_units_emu.cpp on the product's headers, compiled by g++; once more under the sanitizers as a stand-alone
program): a clip walked as the cutter's units has the bits of the clip walked whole, and per stem the bits of the one-mask emulation
(tests/host_emu/maskfilter_emu.cpp).

Bounds: bit identity; against the oracle max|y - ref| <= 1e-5 max(max|ref|, max|x|) per stem (TOL_FFT at mask_error's level)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import zafx
from zafx import _lib

from conftest import ROOT
from maskfilter_oracle import TOL_FFT, make_mask, mask_error, mask_frames, oracle_maskfilter

CSRC = os.path.join(ROOT, "zaf-python_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "host_emu")
STEMS = (1, 4, 8)
# k_maskfilter_stems' dynamic LDS at one stem (DESIGN.md 4.12 "Stems"); every further stem adds a carry of W/2 floats
SMEM_ONE = {256: 20000, 512: 39936, 1024: 79808, 2048: 90016}
LDS, CUS = 160 * 1024, 256


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tile(wl):
    return _lib.maskfilter_tile_transforms(wl)


def stems_slots(wl, n_stems, cus=CUS):
    """Workgroups the device holds at once under the stems' LDS size: what LDS admits per compute unit, at most 4 (lds_slots of maskfilter_stems_smem)."""
    return cus * max(1, min(4, LDS // (SMEM_ONE[wl] + (n_stems - 1) * (wl // 2) * 4)))


def lengths_of(h):
    base = [0, 1, h - 1, h, h + 1, 2 * h, 2 * h + 1, 14 * h, 60 * h, 61 * h - 3, 200 * h - 500]
    return base + base[::-1] + [61 * h - 3, 0, 60 * h]


# ------------------------------------------------------------------------------------------------------------------ symbols
def test_both_entry_points_are_declared_bound_and_exported(built_library):
    header = open(os.path.join(ROOT, "include", "zafx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+zafx_plan_stems_ragged_layout\s*\(\s*const zafx_plan\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*int64_t\s+\w+,\s*int32_t\s+\w+,"
                     r"\s*int64_t\s*\*\s*\w+,\s*int64_t\s*\*\s*\w+\)", code)
    assert re.search(r"int\s+zafx_execute_masked_stems_ragged\s*\(\s*zafx_plan\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,"
                     r"\s*const void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*int64_t\s+\w+,\s*int32_t\s+\w+\)", code)
    res, args = _lib.SYMBOLS["zafx_plan_stems_ragged_layout"]
    assert res is ctypes.c_int and len(args) == 6
    res, args = _lib.SYMBOLS["zafx_execute_masked_stems_ragged"]
    assert res is ctypes.c_int and len(args) == 10
    lib = ctypes.CDLL(built_library)
    assert hasattr(lib, "zafx_plan_stems_ragged_layout") and hasattr(lib, "zafx_execute_masked_stems_ragged")
    for name in ("stems_ragged_layout", "execute_masked_stems_ragged"):
        assert callable(getattr(zafx.Plan, name))
    assert callable(zafx.maskfilter_stems_ragged) and callable(zafx.pack_ragged_stems_masks)
    # the comment states the contract
    text = header[header.index("Ragged stems:"):header.index("int zafx_execute_masked_stems_ragged")]
    for phrase in ("k_maskfilter_stems_ragged", "CONTRACT", "bit-identical to zafx_execute_masked_stems", "bit-identical to zafx_execute_masked with mask s alone",
                   "ZAFX_COMPUTE_UNITS", "ZAFX_LAYOUT_TF", "2^28", "length 0"):
        assert phrase in text, phrase


def test_null_plan_is_an_error_with_text(built_library):
    lib = _lib.load()
    lengths = (ctypes.c_int64 * 2)(100, 200)
    offs, offs2 = (ctypes.c_int64 * 3)(-1, -1, -1), (ctypes.c_int64 * 3)(-1, -1, -1)
    assert lib.zafx_plan_stems_ragged_layout(None, lengths, 2, 2, offs, offs2) != 0
    assert b"null" in lib.zafx_last_error() and tuple(offs) == tuple(offs2) == (-1, -1, -1)
    assert lib.zafx_execute_masked_stems_ragged(None, None, lengths, lengths, None, lengths, None, lengths, 2, 2) != 0
    assert b"null" in lib.zafx_last_error()


# ------------------------------------------------------------------------------------------------------------------ the refusal predicate
def test_the_refusal_predicate_at_its_edges(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stems_ragged_routes") / "emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(EMU, "maskfilter_stems_ragged_routes_emu.cpp"), "-o", str(exe)], check=True)
    mf, mfr, stft, tf, ft, top = _lib.MASKFILTER, _lib.MASKFILTER_REST, _lib.STFT, _lib.LAYOUT_TF, _lib.LAYOUT_FT, 1 << 28
    cases = [
        (mf, tf, 1, [1]), (mfr, tf, 8, [top - 1, 0, 5]), (mf, tf, 4, []),                               # taken
        (mf, tf, 0, [10]), (mf, tf, 9, [10]), (mfr, tf, -1, []), (mf, tf, 1 << 32, [10]),                # the stem count
        (mf, ft, 1, [10]), (mfr, ft, 0, [top]),                                                          # the layout, named first
        (stft, tf, 2, [10]), (stft, ft, 0, [top]),                                                       # the kind, named first of all
        (mf, tf, 2, [top]), (mfr, tf, 8, [5, 0, top - 1, top + 1, top]),                                 # a clip's length, with its index
    ]
    text = "".join(f"{k} {lay} {s} {len(ls)} {' '.join(str(v) for v in ls)}\n" for k, lay, s, ls in cases)
    res = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    head, *out = res.stdout.strip().split("\n")
    assert head == f"{mf} {mfr} {_lib.MASKFILTER_MAX_STEMS}" and len(out) == len(cases)
    assert out[:3] == ["taken"] * 3
    for line in out[3:7]:
        assert line.startswith("refused -1:") and "n_stems" in line and "1 .. 8" in line, line
    for line in out[7:9]:
        assert line.startswith("refused -1:") and "ZAFX_LAYOUT_TF" in line, line
    for line in out[9:11]:
        assert line.startswith("refused -1:") and "ZAFX_MASKFILTER" in line and "plans only" in line, line
    assert out[11].startswith("refused 0:") and "2^28" in out[11]
    assert out[12].startswith("refused 3:") and "2^28" in out[12]


# ------------------------------------------------------------------------------------------------------------------ packing and validation
@pytest.mark.parametrize("layout", ["FT", "TF"])
def test_pack_ragged_stems_masks_layout_and_round_trip(layout):
    wl, h, s = 256, 128, 3
    lengths = [0, 1, h, h + 1, 5 * h - 3, 40 * h]
    rng = np.random.default_rng(2)
    masks = [rng.random((s, h + 1, mask_frames(n, wl))) for n in lengths]
    given = masks if layout == "FT" else [m.transpose(0, 2, 1) for m in masks]
    packed, offs = zafx.pack_ragged_stems_masks(given, lengths, wl, layout)
    assert packed.dtype == np.float32 and packed.ndim == 1 and offs.dtype == np.int64 and len(offs) == len(lengths) + 1 and offs[0] == 0
    one, _ = zafx.pack_ragged_masks([m[0] for m in masks], lengths, wl, "FT")[1], None
    assert offs.tolist() == (s * one).tolist()   # n_stems x the one-mask layout of a TF plan (compact: FT without row_align has the same sizes)
    for m, n, o, e in zip(masks, lengths, offs[:-1].tolist(), offs[1:].tolist()):
        t = mask_frames(n, wl)
        assert e - o == s * t * (h + 1)
        np.testing.assert_array_equal(packed[o:e].reshape(s, t, h + 1), m.transpose(0, 2, 1).astype(np.float32))
    assert len(packed) == offs[-1]


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: validation must come first."""
    def forbidden(*a, **k):
        raise AssertionError("the library was asked for a device before the input was validated")
    monkeypatch.setattr(_lib, "load", forbidden)


def test_bad_batches_are_rejected_before_the_library_is_loaded(no_device):
    w, wl, h = zafx.hamming(256), 256, 128
    ok = [np.zeros(300), np.zeros(5)]
    good = [np.ones((2, h + 1, mask_frames(300, wl))), np.ones((2, h + 1, mask_frames(5, wl)))]
    good_tf = [m.transpose(0, 2, 1) for m in good]
    with pytest.raises(ValueError, match="mask 1 must have shape .* for clip 1 of 5 samples"):
        zafx.maskfilter_stems_ragged(ok, w, [good[0], np.ones((2, h + 1, 5))])
    with pytest.raises(ValueError, match="mask 0 must have shape"):
        zafx.maskfilter_stems_ragged(ok, w, good, layout="TF")            # FT-shaped masks under TF
    with pytest.raises(ValueError, match="mask 0 must have shape"):
        zafx.maskfilter_stems_ragged(ok, w, good_tf)                      # ... and the reverse
    with pytest.raises(ValueError, match="mask 1 has 3 stems, mask 0 has 2"):
        zafx.maskfilter_stems_ragged(ok, w, [good[0], np.ones((3, h + 1, mask_frames(5, wl)))])
    with pytest.raises(ValueError, match="mask 1 has 1 stems"):
        zafx.maskfilter_stems_ragged(ok, w, [good_tf[0], good_tf[1][:1]], layout="TF")
    with pytest.raises(ValueError, match="stems"):
        zafx.maskfilter_stems_ragged(ok, w, [np.ones((9, h + 1, mask_frames(300, wl))), np.ones((9, h + 1, mask_frames(5, wl)))])
    with pytest.raises(ValueError, match="stems"):
        zafx.maskfilter_stems_ragged(ok, w, [m[:0] for m in good])
    with pytest.raises(ValueError, match="mask 1 .* must be 3-D"):
        zafx.maskfilter_stems_ragged(ok, w, [good[0], good[1][0]])
    with pytest.raises(ValueError, match="one entry per clip"):
        zafx.maskfilter_stems_ragged(ok, w, good[:1])
    with pytest.raises(ValueError, match="clip 1 .* must be 1-D"):
        zafx.maskfilter_stems_ragged([ok[0], np.zeros((5, 2))], w, good)
    with pytest.raises(ValueError, match="must be real"):
        zafx.maskfilter_stems_ragged([ok[0], np.zeros(5, np.complex64)], w, good)
    with pytest.raises(ValueError, match="must be real"):
        zafx.maskfilter_stems_ragged(ok, w, [good[0], good[1].astype(np.complex64)])
    with pytest.raises(ValueError, match="sequence"):
        zafx.maskfilter_stems_ragged(np.zeros(300), w, good)
    with pytest.raises(ValueError, match="at least one clip"):
        zafx.maskfilter_stems_ragged([], w, [])
    with pytest.raises(ValueError, match="power-of-two window_length"):
        zafx.maskfilter_stems_ragged(ok, zafx.hamming(4096), good)
    with pytest.raises(ValueError, match="step_length must be window_length / 2"):
        zafx.maskfilter_stems_ragged(ok, w, good, step_length=64)


# ------------------------------------------------------------------------------------------------------------------ the cutter under the stems' slots
def _build(tmp_path_factory, name, src, flags):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-DZAFX_HOST_EMU", "-I", CSRC, *flags, os.path.join(EMU, src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return _build(tmp_path_factory, "maskfilter_stems_units_emu", "maskfilter_stems_units_emu.cpp", ["-O2"])


@pytest.fixture(scope="module")
def single_emu(tmp_path_factory):
    return _build(tmp_path_factory, "maskfilter_emu", "maskfilter_emu.cpp", ["-O2"])


def cut(emu, lengths, wl, slots, n_stems, rest, per_slot=8):
    res = subprocess.run([emu, "cut", str(wl), str(tile(wl)), str(slots), str(per_slot), str(n_stems), str(int(rest))], input=" ".join(str(n) for n in lengths),
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-500:] + res.stderr[-500:]
    return [tuple(int(v) for v in ln.split()[1:]) for ln in res.stdout.split("\n") if ln.startswith("U")]


def test_the_stems_slots_follow_the_lds_size():
    assert [stems_slots(2048, s) // CUS for s in STEMS] == [1, 1, 1]
    assert [stems_slots(1024, s) // CUS for s in STEMS] == [2, 1, 1]
    assert [stems_slots(512, s) // CUS for s in STEMS] == [4, 3, 3]
    assert [stems_slots(256, s) // CUS for s in STEMS] == [4, 4, 4]


@pytest.mark.parametrize("n_stems", STEMS)
@pytest.mark.parametrize("wl", [256, 1024, 2048])
def test_cutter_invariants_under_the_stems_slots(emu, wl, n_stems):
    h, f = wl // 2, tile(wl)
    lengths = lengths_of(h)
    n_blocks = [-(-n // h) for n in lengths]
    lib_in = np.concatenate([[0], np.cumsum(lengths)])
    for cus, rest in ((CUS, True), (1, False), (8, True)):
        units = cut(emu, lengths, wl, stems_slots(wl, n_stems, cus), n_stems, rest)
        blocks = n_stems + int(rest)
        own = {}
        for clip, in_off, n, out_off, mask_off, b0, b1 in units:
            # the record carries the clip's place: clips, masks (S per clip) and output blocks back to back
            assert (in_off, n, out_off) == (lib_in[clip], lengths[clip], blocks * lib_in[clip])
            assert mask_off == n_stems * sum(mask_frames(m, wl) * (h + 1) for m in lengths[:clip])
            assert b0 % 2 == 0 and 0 <= b0 < b1 <= n_blocks[clip], (clip, b0, b1)      # every unit starts on an even block
            assert b1 % 2 == 0 or b1 == n_blocks[clip], (clip, b0, b1)                   # ... and only a clip's last may end on an odd one
            own.setdefault(clip, []).append((b0, b1))
        assert set(own) == {i for i, n in enumerate(lengths) if n > 0}                   # length 0 gives no unit
        for clip, segs in own.items():
            segs.sort()
            assert segs[0][0] == 0 and segs[-1][1] == n_blocks[clip]
            assert all(a[1] == b[0] for a, b in zip(segs, segs[1:])), (clip, segs)       # an exact cover, in order
            if len(segs) > 1:
                for b0, b1 in segs:
                    assert -(-(b1 - b0) // 2) >= 2 * f - 1, (clip, b0, b1)               # no cut unit below 2 F - 1 pieces: the floor 4 F - 3
        pieces = [-(-(b1 - b0) // 2) for *_, b0, b1 in units]
        assert pieces == sorted(pieces, reverse=True)                                    # ordered for the deal
        assert max(pieces) <= max(4 * f - 3, -(-sum(-(-b // 2) for b in n_blocks) // (8 * stems_slots(wl, n_stems, cus))))
        if cus == CUS:
            assert any(len(s) > 1 for s in own.values())                                 # slots to fill: the long clips are cut


# ------------------------------------------------------------------------------------------------------------------ the walk
def payload(wl, x, m, rest, slots, per_slot):
    """x (N,), m (S, W/2 + 1, T) -> the walk's input (masks in ZAFX_LAYOUT_TF, as the device reads them)."""
    x, mt = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(np.asarray(m, np.float32).transpose(0, 2, 1))
    assert mt.shape[1:] == (mask_frames(len(x), wl), wl // 2 + 1)
    return (struct.pack("<7i", wl, len(x), mt.shape[0], int(rest), tile(wl), slots, per_slot) + zafx.hamming(wl).astype(np.float32).tobytes() + x.tobytes()
            + mt.tobytes())


def parse(out, n_stems, rest, n):
    n_units = struct.unpack("<i", out[:4])[0]
    y = np.frombuffer(out[4:], np.float32)
    blocks = n_stems + int(rest)
    assert len(y) == 2 * blocks * n
    return n_units, y[:blocks * n].reshape(blocks, n), y[blocks * n:].reshape(blocks, n)


def walk(exe, wl, x, m, rest, slots, per_slot):
    res = subprocess.run([exe, "walk"], input=payload(wl, x, m, rest, slots, per_slot), capture_output=True)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr.decode()[-2000:])
    return parse(res.stdout, m.shape[0], rest, len(x))


def emulate_single(exe, x, w, m):
    data = struct.pack("ii", len(w), len(x)) + np.asarray(w, np.float32).tobytes() + np.ascontiguousarray(x, np.float32).tobytes() + np.ascontiguousarray(m, np.float32).tobytes()
    return np.frombuffer(subprocess.run([exe], input=data, capture_output=True, check=True).stdout, np.float32)


def chain(x, y):
    """((x - y_0) - y_1) - ... in float32, left to right."""
    r = np.asarray(x, np.float32).copy()
    for s in range(len(y)):
        r = r - y[s]
    assert r.dtype == np.float32
    return r


@pytest.mark.parametrize("wl,blocks,tail", [(256, 61, -3), (256, 60, 0), (256, 201, 1), (2048, 29, -5), (2048, 27, 0)])
def test_a_clip_walked_as_units_has_the_bits_of_the_clip_walked_whole_and_of_the_one_mask_emulation(emu, single_emu, wl, blocks, tail):
    n = blocks * (wl // 2) + tail
    w = zafx.hamming(wl)
    x = np.random.default_rng([4, wl, n]).standard_normal(n).astype(np.float32)
    m8 = np.stack([make_mask("unit", wl, n, seed=s) for s in range(8)])
    ones = [emulate_single(single_emu, x, w, m8[s]) for s in range(8)]
    for n_stems in STEMS:
        # slots to spare (the device's, under this stem count): the segment length is the floor
        n_units, y_cut, y_whole = walk(emu, wl, x, m8[:n_stems], True, stems_slots(wl, n_stems), 64)
        assert n_units >= 2
        assert np.array_equal(bits(y_cut), bits(y_whole)), (wl, n, n_stems)
        for s in range(n_stems):
            assert np.array_equal(bits(y_cut[s]), bits(ones[s])), (wl, n, n_stems, s)
        assert np.array_equal(bits(y_cut[n_stems]), bits(chain(x, y_cut[:n_stems]))), (wl, n, n_stems, "rest")
    assert mask_error(y_whole[0], oracle_maskfilter(x, w, m8[0]), x) <= TOL_FFT
    # without the rest: the same stems, no block more
    _, y_cut, y_whole = walk(emu, wl, x, m8[:4], False, stems_slots(wl, 4), 64)
    assert y_cut.shape == (4, n) and np.array_equal(bits(y_cut), bits(y_whole))
    assert all(np.array_equal(bits(y_cut[s]), bits(ones[s])) for s in range(4))


def test_short_clips_walk_as_one_unit_and_a_clip_of_length_0_gives_none(emu, single_emu):
    wl, h = 256, 128
    w = zafx.hamming(wl)
    for n in (0, 1, h - 1, h, h + 1, 2 * h, 2 * h + 1):
        x = np.random.default_rng([5, n]).standard_normal(n).astype(np.float32)
        m = np.stack([make_mask("unit", wl, n, seed=s) for s in range(4)])
        n_units, y_cut, y_whole = walk(emu, wl, x, m, True, stems_slots(wl, 4), 64)
        assert n_units == (1 if n else 0)
        assert np.array_equal(bits(y_cut), bits(y_whole))
        for s in range(4 if n else 0):
            assert np.array_equal(bits(y_cut[s]), bits(emulate_single(single_emu, x, w, m[s]))), (n, s)


def test_the_walk_under_the_sanitizers(tmp_path_factory):
    """The same program built with AddressSanitizer and UndefinedBehaviorSanitizer, run as a program on the edge lengths: the clip, its masks and
    its block end with their allocations, so a read or a write behind any of them is reported.  A clean exit, and the bits of the whole walk."""
    exe = _build(tmp_path_factory, "maskfilter_stems_units_emu_san", "maskfilter_stems_units_emu.cpp",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    for wl in (256, 2048):
        h, f = wl // 2, tile(wl)
        for n in (0, 1, h, 2 * h + 1, 2 * f * h - 1, 2 * f * h, 2 * f * h + 1, 4 * f * h + 3, (8 * f - 5) * h - 3):
            x = np.random.default_rng([13, wl, n]).standard_normal(n).astype(np.float32)
            m = np.stack([make_mask("unit", wl, n, seed=s) for s in range(3)])
            for rest in (False, True):
                n_units, y_cut, y_whole = walk(exe, wl, x, m, rest, stems_slots(wl, 3), 64)
                assert np.array_equal(bits(y_cut), bits(y_whole)), (wl, n, rest)
                if n == (8 * f - 5) * h - 3:
                    assert n_units >= 2
                if rest and n:
                    assert np.array_equal(bits(y_cut[3]), bits(chain(x, y_cut[:3])))
            lengths = [n, 0, 3 * n + 1]
            units = cut(exe, lengths, wl, stems_slots(wl, 3), 3, True)
            assert {u[0] for u in units} == {i for i, v in enumerate(lengths) if v > 0}
