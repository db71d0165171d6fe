"""Mask filter stems (zafx_execute_masked_stems, k_maskfilter_stems) without a GPU: the entry point and its constant in the C-ABI and the
Python mirror, the launcher's refusal predicate at its edges, the argument checks of the Python layer, and the kernel's algorithm -- one
forward transform of a clip, then per stem the caller's mask, the inverse and the overlap-add with the stem's own carry, and the rest's
chain (tests/host_emu/maskfilter_stems_emu.cpp on the kernel's own headers, compiled by g++) -- held bit for bit to the one-mask emulation
(tests/host_emu/maskfilter_emu.cpp) per stem, to the float64 oracle, and to the float32 subtraction chain in NumPy.

Bounds: bit identity per stem and for the rest; against the oracle max|y - ref| <= 1e-5 max(max|ref|, max|x|) per stem (TOL_FFT at
mask_error's level, as tests/test_maskfilter_host.py)."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from maskfilter_oracle import TOL_FFT, make_mask, mask_error, mask_frames, oracle_maskfilter

CSRC = os.path.join(ROOT, "zaf-python_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "host_emu")
WINDOWS = (256, 512, 1024, 2048)
KINDS = ("ones", "uniform", "sparse")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def edge_lengths(wl):
    """The pair, tile and segment edges of k_maskfilter, both parities of the frame count (tests/test_maskfilter_host.py's); F: packed transforms per tile."""
    from zafx import _lib
    h, f = wl // 2, _lib.maskfilter_tile_transforms(wl)
    return [1, h - 1, h, h + 1, 2 * h - 1, 2 * h, 2 * h + 1, 2 * f * h - 1, 2 * f * h, 2 * f * h + 1, 4 * f * h + 3, 44100]


def test_entry_point_and_constant_in_header_and_binding():
    import zafx
    from zafx import _lib
    header = open(os.path.join(ROOT, "include", "zafx.h")).read()
    assert re.search(r"#define ZAFX_MASKFILTER_MAX_STEMS 8\b", header) and re.search(r"#define ZAFX_VERSION 101\b", header)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+zafx_execute_masked_stems\s*\(\s*zafx_plan\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*void\s*\*\s*\w+,"
                     r"\s*int64_t\s+\w+,\s*int64_t\s+\w+,\s*int32_t\s+\w+\)", code)
    res, args = _lib.SYMBOLS["zafx_execute_masked_stems"]
    assert res is ctypes.c_int and len(args) == 7
    assert _lib.MASKFILTER_MAX_STEMS == zafx.MASKFILTER_MAX_STEMS == 8
    assert ctypes.sizeof(_lib.ZafxParams) == 64
    for name in ("execute_masked_stems", "stems_mask_shape", "stems_out_shape"):
        assert callable(getattr(zafx.Plan, name))
    for name in ("maskfilter_stems", "maskfilter_stems_batch"):
        assert callable(getattr(zafx, name))
    # the comment states the shapes, the order of the rest's subtractions, the bit identity, the alignment and what is never read
    text = header[header.index("Stems: n_stems masks"):header.index("int zafx_execute_masked_stems")]
    for phrase in ("(B, n_stems, frames, rows)", "(B, n_stems + 1, n_in)", "((x - y_0) - y_1)", "bit-identical", "4-byte alignment", "behind a mask's last frame",
                   "ZAFX_LAYOUT_TF", "k_maskfilter_stems"):
        assert phrase in text, phrase


def test_null_plan_is_an_error_with_text(built_library):
    from zafx import _lib
    lib = _lib.load()
    assert lib.zafx_version() == 101
    assert lib.zafx_execute_masked_stems(None, None, None, None, 1, 1000, 2) != 0
    assert b"null" in lib.zafx_last_error()


@pytest.fixture(scope="module")
def routes_emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stems_routes") / "stems_routes_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(EMU, "maskfilter_stems_routes_emu.cpp"), "-o", str(exe)], check=True)

    def run(cases):
        res = subprocess.run([str(exe)], input="".join(f"{a} {b} {c}\n" for a, b, c in cases), capture_output=True, text=True, timeout=60)
        assert res.returncode == 0, res.stderr[-2000:]
        lines = res.stdout.strip().split("\n")
        assert len(lines) == len(cases) + 1
        return lines[0], lines[1:]
    return run


def test_the_route_predicate_at_its_edges(routes_emu):
    """Layout (0 FT, 1 TF), stem count and clip length at the edges of what the call takes."""
    tf, ft, top = 1, 0, 1 << 28
    cases = [(tf, 1, 1), (tf, 8, top - 1), (tf, 4, 0), (tf, 0, 1000), (tf, 9, 1000), (tf, -1, 1000), (tf, 1 << 32, 1000), (ft, 1, 1000), (ft, 8, 1000),
             (tf, 1, top), (tf, 8, top + 1), (ft, 0, top)]
    head, out = routes_emu(cases)
    assert head == "k_maskfilter_stems 8"
    assert out[:3] == ["taken"] * 3
    for line in out[3:7]:
        assert line.startswith("refused") and "n_stems" in line and "1 .. 8" in line, line
    for line in out[7:9]:
        assert line.startswith("refused") and "ZAFX_LAYOUT_TF" in line, line
    for line in out[9:11]:
        assert line.startswith("refused") and "2^28" in line, line
    assert "ZAFX_LAYOUT_TF" in out[11]   # the layout is named first


def test_argument_validation_before_the_library_is_loaded(monkeypatch):
    import zafx
    from zafx import _lib

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    w = zafx.hamming(1024)
    n = 4000
    t = mask_frames(n, 1024)
    x, m = np.zeros((3, n), np.float32), np.ones((3, 2, 513, t), np.float32)
    mt = np.ones((3, 2, t, 513), np.float32)
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems_batch(x, w, m[:, :, :, :-1])            # a frame short
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems_batch(x, w, m[:, :, :-1])               # a row short
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems_batch(x, w, m[:2])                      # a clip short
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems_batch(x, w, m, layout="TF")             # the other layout's shape
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems_batch(x, w, mt)                         # ... and the reverse
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems_batch(x, w, mt[:, :, :-1], layout="TF")
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems_batch(x, w, mt[:, :, :, :-1], layout="TF")
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems_batch(x[:, :-1000], w, m)               # the masks of a longer clip
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems_batch(x, w, m[:, 0])                    # no stem axis
    with pytest.raises(ValueError, match="stems"):
        zafx.maskfilter_stems_batch(x, w, m[:, :0])                   # S = 0
    with pytest.raises(ValueError, match="stems"):
        zafx.maskfilter_stems_batch(x, w, np.ones((3, 9, 513, t), np.float32))
    with pytest.raises(ValueError, match="stems"):
        zafx.maskfilter_stems_batch(x, w, np.ones((3, 9, t, 513), np.float32), layout="TF")
    with pytest.raises(ValueError, match="real"):
        zafx.maskfilter_stems_batch(x.astype(np.complex64), w, m)
    with pytest.raises(ValueError, match="real"):
        zafx.maskfilter_stems_batch(x, w, m.astype(np.complex64))
    with pytest.raises(ValueError, match="step_length"):
        zafx.maskfilter_stems_batch(x, w, m, step_length=256)
    with pytest.raises(ValueError, match="window_length"):
        zafx.maskfilter_stems_batch(np.zeros((1, 9000), np.float32), zafx.hamming(4096), np.ones((1, 2, 2049, 6), np.float32))
    with pytest.raises(ValueError, match="window_length"):
        zafx.maskfilter_stems_batch(np.zeros((1, 900), np.float32), zafx.hamming(128), np.ones((1, 2, 65, 16), np.float32))
    with pytest.raises(ValueError):
        zafx.maskfilter_stems_batch(np.zeros((3, n, 2), np.float32), w, m)
    with pytest.raises(ValueError, match="out must"):
        zafx.maskfilter_stems_batch(x, w, m, rest=True, out=np.empty((3, 2, n), np.float32))   # the rest needs a block more
    with pytest.raises(ValueError, match="step_length"):
        zafx.maskfilter_stems(np.zeros(n), w, 256, m[0])
    with pytest.raises(ValueError):
        zafx.maskfilter_stems(np.zeros((n, 2)), w, 512, m[0])
    with pytest.raises(ValueError):
        zafx.maskfilter_stems(np.zeros(n), w, 512, m)
    with pytest.raises(ValueError, match="stems"):
        zafx.maskfilter_stems(np.zeros(n), w, 512, np.ones((9, 513, t)))
    with pytest.raises(ValueError, match="stems"):
        zafx.maskfilter_stems(np.zeros(n), w, 512, np.ones((0, 513, t)))
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_stems(np.zeros(n), w, 512, m[0, :, :, 1:])


def _build(tmp_path_factory, name, src, flags):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-DZAFX_HOST_EMU", "-I", CSRC, *flags, os.path.join(EMU, src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def stems_emu(tmp_path_factory):
    return _build(tmp_path_factory, "maskfilter_stems_emu", "maskfilter_stems_emu.cpp", ["-O2"])


@pytest.fixture(scope="module")
def single_emu(tmp_path_factory):
    return _build(tmp_path_factory, "maskfilter_emu", "maskfilter_emu.cpp", ["-O2"])


def payload(x, w, m, rest):
    """x (N,), m (S, W/2 + 1, T) -> the stems emulation's input."""
    x, m = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(m, np.float32)
    assert m.shape[1:] == (len(w) // 2 + 1, mask_frames(len(x), len(w)))
    return struct.pack("iiii", len(w), len(x), m.shape[0], int(rest)) + np.asarray(w, np.float32).tobytes() + x.tobytes() + m.tobytes()


def emulate_stems(exe, x, w, m, rest):
    res = subprocess.run([exe], input=payload(x, w, m, rest), capture_output=True, check=True)
    return np.frombuffer(res.stdout, np.float32).reshape(m.shape[0] + int(rest), len(x))


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


@pytest.fixture(scope="module")
def singles(single_emu):
    """The one-mask emulation and the oracle per (W, N, kind), computed once and shared: -> (bits of the emulation, float64 reference)."""
    import zafx
    memo = {}

    def get(wl, n, kind, x):
        key = (wl, n, kind)
        if key not in memo:
            w, m = zafx.hamming(wl), make_mask(kind, wl, n)
            memo[key] = (emulate_single(single_emu, x, w, m), oracle_maskfilter(x, w, m))
        return memo[key]
    return get


@pytest.mark.parametrize("wl", WINDOWS)
def test_stems_against_the_single_mask_emulation_and_the_oracle(stems_emu, singles, wl):
    """S = 1, 3 and 8 at the pair, tile and segment edges, the three mask kinds mixed over the stems (stem s takes kind (s + S) mod 3)."""
    import zafx
    w = zafx.hamming(wl)
    worst = 0.0
    for n in edge_lengths(wl):
        x = np.random.default_rng([11, wl, n]).standard_normal(n).astype(np.float32)
        for stems in (1, 3, 8):
            kinds = [KINDS[(s + stems) % 3] for s in range(stems)]
            m = np.stack([make_mask(k, wl, n) for k in kinds])
            got = emulate_stems(stems_emu, x, w, m, True)
            assert got.shape == (stems + 1, n)
            for s, kind in enumerate(kinds):
                one, ref = singles(wl, n, kind, x)
                assert np.array_equal(bits(got[s]), bits(one)), (wl, n, stems, s, kind)
                err = mask_error(got[s], ref, x)
                worst = max(worst, err)
                assert err <= TOL_FFT, (wl, n, stems, s, kind, err)
            assert np.array_equal(bits(got[stems]), bits(chain(x, got[:stems]))), (wl, n, stems, "rest")
            if n in (1, 2 * wl + 1):   # without the rest: the same stems, no block more
                assert np.array_equal(bits(emulate_stems(stems_emu, x, w, m, False)), bits(got[:stems])), (wl, n, stems)
    print(f"W={wl}: worst error {worst:.3e} of the level")


def test_stems_fixed_values(stems_emu):
    """A stem of zeros is exact zeros whatever its neighbours; silence gives exact zeros under wild finite masks, the rest included."""
    import zafx
    wl, n = 512, 3001
    w = zafx.hamming(wl)
    x = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    m = np.stack([make_mask("unit", wl, n, seed=1), np.zeros_like(make_mask("ones", wl, n)), make_mask("unit", wl, n, seed=2)])
    got = emulate_stems(stems_emu, x, w, m, True)
    assert not got[1].any() and got[0].any() and got[2].any()
    assert np.array_equal(bits(got[3]), bits(chain(x, got[:3])))
    wild = np.stack([make_mask("unit", wl, n, seed=s) * np.float32(1e30) - np.float32(4e29) for s in range(3)])
    assert not emulate_stems(stems_emu, np.zeros(n, np.float32), w, wild, True).any()


def test_stems_emulation_under_the_sanitizers(tmp_path_factory):
    """The emulation as a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, run as such on the shortest clip, a
    tile edge and an odd length with three stems and the rest: a clean exit and every stem within the bound."""
    import zafx
    exe = _build(tmp_path_factory, "maskfilter_stems_emu_san", "maskfilter_stems_emu.cpp",
                 ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    for wl, n in ((256, 1), (2048, 8 * 1024), (512, 3001)):
        w = zafx.hamming(wl)
        x = np.random.default_rng([13, wl, n]).standard_normal(n).astype(np.float32)
        m = np.stack([make_mask("unit", wl, n, seed=s) for s in range(3)])
        res = subprocess.run([exe], input=payload(x, w, m, True), capture_output=True)
        assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
        got = np.frombuffer(res.stdout, np.float32).reshape(4, n)
        for s in range(3):
            assert mask_error(got[s], oracle_maskfilter(x, w, m[s]), x) <= TOL_FFT
        assert np.array_equal(bits(got[3]), bits(chain(x, got[:3])))
