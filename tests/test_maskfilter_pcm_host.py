"""The PCM mask filter (zafx_execute_masked_pcm, zafx_execute_masked_pcm_ragged) without a GPU: the quantiser and the integer rest of
zafx_maskfilter_pcm.hpp -- the functions the kernels call, compiled by g++ as a stand-alone program, plain and under the sanitizers -- against
the NumPy formula of the contract on every boundary; the refusal predicates of zafx_routes.hpp from both sides of each bound, in the entry
points' order; the header's text, the ctypes signatures, the null-plan calls and the argument checks of the Python layer, the dtype refusals
among them."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from maskfilter_oracle import mask_frames

CSRC = os.path.join(ROOT, "zaf-python_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "host_emu")
EMU_SRC = os.path.join(EMU, "maskfilter_pcm_emu.cpp")
ROUTES_SRC = os.path.join(EMU, "maskfilter_pcm_routes_emu.cpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def numpy_quantise(y):
    """The contract's reference, word for word."""
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isnan(y), 0, np.clip(np.rint(y * np.float32(32768)), -32768, 32767)).astype(np.int16)


def _build(tmp_path_factory, name, flags, src):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-DZAFX_HOST_EMU", "-Wno-unknown-pragmas", "-I", CSRC, *flags, src, "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module", params=["O2", "sanitized"])
def pcm_emu(request, tmp_path_factory):
    """The quantiser program, once at -O2 and once under AddressSanitizer and UndefinedBehaviorSanitizer: every test of the arithmetic runs on both."""
    return _build(tmp_path_factory, "maskfilter_pcm_emu_" + request.param, ["-O2"] if request.param == "O2" else SANITIZE, EMU_SRC)


@pytest.fixture(scope="module")
def routes_emu(tmp_path_factory):
    return _build(tmp_path_factory, "maskfilter_pcm_routes_emu", ["-O2", "-Wall"], ROUTES_SRC)


def _run(exe, mode, data=b""):
    res = subprocess.run([exe, mode], input=data, capture_output=True, timeout=120)
    assert res.returncode == 0 and not res.stderr, res.stderr.decode()[-2000:]
    return res.stdout


def quantise(exe, y):
    return np.frombuffer(_run(exe, "q", np.ascontiguousarray(y, np.float32).tobytes()), np.int32)


# ------------------------------------------------------------------------------------------------------------------ the quantiser
def boundary_values():
    """y = t / 32768 for every t the contract names -- exact in float32: a power-of-two scale --, both signs where it names both."""
    lsb = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5,                 # ties: to even
           32766.5, 32767.0, 32767.5, -32768.0, -32768.5,   # the two ends
           0.0, 1.0, -1.0, 0.49999997, 0.50000006, 32766.498, 32766.502, -32767.5, -32767.498, -32767.502, 40000.0, -40000.0, 1e30, -1e30]
    y = [np.float32(t) / np.float32(32768) for t in lsb]
    y += [np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), np.float32(-0.0), np.float32(1e-42), np.float32(-1e-42),
          np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny]
    return np.array(y, np.float32)


def test_quantiser_on_every_boundary(pcm_emu):
    y = boundary_values()
    got, want = quantise(pcm_emu, y), numpy_quantise(y)
    assert got.tolist() == want.astype(np.int32).tolist(), list(zip(y.tolist(), got.tolist(), want.tolist()))
    # the table of the contract, value by value -- the NumPy formula is held to it as well
    table = {0.5: 0, 1.5: 2, 2.5: 2, -0.5: 0, -1.5: -2, -2.5: -2, 32766.5: 32766, 32767.0: 32767, 32767.5: 32767, -32768.0: -32768, -32768.5: -32768}
    for t, q in table.items():
        one = np.array([np.float32(t) / np.float32(32768)], np.float32)
        assert quantise(pcm_emu, one)[0] == q == numpy_quantise(one)[0], t
    specials = np.array([np.inf, -np.inf, np.nan, -0.0, 1e-42], np.float32)
    assert quantise(pcm_emu, specials).tolist() == [32767, -32768, 0, 0, 0]
    assert 0 < abs(float(np.float32(1e-42))) < float(np.finfo(np.float32).tiny)   # a denormal indeed


def test_quantiser_on_random_values(pcm_emu):
    g = np.random.default_rng(16)
    y = np.concatenate([g.uniform(-1.2, 1.2, 200000), g.standard_normal(50000) * 1e-4, (g.integers(-70000, 70000, 50000) + 0.5) / 32768]).astype(np.float32)
    assert np.array_equal(quantise(pcm_emu, y), numpy_quantise(y).astype(np.int32))


def test_every_int16_value_round_trips(pcm_emu):
    """q(s / 32768) == s for all 65536 values, s / 32768 is the float32 NumPy computes, and a packed sample frame unpacks to its two channels."""
    rec = np.frombuffer(_run(pcm_emu, "s"), np.dtype([("q", np.int32), ("x", np.float32), ("l", np.int32), ("r", np.int32)]))
    s = np.arange(-32768, 32768, dtype=np.int32)
    assert len(rec) == 65536 and np.array_equal(rec["q"], s)
    assert np.array_equal(rec["x"].view(np.uint32), (s.astype(np.float32) / np.float32(32768)).view(np.uint32))
    assert np.array_equal(rec["l"], s) and np.array_equal(rec["r"], -s - 1)
    assert np.array_equal(numpy_quantise(rec["x"]), s.astype(np.int16))


def test_integer_rest_saturates_at_all_four_corners(pcm_emu):
    # the four corners of the (x, q) square -- two saturate by the widest margin there is, two cancel -- and both sides of either clamp
    corners = [(-32768, 32767), (32767, -32768), (-32768, -32768), (32767, 32767)]
    edges = [(0, -32768), (-1, -32768), (-32768, 1), (-32768, 0), (32767, -1), (32767, 0), (-2, 32767), (-1, 32767)]
    inner = [(0, 0), (0, 32767), (1, 32767), (12345, -20000)]
    pairs = np.array(corners + edges + inner, np.int32)
    got = np.frombuffer(_run(pcm_emu, "r", pairs.tobytes()), np.int32)
    want = np.clip(pairs[:, 0].astype(np.int64) - pairs[:, 1], -32768, 32767)
    assert got.tolist() == want.tolist()
    assert got[:4].tolist() == [-32768, 32767, 0, 0]
    assert got[4:12].tolist() == [32767, 32767, -32768, -32768, 32767, 32767, -32768, -32768]   # 32768 and 32767, -32769 and -32768, ...
    diff = pairs[:, 0] - pairs[:, 1]
    exact = (diff >= -32768) & (diff <= 32767)
    assert (~exact).tolist() == [True, True, False, False, True, False, True, False, True, False, True, False, False, False, False, False]
    assert np.array_equal((got + pairs[:, 1])[exact], pairs[:, 0][exact])   # q + rest == x wherever the rest did not saturate
    g = np.random.default_rng(17).integers(-32768, 32768, (100000, 2)).astype(np.int32)
    got = np.frombuffer(_run(pcm_emu, "r", g.tobytes()), np.int32)
    assert np.array_equal(got, np.clip(g[:, 0] - g[:, 1], -32768, 32767))


# ------------------------------------------------------------------------------------------------------------------ the refusals
def _ask(exe, cases):
    text = ""
    for form, kind, lay, ch, mc, ob, a_in, a_mask, a_out, ls in cases:
        text += f"{form} {kind} {lay} {ch} {mc} {ob} {a_in} {a_mask} {a_out} " + (f"{ls[0]}" if form == "e" else f"{len(ls)} {' '.join(str(v) for v in ls)}") + "\n"
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    head, names, *out = res.stdout.strip().split("\n")
    assert len(out) == len(cases)
    return head, names, out


def test_the_refusal_predicates_from_both_sides(routes_emu):
    from zafx import _lib
    mf, mfr, stft, tf, ft = _lib.MASKFILTER, _lib.MASKFILTER_REST, _lib.STFT, _lib.LAYOUT_TF, _lib.LAYOUT_FT
    A = 1 << 20   # an address on every grid
    top = {(1, 1): 1 << 28, (2, 1): 1 << 28, (2, 2): 1 << 27}
    taken, refused = [], []
    for (ch, mc), t in top.items():
        for ob in (2, 4):
            taken += [("e", mf, tf, ch, mc, ob, A, A, A, [t - 1]), ("e", mfr, tf, ch, mc, ob, A, A, A, [0]), ("r", mf, tf, ch, mc, ob, A, A, A, [1]),
                      ("r", mfr, tf, ch, mc, ob, A, A, A, [t - 1, 0, 5]), ("r", mf, tf, ch, mc, ob, A, A, A, [])]
            refused += [(("e", mf, tf, ch, mc, ob, A, A, A, [t]), -1, "2^28" if t == 1 << 28 else "2^27"),
                        (("e", mfr, tf, ch, mc, ob, A, A, A, [t + 1]), -1, "2^28" if t == 1 << 28 else "2^27"),
                        (("r", mf, tf, ch, mc, ob, A, A, A, [t]), 0, "2^28" if t == 1 << 28 else "2^27"),
                        (("r", mfr, tf, ch, mc, ob, A, A, A, [5, 0, t - 1, t + 1, t]), 3, "2^28" if t == 1 << 28 else "2^27")]
    # the grids, from both sides: mono int16 on 2 bytes, stereo int16 on 4, float32 (the masks, a float32 output) on 4
    taken += [("e", mf, tf, 1, 1, 2, A + 2, A, A + 2, [10]), ("e", mf, tf, 1, 1, 2, A + 6, A + 4, A + 2, [10]), ("e", mf, tf, 1, 1, 4, A + 2, A + 4, A + 4, [10]),
              ("e", mf, tf, 2, 1, 2, A + 4, A + 4, A + 4, [10]), ("r", mf, tf, 2, 2, 2, A + 124, A + 4, A + 12, [10]), ("e", mf, tf, 2, 2, 4, A + 4, A, A + 4, [10])]
    refused += [(("e", mf, tf, 1, 1, 2, A + 1, A, A, [10]), -1, "d_pcm must be 2-byte aligned"), (("e", mf, tf, 1, 1, 2, A, A, A + 1, [10]), -1, "d_out must be 2-byte aligned"),
                (("e", mf, tf, 1, 1, 4, A, A, A + 2, [10]), -1, "d_out must be 4-byte aligned (float32)"), (("r", mf, tf, 1, 1, 2, A, A + 2, A, [10]), -1, "d_mask must be 4-byte"),
                (("e", mf, tf, 2, 1, 2, A + 2, A, A, [10]), -1, "d_pcm must be 4-byte aligned (stereo int16"), (("r", mf, tf, 2, 2, 2, A + 2, A, A, []), -1, "d_pcm must be 4-byte"),
                (("e", mf, tf, 2, 1, 2, A, A, A + 2, [10]), -1, "d_out must be 4-byte aligned (stereo int16"), (("e", mf, tf, 2, 2, 4, A, A, A + 2, [10]), -1, "d_out must be 4-byte aligned (float32)"),
                (("e", mf, tf, 2, 2, 2, A, A + 1, A, [10]), -1, "d_mask must be 4-byte")]
    # the channels and the output type, named before a length or a layout; the layout before a length; the kind
    refused += [(("e", mf, tf, 0, 1, 2, A, A, A, [1 << 28]), -1, "n_channels"), (("e", mf, tf, 3, 1, 2, A, A, A, [10]), -1, "n_channels"), (("r", mf, ft, -1, 1, 2, A, A, A, []), -1, "n_channels"),
                (("e", mf, tf, 1, 2, 2, A, A, A, [10]), -1, "mask_channels must be 1 with one channel"), (("r", mfr, tf, 1, 2, 4, A, A, A, [10]), -1, "mask_channels must be 1 with one channel"),
                (("e", mf, tf, 1, 0, 2, A, A, A, [10]), -1, "mask_channels"), (("e", mf, tf, 2, 3, 2, A, A, A, [10]), -1, "mask_channels"), (("r", mf, tf, 2, 0, 2, A, A, A, []), -1, "mask_channels"),
                (("e", mf, tf, 1, 1, 0, A, A, A, [10]), -1, "out_sample_bytes"), (("e", mf, tf, 2, 1, 3, A, A, A, [10]), -1, "out_sample_bytes"), (("r", mf, tf, 2, 2, 8, A, A, A, []), -1, "out_sample_bytes"),
                (("e", mf, tf, 1, 1, 1, A + 1, A, A, [10]), -1, "out_sample_bytes"),
                (("e", mf, ft, 1, 1, 2, A, A, A, [1 << 28]), -1, "ZAFX_LAYOUT_TF"), (("r", mfr, ft, 1, 1, 4, A, A, A, []), -1, "ZAFX_LAYOUT_TF"), (("e", mf, ft, 2, 2, 2, A, A, A, [10]), -1, "ZAFX_LAYOUT_TF"),
                (("r", mfr, ft, 2, 1, 4, A, A, A, [10]), -1, "ZAFX_LAYOUT_TF"),
                (("e", stft, tf, 1, 1, 2, A, A, A, [10]), -1, "plans only"), (("r", stft, ft, 1, 1, 2, A, A, A, [1 << 28]), -1, "plans only"), (("e", _lib.CENTER, tf, 2, 2, 2, A, A, A, [10]), -1, "plans only"),
                (("r", _lib.ISTFT, ft, 2, 1, 4, A, A, A, []), -1, "plans only")]
    head, names, out = _ask(routes_emu, taken + [c for c, _, _ in refused])
    assert head == f"{mf} {mfr} {1 << 28} {1 << 28} {1 << 27}"
    assert names == "k_maskfilter_pcm k_maskfilter_pcm_ragged k_maskfilter_stereo_pcm k_maskfilter_stereo_pcm_ragged"
    assert out[:len(taken)] == ["taken"] * len(taken), [(c, o) for c, o in zip(taken, out) if o != "taken"]
    for (case, clip, text), line in zip(refused, out[len(taken):]):
        assert line.startswith(f"refused {clip}:") and text in line, (case, line)


def test_the_routes_program_under_the_sanitizers(tmp_path_factory):
    from zafx import _lib
    exe = _build(tmp_path_factory, "maskfilter_pcm_routes_emu_san", SANITIZE, ROUTES_SRC)
    text = f"r {_lib.MASKFILTER} {_lib.LAYOUT_TF} 2 2 2 1024 1024 1024 3 5 {1 << 27} 0\ne {_lib.MASKFILTER_REST} {_lib.LAYOUT_TF} 1 1 4 1026 1024 1028 4000\n"
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
    assert "refused 1:" in res.stdout and res.stdout.strip().endswith("taken")


# ------------------------------------------------------------------------------------------------------------------ header, binding, Python layer
def test_header_text_and_binding():
    from zafx import _lib
    import zafx
    header = open(os.path.join(ROOT, "include", "zafx.h")).read()
    assert "zafx_execute_masked_pcm" in header.split("#ifndef ZAFX_H")[0]
    text = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("s / 32768", "BIT-IDENTICAL to zafx_execute_masked / zafx_execute_masked_stereo", "NaN -> 0", "t >= 32767 (+inf too) -> 32767", "t <= -32768 (-inf too) -> -32768",
                   "ties to even", "rest = clamp(x - q(y), -32768, 32767)", "q(y) + rest == x", "stereo int16 arrays 4 bytes",
                   "zafx_execute_pcm, zafx_run_host_pcm and zafx_execute_ragged_pcm go on refusing mask-filter plans"):
        assert phrase in text, phrase
    for name in ("k_maskfilter_pcm", "k_maskfilter_pcm_ragged", "k_maskfilter_stereo_pcm", "k_maskfilter_stereo_pcm_ragged"):
        assert f'"{name}"' in text, name
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"int\s+zafx_execute_masked_pcm\s*\(\s*zafx_plan\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*void\s*\*\s*\w+,\s*int64_t\s+\w+,\s*int64_t\s+\w+,"
                     r"\s*int32_t\s+\w+,\s*int32_t\s+\w+,\s*int32_t\s+\w+\s*\)", code)
    assert re.search(r"int\s+zafx_execute_masked_pcm_ragged\s*\(\s*zafx_plan\s*\*\s*\w+,\s*const void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,"
                     r"\s*const void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*void\s*\*\s*\w+,\s*const int64_t\s*\*\s*\w+,\s*int64_t\s+\w+,\s*int32_t\s+\w+,\s*int32_t\s+\w+,"
                     r"\s*int32_t\s+\w+\)", code)
    assert "#define ZAFX_VERSION 101" in header
    i32 = ctypes.c_int32
    assert _lib.SYMBOLS["zafx_execute_masked_pcm"] == (_lib.SYMBOLS["zafx_execute_masked_stereo"][0], _lib.SYMBOLS["zafx_execute_masked_stereo"][1] + [i32, i32])
    assert _lib.SYMBOLS["zafx_execute_masked_pcm_ragged"] == (_lib.SYMBOLS["zafx_execute_masked_stereo_ragged"][0], _lib.SYMBOLS["zafx_execute_masked_stereo_ragged"][1] + [i32, i32])
    for name in ("execute_masked_pcm", "execute_masked_pcm_ragged"):
        assert callable(getattr(zafx.Plan, name))
    for name in ("maskfilter_pcm", "maskfilter_pcm_batch", "maskfilter_pcm_ragged"):
        assert callable(getattr(zafx, name))
    routes = open(os.path.join(CSRC, "zafx_routes.hpp")).read()
    for name in ("k_maskfilter_pcm", "k_maskfilter_pcm_ragged", "k_maskfilter_stereo_pcm", "k_maskfilter_stereo_pcm_ragged"):
        assert f'"{name}"' in routes
    assert "zafx_maskfilter_pcm.hip" in open(os.path.join(CSRC, "Makefile")).read()
    # the float kernels' translation units know nothing of the sample types
    for unit in ("zafx_maskfilter.hip", "zafx_maskfilter_stems.hip", "zafx_maskfilter_stereo.hip"):
        assert "pcm" not in open(os.path.join(CSRC, unit)).read().lower(), unit


def test_null_plan_is_an_error_with_text(built_library):
    from zafx import _lib
    lib = _lib.load()
    assert lib.zafx_execute_masked_pcm(None, None, None, None, 1, 1000, 1, 1, 2) != 0
    assert b"null plan" in lib.zafx_last_error()
    one = (ctypes.c_int64 * 2)(0, 0)
    assert lib.zafx_execute_masked_pcm_ragged(None, None, one, one, None, one, None, one, 1, 2, 2, 4) != 0
    assert b"null plan" in lib.zafx_last_error()


class _Buf:
    """What the Plan methods read of a device buffer, without a device."""

    def __init__(self, dtype, nbytes=1 << 20):
        self.dtype, self.nbytes, self.ptr = np.dtype(dtype), nbytes, ctypes.c_void_p(1 << 20)


def test_argument_validation_before_the_library_is_loaded(monkeypatch):
    import zafx
    from zafx import _lib

    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    w = zafx.hamming(1024)
    n = 4000
    t = mask_frames(n, 1024)
    mono, stereo = np.zeros((3, n), np.int16), np.zeros((3, n, 2), np.int16)
    m1, m2 = np.ones((3, 513, t), np.float32), np.ones((3, 2, 513, t), np.float32)
    # the dtype refusals: anything but int16 raises and names int16 -- no silent cast
    for bad in (np.float32, np.float64, np.int32, np.uint16, np.int8, np.int64):
        with pytest.raises(ValueError, match="int16"):
            zafx.maskfilter_pcm_batch(mono.astype(bad), w, m1)
        with pytest.raises(ValueError, match="int16"):
            zafx.maskfilter_pcm_batch(stereo.astype(bad), w, m2)
        with pytest.raises(ValueError, match="int16"):
            zafx.maskfilter_pcm(mono[0].astype(bad), w, 512, m1[0])
        with pytest.raises(ValueError, match="clip 1 .* int16"):
            zafx.maskfilter_pcm_ragged([mono[0], mono[1].astype(bad)], w, [m1[0], m1[1]])
    with pytest.raises(ValueError, match="int16"):
        zafx.maskfilter_pcm_batch(mono.tolist(), w, m1)   # a list of Python ints is int64
    for bad in (np.float64, np.int32, np.complex64):
        with pytest.raises(ValueError, match="out_dtype must be int16 or float32"):
            zafx.maskfilter_pcm_batch(mono, w, m1, out_dtype=bad)
        with pytest.raises(ValueError, match="out_dtype must be int16 or float32"):
            zafx.maskfilter_pcm_ragged([mono[0]], w, [m1[0]], out_dtype=bad)
        with pytest.raises(ValueError, match="out_dtype must be int16 or float32"):
            zafx.maskfilter_pcm_batch(mono, w, m1, out=np.empty((3, n), bad))
    # shapes
    with pytest.raises(ValueError, match="mono, .* or interleaved stereo"):
        zafx.maskfilter_pcm_batch(mono[0], w, m1)
    with pytest.raises(ValueError, match="mono, .* or interleaved stereo"):
        zafx.maskfilter_pcm_batch(np.zeros((3, n, 3), np.int16), w, m1)
    for x, m in ((mono, m1), (stereo, m1), (stereo, m2)):
        with pytest.raises(ValueError, match="shape"):
            zafx.maskfilter_pcm_batch(x, w, m[..., :-1])                # a frame short
        with pytest.raises(ValueError, match="shape"):
            zafx.maskfilter_pcm_batch(x, w, m[:2])                      # a clip short
        with pytest.raises(ValueError, match="shape"):
            zafx.maskfilter_pcm_batch(x, w, m, layout="TF")             # the other layout's shape
    with pytest.raises(ValueError, match="shape"):
        zafx.maskfilter_pcm_batch(mono, w, m2)                           # a mask per channel for one channel
    with pytest.raises(ValueError, match="3-D .* or 4-D"):
        zafx.maskfilter_pcm_batch(stereo, w, m1[0])
    with pytest.raises(ValueError, match="real"):
        zafx.maskfilter_pcm_batch(mono, w, m1.astype(np.complex64))
    with pytest.raises(ValueError, match="step_length"):
        zafx.maskfilter_pcm_batch(mono, w, m1, step_length=256)
    with pytest.raises(ValueError, match="window_length"):
        zafx.maskfilter_pcm_batch(np.zeros((1, 9000), np.int16), zafx.hamming(4096), np.ones((1, 2049, 6), np.float32))
    for bad in (np.empty((3, n), np.float64), np.empty((3, 2, n), np.int16), np.empty((2, n), np.int16), np.empty((3, n, 2), np.int16)):
        with pytest.raises(ValueError, match="out must be|out_dtype"):
            zafx.maskfilter_pcm_batch(mono, w, m1, out=bad)
    with pytest.raises(ValueError, match="out must be"):
        zafx.maskfilter_pcm_batch(stereo, w, m2, rest=True, out=np.empty((3, n, 2), np.int16))
    with pytest.raises(ValueError, match="step_length"):
        zafx.maskfilter_pcm(mono[0], w, 256, m1[0])
    with pytest.raises(ValueError, match="mono, .* or interleaved stereo"):
        zafx.maskfilter_pcm(np.zeros((n, 3), np.int16), w, 512, m1[0])
    with pytest.raises(ValueError, match="2-D"):
        zafx.maskfilter_pcm(mono[0], w, 512, m2[0])
    with pytest.raises(ValueError, match="2-D .* or 3-D"):
        zafx.maskfilter_pcm(stereo[0], w, 512, m2)
    # ragged
    clips = [np.zeros(700, np.int16), np.zeros(1, np.int16)]
    masks = [np.ones((513, mask_frames(700, 1024)), np.float32), np.ones((513, 2), np.float32)]
    with pytest.raises(ValueError, match="one entry per clip"):
        zafx.maskfilter_pcm_ragged(clips, w, masks[:1])
    with pytest.raises(ValueError, match="mask 1 must have shape"):
        zafx.maskfilter_pcm_ragged(clips, w, [masks[0], masks[1][:, :1]])
    with pytest.raises(ValueError, match="mask 0 must have shape"):
        zafx.maskfilter_pcm_ragged(clips, w, masks, layout="TF")
    with pytest.raises(ValueError, match="clip 1 .* as clip 0 is"):
        zafx.maskfilter_pcm_ragged([clips[0], np.zeros((5, 2), np.int16)], w, masks)
    with pytest.raises(ValueError, match="not one array"):
        zafx.maskfilter_pcm_ragged(mono, w, masks)
    with pytest.raises(ValueError, match="at least one clip"):
        zafx.maskfilter_pcm_ragged([], w, [])
    # the Plan methods: the dtypes of the three buffers, before anything else
    plan = zafx.Plan.__new__(zafx.Plan)
    for d_pcm, d_mask, d_out, text in ((_Buf(np.float32), _Buf(np.float32), _Buf(np.int16), "int16 samples"), (_Buf(np.int32), _Buf(np.float32), _Buf(np.int16), "int16 samples"),
                                       (_Buf(np.int16), _Buf(np.complex64), _Buf(np.int16), "float32 masks"), (_Buf(np.int16), _Buf(np.float32), _Buf(np.float64), "int16 or float32"),
                                       (_Buf(np.int16), _Buf(np.float32), _Buf(np.int32), "int16 or float32")):
        with pytest.raises(ValueError, match=text):
            zafx.Plan.execute_masked_pcm(plan, d_pcm, d_mask, d_out, 1, 100)
        with pytest.raises(ValueError, match=text):
            zafx.Plan.execute_masked_pcm_ragged(plan, d_pcm, [0], [100], d_mask, [0], d_out, [0])
    # an empty batch is taken, and needs no device
    for x, m, shape in ((mono[:0], m1[:0], (0, n)), (stereo[:0], m2[:0], (0, n, 2))):
        got = zafx.maskfilter_pcm_batch(x, w, m)
        assert got.shape == shape and got.dtype == np.int16
        assert zafx.maskfilter_pcm_batch(x, w, m, out_dtype=np.float32).dtype == np.float32
