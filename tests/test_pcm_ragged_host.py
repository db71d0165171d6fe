"""Ragged batches of integer PCM on the host side (no GPU): the packing, the validation that runs before any device call, the argument
checks of Plan.execute_ragged_pcm, the declaration of zafx_execute_ragged_pcm, and the group cutter of its convert-first route
(rg_pcm_groups in zafx_ragged_table.hpp, compiled by g++ -- once more under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
program)."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import zafx
from zafx import _lib, core

from conftest import ROOT


# ------------------------------------------------------------------------------------------------------------------ the packing
@pytest.mark.parametrize("channels", [None, 1, 2, 5])
@pytest.mark.parametrize("dtype", [np.int16, np.int32])
def test_pack_ragged_pcm_offsets_gaps_and_round_trip(channels, dtype):
    rng = np.random.default_rng(11)
    lengths = [0, 1, 63, 64, 65, 1000, 44100, 5]
    info = np.iinfo(dtype)
    clips = [rng.integers(info.min, info.max, (n,) if channels is None else (n, channels), dtype=dtype, endpoint=True) for n in lengths]
    packed, offsets, lens = zafx.pack_ragged_pcm(clips)
    assert packed.dtype == dtype and packed.shape[1:] == (() if channels is None else (channels,))
    assert lens.tolist() == lengths and offsets.dtype == np.int64 and lens.dtype == np.int64
    assert all(o % 64 == 0 for o in offsets.tolist())
    assert offsets[0] == 0 and all(np.diff(offsets) >= lens[:-1])
    used = np.zeros(len(packed), bool)
    for c, o, n in zip(clips, offsets.tolist(), lengths):
        np.testing.assert_array_equal(packed[o:o + n], c)   # exact
        used[o:o + n] = True
    assert not packed[~used].any()   # every gap is zero
    assert len(packed) % 64 == 0 and packed.flags.c_contiguous


def test_pack_ragged_pcm_is_never_empty():
    packed, offsets, lens = zafx.pack_ragged_pcm([np.zeros(0, np.int16)])
    assert packed.shape == (64,) and not packed.any() and offsets.tolist() == [0] and lens.tolist() == [0]
    packed, _, _ = zafx.pack_ragged_pcm([np.zeros((0, 2), np.int16), np.zeros((0, 2), np.int16)])
    assert packed.shape == (64, 2)


def test_pack_ragged_pcm_rejects_mixed_batches():
    a16, a32 = np.zeros(10, np.int16), np.zeros(10, np.int32)
    with pytest.raises(ValueError, match="clip 1 of the ragged PCM batch must be int16 as clip 0"):
        zafx.pack_ragged_pcm([a16, a32])
    with pytest.raises(ValueError, match="clip 2 of the ragged PCM batch must have 2 channel"):
        zafx.pack_ragged_pcm([np.zeros((4, 2), np.int16), np.zeros((9, 2), np.int16), np.zeros((4, 1), np.int16)])
    with pytest.raises(ValueError, match="clip 1 of the ragged PCM batch must have 1 channel"):
        zafx.pack_ragged_pcm([a16, np.zeros((4, 2), np.int16)])
    with pytest.raises(ValueError, match="at least one clip"):
        zafx.pack_ragged_pcm([])


# ------------------------------------------------------------------------------------------------------------------ validation first
@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: validation must come first."""
    def forbidden(*a, **k):
        raise AssertionError("the library was asked for a device before the input was validated")
    monkeypatch.setattr(_lib, "load", forbidden)


BAD = [
    ([], "at least one clip"),
    ([np.zeros(10, np.float32)], "clip 0 of the ragged PCM batch must be int16 or int32"),              # float clips
    ([np.zeros(10, np.int16), np.zeros(10)], "clip 1 of the ragged PCM batch must be int16 or int32"),
    ([np.zeros(10, np.int16), np.zeros(10, np.int64)], "clip 1 .* must be int16 or int32"),
    ([np.zeros((2, 3, 2), np.int16)], "clip 0 of the ragged PCM batch must be 1-D or \\(N, C\\), got 3-D"),   # 3-D items
    ([np.zeros(10, np.int16), np.int16(3)], "clip 1 .* got 0-D"),
    (np.zeros(100, np.int16), "sequence of \\(N,\\) or \\(N, C\\) integer clips, not one array"),         # one array, not a batch
    (5, "sequence of \\(N,\\) or \\(N, C\\) integer clips"),                                              # not a sequence
    ([np.zeros(10, np.int16), np.zeros(10, np.int32)], "one dtype per batch"),
    ([np.zeros((10, 2), np.int16), np.zeros((10, 3), np.int16)], "one channel count per batch"),
]


def _calls():
    fb = zafx.melfilterbank(44100, 2048, 64)
    w = zafx.hamming(2048)
    return [(zafx.stft_pcm_ragged, (w, 1024)), (zafx.melspectrogram_pcm_ragged, (w, 1024, fb)), (zafx.mfcc_pcm_ragged, (w, 1024, fb, 20)),
            (zafx.mel_mfcc_pcm_ragged, (w, 1024, fb, 20)), (zafx.mdct_pcm_ragged, (zafx.kaiser_bessel_derived(2048),))]


@pytest.mark.parametrize("clips,msg", BAD)
def test_every_function_rejects_bad_batches_before_the_device(no_device, clips, msg):
    for fn, args in _calls():
        if fn is zafx.mdct_pcm_ragged and isinstance(clips, list) and not clips:
            assert fn(clips, *args) == []   # (an empty list gives an empty list where the float twin does: mdct_ragged)
            continue
        with pytest.raises(ValueError, match=msg):
            fn(clips, *args)


def test_the_empty_batch_follows_the_float_twins(no_device):
    w, fb = zafx.hamming(2048), zafx.melfilterbank(44100, 2048, 64)
    with pytest.raises(ValueError, match="at least one clip"):
        zafx.stft_ragged([], w, 1024)
    with pytest.raises(ValueError, match="at least one clip"):
        zafx.stft_pcm_ragged([], w, 1024)
    with pytest.raises(ValueError, match="at least one clip"):
        zafx.melspectrogram_ragged([], w, 1024, fb)
    with pytest.raises(ValueError, match="at least one clip"):
        zafx.melspectrogram_pcm_ragged([], w, 1024, fb)
    assert zafx.mdct_ragged([], zafx.kaiser_bessel_derived(2048)) == [] == zafx.mdct_pcm_ragged((), zafx.kaiser_bessel_derived(2048), layout="TF")
    with pytest.raises(ValueError, match="even window_length"):
        zafx.mdct_pcm_ragged([], np.ones(1023))   # (the window is checked for an empty batch too)


@pytest.mark.parametrize("onesided", ["both", None, 2, "abs"])
def test_stft_pcm_ragged_rejects_bad_onesided_before_the_device(no_device, onesided):
    with pytest.raises(ValueError, match="onesided"):
        zafx.stft_pcm_ragged([np.zeros(100, np.int16), np.zeros(300, np.int16)], np.hanning(256), 128, onesided=onesided)


def test_no_f64_argument():
    import inspect
    for fn, _ in _calls():
        assert "f64" not in inspect.signature(fn).parameters, fn.__name__


# ------------------------------------------------------------------------------------------------------------------ Plan.execute_ragged_pcm
class FakeLib:
    def __init__(self):
        self.calls = []

    def zafx_execute_ragged_pcm(self, *args):
        self.calls.append(args)
        return 0


@pytest.fixture
def plan(monkeypatch):
    """A float32 mel plan that never met a device: four output elements per sample frame of a clip; the library records its calls."""
    lib = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    p = object.__new__(core.Plan)
    p.kind, p.f64, p.spectrum, p.handle = _lib.MEL, False, 0, None
    p._ragged_offsets = lambda lengths: np.concatenate([[0], np.cumsum(4 * np.asarray(lengths, np.int64))]).astype(np.int64)
    p.lib = lib
    return p


def buf(n, dtype):
    return types.SimpleNamespace(dtype=np.dtype(dtype), nbytes=n * np.dtype(dtype).itemsize, ptr=0)


def test_execute_ragged_pcm_argument_errors(plan):
    ok = dict(d_pcm=buf(200, np.int16), in_offsets=[0, 64], lengths=[50, 36], d_out=buf(4 * 86, np.float32))
    call = lambda **kw: plan.execute_ragged_pcm(**{**ok, **kw})
    with pytest.raises(ValueError, match="one entry per clip"):
        call(in_offsets=[0])
    with pytest.raises(ValueError, match="lengths must not be negative"):
        call(lengths=[50, -1])
    with pytest.raises(ValueError, match="in_offsets must not be negative"):
        call(in_offsets=[-64, 0])
    with pytest.raises(ValueError, match="1-D sequence of integers"):
        call(lengths=[50.0, 36.5])
    with pytest.raises(ValueError, match="int16 or int32 sample frames and a float32 output buffer"):
        call(d_pcm=buf(200, np.float32))
    with pytest.raises(ValueError, match="int16 or int32 sample frames and a float32 output buffer"):
        call(d_out=buf(4 * 86, np.float64))
    with pytest.raises(ValueError, match="n_channels must be at least 1"):
        call(n_channels=0)
    with pytest.raises(ValueError, match="a clip reaches past the end of d_pcm"):
        call(lengths=[50, 137])
    with pytest.raises(ValueError, match="a clip reaches past the end of d_pcm"):
        call(n_channels=2, d_pcm=buf(199, np.int16))        # 99 whole sample frames of two channels: the second clip ends at 100
    with pytest.raises(ValueError, match="d_out is smaller"):
        call(d_out=buf(4 * 86 - 1, np.float32))
    assert plan.lib.calls == []                              # nothing reached the library
    call()
    call(n_channels=2)                                       # (100 sample frames of two channels hold both clips)
    call(d_pcm=buf(400, np.int32), n_channels=2)
    (a, b, c) = plan.lib.calls
    assert a[5:] == (2, 1, 2) and b[5:] == (2, 2, 2) and c[5:] == (2, 2, 4)         # n_clips, n_channels, sample_bytes


# ------------------------------------------------------------------------------------------------------------------ the declaration
def test_header_binding_and_package_agree():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zafx.h")).read(), flags=re.S)
    m = re.search(r"int\s+zafx_execute_ragged_pcm\s*\(([^)]*)\)", text)
    assert m, "include/zafx.h declares zafx_execute_ragged_pcm"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["zafx_plan* plan", "const void* d_pcm", "const int64_t* in_offsets", "const int64_t* lengths", "void* d_out", "int64_t n_clips",
                      "int n_channels", "int sample_bytes"]
    restype, argtypes = _lib.SYMBOLS["zafx_execute_ragged_pcm"]
    import ctypes
    i64p = ctypes.POINTER(ctypes.c_int64)
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_void_p, i64p, i64p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    for name in ("stft_pcm_ragged", "mdct_pcm_ragged", "melspectrogram_pcm_ragged", "mfcc_pcm_ragged", "mel_mfcc_pcm_ragged", "pack_ragged_pcm"):
        assert callable(getattr(zafx, name)) and name in zafx.__doc__
    assert callable(zafx.Plan.execute_ragged_pcm) and "Plan.execute_ragged_pcm" in zafx.__doc__


def test_library_exports_the_entry_point(built_library):
    import ctypes
    lib = ctypes.CDLL(built_library)
    assert hasattr(lib, "zafx_execute_ragged_pcm")
    lib.zafx_version.restype = ctypes.c_int
    assert lib.zafx_version() == 101


# ------------------------------------------------------------------------------------------------------------------ the group cutter
SRC = os.path.join(ROOT, "tests", "host_emu", "pcm_groups_emu.cpp")
INC = os.path.join(ROOT, "zaf-python_amd", "csrc")


def _runner(exe):
    def run(budget, offsets, lengths):
        args = [str(budget)] + [str(v) for pair in zip(offsets, lengths) for v in pair]
        res = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
        lines = res.stdout.strip().split("\n")
        groups = [tuple(int(v) for v in ln.split()) for ln in lines[1:]]
        assert int(lines[0].split()[1]) == len(groups)
        return groups
    return run


@pytest.fixture(scope="module")
def cutter(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pcm_groups") / "pcm_groups_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", INC, SRC, "-o", str(exe)], check=True)
    return _runner(exe)


@pytest.fixture(scope="module")
def cutter_sanitized(tmp_path_factory):
    """The same stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer, run directly."""
    exe = tmp_path_factory.mktemp("pcm_groups_san") / "pcm_groups_emu_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-I", INC, SRC, "-o", str(exe)], check=True)
    return _runner(exe)


def _batches():
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 5000, 40)
    slots = (lens + 63) // 64 * 64
    inc = np.concatenate([[0], np.cumsum(slots)[:-1]])
    perm = rng.permutation(40)
    zero = lens.copy()
    zero[::3] = 0
    return {
        "increasing": (inc, lens),
        "back to back": (np.concatenate([[0], np.cumsum(lens)[:-1]]), lens),
        "shuffled": (inc[perm], lens[perm]),
        "overlapping": (rng.integers(0, 3000, 40), lens),
        "all at one offset": (np.full(40, 128), lens),
        "zero-length clips": (inc, zero),
        "only zero-length clips": (inc, np.zeros(40, np.int64)),
        "one clip": (np.array([77]), np.array([4000])),
        "no clips": (np.zeros(0, np.int64), np.zeros(0, np.int64)),
        "near the top of int64": (np.array([2**63 - 10, 0, 2**62]), np.array([9, 5, 2**62 - 1])),
    }


def check_groups(groups, offsets, lengths, budget):
    offsets, lengths = [int(v) for v in offsets], [int(v) for v in lengths]
    n = len(offsets)
    assert (not groups) == (n == 0)
    nxt = 0
    for first, count, lo, hi in groups:
        assert first == nxt and count >= 1                                  # a partition of the clips, in order; never an empty group
        nxt = first + count
        ids = range(first, first + count)
        assert lo == min(offsets[i] for i in ids) and hi == max(offsets[i] + lengths[i] for i in ids)   # the covered span
        assert hi - lo <= budget or count == 1                               # within the budget, unless it is a single clip
        for i in ids:
            assert 0 <= offsets[i] - lo and offsets[i] - lo + lengths[i] <= hi - lo   # the rebased clip lies inside the span
        if nxt < n:   # greedy: the next clip did not fit
            lo2, hi2 = min(lo, offsets[nxt]), max(hi, offsets[nxt] + lengths[nxt])
            assert hi2 - lo2 > budget
    assert nxt == n


@pytest.mark.parametrize("budget", [0, 1, 4999, 5000, 20000, 2**40])
@pytest.mark.parametrize("name", list(_batches()))
def test_groups_partition_the_clips_within_the_budget(cutter, name, budget):
    offsets, lengths = _batches()[name]
    check_groups(cutter(budget, offsets, lengths), offsets, lengths, budget)


def test_groups_of_known_batches(cutter):
    assert cutter(100, [], []) == []
    assert cutter(100, [0, 64, 128], [50, 36, 10]) == [(0, 2, 0, 100), (2, 1, 128, 138)]
    assert cutter(10, [0, 64], [50, 36]) == [(0, 1, 0, 50), (1, 1, 64, 100)]        # a budget smaller than one clip: one clip per group
    assert cutter(100, [128, 0, 64], [10, 50, 36]) == [(0, 1, 128, 138), (1, 2, 0, 100)]   # offsets that go back: the span is what counts
    assert cutter(1000, [128, 0, 64], [10, 50, 36]) == [(0, 3, 0, 138)]
    assert cutter(0, [5, 5, 5], [0, 0, 0]) == [(0, 3, 5, 5)]                        # empty clips at one place cost nothing


@pytest.mark.parametrize("name", list(_batches()))
def test_groups_under_the_sanitizers(cutter, cutter_sanitized, name):
    offsets, lengths = _batches()[name]
    for budget in (0, 4999, 20000, 2**40):
        assert cutter_sanitized(budget, offsets, lengths) == cutter(budget, offsets, lengths)
