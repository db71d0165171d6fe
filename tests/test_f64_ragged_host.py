"""Ragged float64 batches on the host side (no GPU): the 8-frame tiling of a batch -- what zafx_execute_ragged uploads for k_stft_ft8_f64's
RAGGED form (zafx_ragged_table.hpp at tile_frames = 8) -- from tests/host_emu/ragged_table_emu.cpp built under AddressSanitizer and
UndefinedBehaviorSanitizer (a stand-alone program: nothing is preloaded), and the validation the f64=True calls run before any device call."""
import os
import subprocess

import numpy as np
import pytest

import zafx
from zafx import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HOP = 2048, 1024


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = tmp_path_factory.mktemp("f64_ragged_table") / "ragged_table_emu_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    os.path.join(ROOT, "zaf-python_amd", "csrc"), os.path.join(ROOT, "tests", "host_emu", "ragged_table_emu.cpp"), "-o", str(exe)], check=True)

    def run(tile_frames, frames):
        res = subprocess.run([str(exe), str(tile_frames)] + [str(t) for t in frames], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
        tiles, first, clip_of = res.stdout.strip().split("\n")
        assert tiles.startswith("tiles ") and first.startswith("first") and clip_of.startswith("clip_of")
        return int(tiles.split()[1]), [int(v) for v in first.split()[1:]], [int(v) for v in clip_of.split()[1:]]
    return run


def stft_frames(n, hop=HOP, w=W):
    """zaf.py:99-112 (oracle.stft_num_frames): a clip of length 0 still has frames."""
    from oracle import zaf_oracle as orc
    return orc.stft_num_frames(n, w, hop)


def test_table_of_8_frame_tiles(table):
    """Clips of no samples (they still own a tile) and of T = 1, 8, 9 frames among longer ones: every tile owned once, in clip order."""
    frames = [stft_frames(0), 1, 8, 9, stft_frames(0), 15, 16, 17, 100, 1]
    tiles, first, clip_of = table(8, frames)
    own = [-(-t // 8) for t in frames]
    assert own[1:4] == [1, 1, 2] and own[0] >= 1
    assert tiles == sum(own) == len(clip_of)
    assert first == np.concatenate([[0], np.cumsum(own)[:-1]]).tolist()
    assert clip_of == [c for c, k in enumerate(own) for _ in range(k)]


def test_8_and_16_frame_tables_of_one_batch_differ_only_in_the_tiling(table):
    frames = [1, 8, 9, 16, 17, 33]
    t8, first8, _ = table(8, frames)
    t16, first16, _ = table(16, frames)
    assert t8 == 1 + 1 + 2 + 2 + 3 + 5 and t16 == 1 + 1 + 1 + 1 + 2 + 3
    assert first8 == [0, 1, 2, 4, 6, 9] and first16 == [0, 1, 2, 3, 4, 6]


# ------------------------------------------------------------------------------------------------------------------ validation, f64=True
@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: validation must come first."""
    def forbidden(*a, **k):
        raise AssertionError("the library was asked for a device before the input was validated")
    monkeypatch.setattr(_lib, "load", forbidden)


BAD = [
    ([], "at least one clip"),
    ([np.zeros((2, 3))], "1-D"),
    ([np.zeros(10), np.zeros(4, np.complex128)], "real"),
    (np.zeros(100), "sequence of 1-D clips"),
    ([np.zeros(10), 3.0], "1-D"),
    (5, "sequence of 1-D clips"),
]


@pytest.mark.parametrize("clips,msg", BAD)
def test_f64_ragged_calls_reject_bad_batches_before_the_device(no_device, clips, msg):
    fb = zafx.melfilterbank(44100, W, 128)
    ham, kbd = zafx.hamming(W), zafx.kaiser_bessel_derived(W)
    calls = [(zafx.stft_ragged, (ham, HOP)), (zafx.melspectrogram_ragged, (ham, HOP, fb)), (zafx.mfcc_ragged, (ham, HOP, fb, 20)),
             (zafx.mel_mfcc_ragged, (ham, HOP, fb, 20))]
    if not (isinstance(clips, list) and not clips):   # (mdct_ragged of no clips is no arrays: tests/test_mdct_ragged_host.py)
        calls.append((zafx.mdct_ragged, (kbd,)))
    for fn, args in calls:
        with pytest.raises(ValueError, match=msg):
            fn(clips, *args, f64=True)


@pytest.mark.parametrize("onesided", ["both", None, 2, "abs"])
def test_f64_stft_ragged_rejects_bad_onesided_before_the_device(no_device, onesided):
    with pytest.raises(ValueError, match="onesided"):
        zafx.stft_ragged([np.zeros(100), np.zeros(300)], zafx.hamming(W), HOP, onesided=onesided, f64=True)


def test_f64_mdct_ragged_window_rules_before_the_device(no_device):
    with pytest.raises(ValueError, match="even window_length"):
        zafx.mdct_ragged([np.zeros(100), np.zeros(300)], np.ones(1023), f64=True)


def test_the_route_is_documented_where_callers_look():
    for fn in (zafx.stft_ragged, zafx.mdct_ragged, zafx.melspectrogram_ragged, zafx.mfcc_ragged):
        assert "_f64_ragged" in fn.__doc__, fn.__name__
    header = open(os.path.join(ROOT, "include", "zafx.h")).read()
    assert "ZAFX_RAGGED_F64_NATIVE" in header and "k_stft_ft8_f64_ragged" in header
    assert "zafx_execute_ragged" in _lib.SYMBOLS   # (no entry point of its own: the export count stays)
