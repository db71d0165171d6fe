"""Ragged batches of the MDCT on the host side (no GPU): the export, the validation that runs before any device call, the empty batch, and
the table of 32-frame tiles zafx_execute_ragged uploads for k_mdct_ft32's RAGGED form (zafx_ragged_table.hpp, compiled by g++)."""
import os
import subprocess

import numpy as np
import pytest

import zafx
from zafx import _lib

from conftest import ROOT


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: validation must come first."""
    def forbidden(*a, **k):
        raise AssertionError("the library was asked for a device before the input was validated")
    monkeypatch.setattr(_lib, "load", forbidden)


def test_mdct_ragged_is_exported():
    assert callable(zafx.mdct_ragged)
    assert "mdct_ragged" in zafx.__doc__
    assert "zafx_execute_ragged" in _lib.SYMBOLS   # (no entry point of its own: the export count stays)


BAD = [
    ([np.zeros((2, 3))], "1-D"),                              # 2-D clips
    ([np.zeros(10), np.zeros((4, 2))], "clip 1 .* must be 1-D"),
    (np.zeros(100), "sequence of 1-D clips"),                 # one array, not a batch
    (5, "sequence of 1-D clips"),                             # not a sequence
    # a mismatched dtype request, of the clips: float32 / float64 arithmetic asked of clips that are not real numbers
    ([np.zeros(10), np.zeros(4, np.complex64)], "real"),
    ([np.array(["a", "b"])], "real"),
]


@pytest.mark.parametrize("clips,msg", BAD)
def test_mdct_ragged_rejects_bad_batches_before_the_device(no_device, clips, msg):
    for f64 in (False, True):
        with pytest.raises(ValueError, match=msg):
            zafx.mdct_ragged(clips, zafx.kaiser_bessel_derived(2048), f64=f64)


def test_mdct_ragged_window_rules_are_those_of_mdct_batch(no_device):
    clips = [np.zeros(100), np.zeros(300)]
    with pytest.raises(ValueError, match="even window_length"):
        zafx.mdct_ragged(clips, np.ones(1023))
    with pytest.raises(ValueError, match="even window_length"):
        zafx.mdct_ragged([], np.ones(1023))                # (the window is checked for an empty batch too)
    with pytest.raises(ValueError, match="2 ... 8192"):
        zafx.mdct_ragged(clips, np.ones(8194))
    with pytest.raises(ValueError, match="1-D"):
        zafx.mdct_ragged(clips, np.ones((2, 512)))
    # a mismatched dtype request, of the plan: float64 (f64=True) asked for a window only the float32 kernels take
    with pytest.raises(ValueError, match="f64=True takes windows"):
        zafx.mdct_ragged(clips, np.ones(4098), f64=True)
    with pytest.raises(ValueError, match="f64=True takes windows"):
        zafx.mdct_batch(np.zeros((2, 100)), np.ones(4098), f64=True)   # (the same rule, the same words)


def test_mdct_ragged_of_no_clips_is_no_arrays(no_device):
    assert zafx.mdct_ragged([], zafx.kaiser_bessel_derived(2048)) == []
    assert zafx.mdct_ragged((), zafx.kaiser_bessel_derived(512), layout="TF", f64=True) == []


# ------------------------------------------------------------------------------------------------------------------ the tile table
@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ragged_table") / "ragged_table_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "ragged_table_emu.cpp"), "-o", str(exe)], check=True)

    def run(tile_frames, frames):
        res = subprocess.run([str(exe), str(tile_frames)] + [str(t) for t in frames], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-500:] + res.stderr[-500:]
        tiles, first, clip_of = res.stdout.strip().split("\n")
        return int(tiles.split()[1]), [int(v) for v in first.split()[1:]], [int(v) for v in clip_of.split()[1:]]
    return run


def mdct_frames(n, w):
    return -(-n // (w // 2)) + 1   # zaf.py:1029-1033; a clip of length 0 has one frame


@pytest.mark.parametrize("w", [512, 1024, 2048])
def test_table_of_32_frame_tiles(table, w):
    m = w // 2
    lengths = [0, 1, m - 1, m, m + 1, 30 * m + 1, 31 * m, 31 * m + 1, 63 * m + 1, 44100, 123457, 0, 49999, 17]
    frames = [mdct_frames(n, w) for n in lengths]
    assert frames[:9] == [1, 2, 2, 2, 3, 32, 32, 33, 65]
    tiles, first, clip_of = table(32, frames)
    own = [-(-t // 32) for t in frames]
    assert own[:9] == [1, 1, 1, 1, 1, 1, 1, 2, 3]          # length 0: exactly one tile; T = 33: a second tile for one frame
    assert tiles == sum(own) == len(clip_of)
    assert first == np.concatenate([[0], np.cumsum(own)[:-1]]).tolist()
    assert clip_of == [c for c, k in enumerate(own) for _ in range(k)]   # every tile owned once, in clip order


def test_table_of_16_frame_tiles_is_what_the_stft_kernels_get(table):
    frames = [1, 16, 17, 32, 33, 100]
    tiles, first, clip_of = table(16, frames)
    assert tiles == 1 + 1 + 2 + 2 + 3 + 7 and first == [0, 1, 2, 4, 6, 9]
    assert clip_of == [0, 1, 2, 2, 3, 3, 4, 4, 4] + [5] * 7
