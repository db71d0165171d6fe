"""Ragged batches on the host side (no GPU): the packing of clips of different lengths and the validation that runs before any
device call."""
import numpy as np
import pytest

import zafx
from zafx import _lib, core


def test_pack_ragged_offsets_gaps_and_round_trip():
    rng = np.random.default_rng(7)
    lengths = [0, 1, 31, 32, 33, 1000, 44100, 5]
    clips = [rng.standard_normal(n) for n in lengths]
    packed, offsets, lens = zafx.pack_ragged(clips)
    assert packed.dtype == np.float32 and packed.ndim == 1
    assert lens.tolist() == lengths and offsets.dtype == np.int64
    assert all(o % 32 == 0 for o in offsets.tolist())
    assert offsets[0] == 0 and all(np.diff(offsets) >= lens[:-1])
    used = np.zeros(len(packed), bool)
    for c, o, n in zip(clips, offsets.tolist(), lengths):
        np.testing.assert_array_equal(packed[o:o + n], c.astype(np.float32))
        used[o:o + n] = True
    assert not packed[~used].any()   # every gap is zero
    assert packed.nbytes % 128 == 0


def test_pack_ragged_float64_and_int_clips():
    packed, offsets, lens = zafx.pack_ragged([np.arange(3), np.arange(40, dtype=np.int16)], dtype=np.float64)
    assert packed.dtype == np.float64
    assert offsets.tolist() == [0, 32] and lens.tolist() == [3, 40]
    np.testing.assert_array_equal(packed[32:72], np.arange(40))


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: validation must come first."""
    def forbidden(*a, **k):
        raise AssertionError("the library was asked for a device before the input was validated")
    monkeypatch.setattr(_lib, "load", forbidden)


BAD = [
    ([], "at least one clip"),
    ([np.zeros((2, 3))], "1-D"),
    ([np.zeros(10), np.zeros(4, np.complex64)], "real"),
    (np.zeros(100), "sequence of 1-D clips"),
    ([np.zeros(10), 3.0], "1-D"),
    (5, "sequence of 1-D clips"),
]


@pytest.mark.parametrize("clips,msg", BAD)
def test_stft_ragged_rejects_bad_batches_before_the_device(no_device, clips, msg):
    with pytest.raises(ValueError, match=msg):
        zafx.stft_ragged(clips, np.hanning(256), 128)


@pytest.mark.parametrize("clips,msg", BAD)
def test_mel_ragged_rejects_bad_batches_before_the_device(no_device, clips, msg):
    fb = zafx.melfilterbank(44100, 2048, 64)
    w = zafx.hamming(2048)
    for fn, args in ((zafx.melspectrogram_ragged, (w, 1024, fb)), (zafx.mfcc_ragged, (w, 1024, fb, 20)),
                     (zafx.mel_mfcc_ragged, (w, 1024, fb, 20))):
        with pytest.raises(ValueError, match=msg):
            fn(clips, *args)


@pytest.mark.parametrize("onesided", ["both", None, 2, "abs"])
def test_stft_ragged_rejects_bad_onesided_before_the_device(no_device, onesided):
    with pytest.raises(ValueError, match="onesided"):
        zafx.stft_ragged([np.zeros(100), np.zeros(300)], np.hanning(256), 128, onesided=onesided)


def test_lengths_validation():
    with pytest.raises(ValueError, match="must not be negative"):
        core._as_lengths([3, -1])
    with pytest.raises(ValueError, match="1-D sequence of integers"):
        core._as_lengths([1.5, 2.0])
    with pytest.raises(ValueError, match="1-D sequence of integers"):
        core._as_lengths([[1, 2]])
    assert core._as_lengths([]).dtype == np.int64


def test_header_declares_the_ragged_entry_points():
    assert "zafx_execute_ragged" in _lib.SYMBOLS and "zafx_plan_ragged_layout" in _lib.SYMBOLS
