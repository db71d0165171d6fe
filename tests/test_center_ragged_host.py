"""Ragged stereo batches of the center / sides extraction on the host side (no GPU): the packing of (N_i, 2) clips of different lengths, the
validation that runs before any device call, the binding of the new entry point, and the cutter that turns a batch into the units k_center's
RAGGED form walks (center_cut_units, zafx_units.hpp, compiled by g++)."""
import os
import subprocess

import numpy as np
import pytest

import zafx
from zafx import _lib

from conftest import ROOT


def test_pack_ragged_stereo_offsets_and_round_trip():
    rng = np.random.default_rng(11)
    lengths = [0, 1, 31, 32, 33, 1000, 44100, 5, 0, 7]
    clips = [rng.standard_normal((n, 2)) for n in lengths]
    packed, offsets, lens = zafx.pack_ragged_stereo(clips)
    assert packed.dtype == np.float32 and packed.shape == (sum(lengths), 2) and packed.flags.c_contiguous
    assert lens.dtype == np.int64 and offsets.dtype == np.int64 and lens.tolist() == lengths
    assert offsets.tolist() == [0] + np.cumsum(lengths)[:-1].tolist()   # back to back: the running sums, no gaps
    for c, o, n in zip(clips, offsets.tolist(), lengths):
        np.testing.assert_array_equal(packed[o:o + n], c.astype(np.float32))


def test_pack_ragged_stereo_takes_integer_clips_and_lists():
    packed, offsets, lens = zafx.pack_ragged_stereo([np.arange(6, dtype=np.int16).reshape(3, 2), [[1.5, -2.5]]])
    assert offsets.tolist() == [0, 3] and lens.tolist() == [3, 1]
    np.testing.assert_array_equal(packed, np.array([[0, 1], [2, 3], [4, 5], [1.5, -2.5]], np.float32))


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: validation must come first."""
    def forbidden(*a, **k):
        raise AssertionError("the library was asked for a device before the input was validated")
    monkeypatch.setattr(_lib, "load", forbidden)


BAD = [
    (5, "sequence"),                                                 # not a sequence
    (np.zeros((100, 2)), "sequence"),                                # one array, not a batch
    ([], "at least one clip"),
    ([np.zeros((4, 2)), np.zeros(10)], "clip 1 .* must be 2-D"),             # wrong rank
    ([np.zeros((4, 2)), np.zeros((2, 4, 2))], "clip 1 .* must be 2-D"),
    ([np.zeros((4, 3))], "clip 0 .* must be stereo"),                        # last axis not 2
    ([np.zeros((4, 2)), np.zeros((4, 2)), np.zeros((4, 1))], "clip 2 .* must be stereo"),
    ([np.zeros((4, 2)), np.zeros((4, 2), np.complex64)], "clip 1 .* must be real"),
    ([np.array([["a", "b"]])], "clip 0 .* must be real"),                    # not numeric
]


@pytest.mark.parametrize("clips,msg", BAD)
def test_bad_batches_are_rejected_before_the_device(no_device, clips, msg):
    with pytest.raises(ValueError, match=msg):
        zafx.pack_ragged_stereo(clips)
    with pytest.raises(ValueError, match=msg):
        zafx.centersides_ragged(clips, zafx.hamming(256))


def test_window_and_hop_rules_are_those_of_centersides_batch(no_device):
    clips = [np.zeros((100, 2)), np.zeros((7, 2))]
    with pytest.raises(ValueError, match="power-of-two window_length"):
        zafx.centersides_ragged(clips, zafx.hamming(4096))
    with pytest.raises(ValueError, match="step_length must be window_length / 2"):
        zafx.centersides_ragged(clips, zafx.hamming(1024), 256)


def test_binding_declares_the_entry_point():
    assert "zafx_execute_center_ragged" in _lib.SYMBOLS
    res, args = _lib.SYMBOLS["zafx_execute_center_ragged"]
    assert len(args) == 7
    assert callable(zafx.Plan.execute_center_ragged)


# ------------------------------------------------------------------------------------------------------------------ the unit cutter
@pytest.fixture(scope="module")
def cutter(tmp_path_factory):
    exe = tmp_path_factory.mktemp("center_units") / "center_units_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "center_units_emu.cpp"), "-o", str(exe)], check=True)

    def run(lengths, wl, f, slots):
        res = subprocess.run([str(exe), str(wl), str(f), str(slots), "-"], input=" ".join(str(n) for n in lengths), capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-500:] + res.stderr[-500:]
        lines = res.stdout.split("\n")
        assert lines[0].startswith("S ")
        return int(lines[0][2:]), [tuple(int(v) for v in ln.split()) for ln in lines[1:] if ln]
    return run


def length_lists(h):
    rng = np.random.default_rng(5)
    return {
        "all equal": [44100] * 40,
        "1 .. 3H and one very long": rng.integers(1, 3 * h + 1, 60).tolist() + [3_000_000] + rng.integers(1, 3 * h + 1, 20).tolist(),
        "a zero-length clip": [5000, 0, 70000, 0],
        "a single clip": [123457],
        "a single short clip": [1],
        "5000 tiny clips": rng.integers(1, 2 * h, 5000).tolist(),
        "only zero lengths": [0, 0, 0],
        "mixed, around the segment length": [h * k + d for k in (1, 13, 14, 15, 28, 29, 30, 57, 58, 59, 200) for d in (-1, 0, 1)],
    }


@pytest.mark.parametrize("slots", [1, 256, 1024])
@pytest.mark.parametrize("wl,f", [(256, 8), (1024, 8), (2048, 4), (512, 4)])
def test_cutter_invariants(cutter, wl, f, slots):
    h = wl // 2
    for what, lengths in length_lists(h).items():
        seg, units = cutter(lengths, wl, f, slots)
        n_blocks = [(n + h - 1) // h for n in lengths]
        assert seg >= 2 * f - 1, what
        covered = [np.zeros(nb, np.int32) for nb in n_blocks]
        sizes = []
        for clip, b0, b1, n in units:
            assert n == lengths[clip] and 0 <= b0 < b1 <= n_blocks[clip], (what, clip, b0, b1)
            covered[clip][b0:b1] += 1
            whole = b0 == 0 and b1 == n_blocks[clip]
            assert whole or b1 - b0 >= 2 * f - 1, (what, clip, b0, b1)   # a cut clip's segments keep two tiles
            assert b1 - b0 <= seg or whole, (what, clip, b0, b1)
            assert whole == (n_blocks[clip] <= seg), (what, clip)        # a clip of at most S blocks is one unit, a longer one is cut
            sizes.append(b1 - b0)
        for clip, c in enumerate(covered):   # every block in exactly one unit; a zero-length clip has none
            assert (c == 1).all(), (what, clip)
        assert {u[0] for u in units} == {i for i, n in enumerate(lengths) if n > 0}, what
        assert sizes == sorted(sizes, reverse=True), what
        # near-equal segments: those of one clip differ by at most one block
        own = {}
        for clip, b0, b1, _ in units:
            own.setdefault(clip, []).append(b1 - b0)
        for clip, segs in own.items():
            assert max(segs) - min(segs) <= 1, (what, clip)


def test_cutter_gives_about_four_units_per_slot_and_more_where_blocks_allow(cutter):
    """1024 clips of 5 - 15 s at W = 2048 on 256 slots (the measured batch): at least 4 units per slot."""
    lengths = np.random.default_rng(0).integers(5 * 44100, 15 * 44100 + 1, 1024).tolist()
    seg, units = cutter(lengths, 2048, 4, 256)
    assert len(units) >= 4 * 256 and seg >= 2 * 4 - 1
