"""Ragged batches of the IMDCT on the host side (no GPU): the export and the binding of the new entry point, the validation that runs before
any device call, the empty batch, and the cutter and the deal that turn a batch of coefficient blocks into the table k_imdct's RAGGED form walks
(imdct_cut_units / deal_table, zafx_units.hpp; tests/host_emu/tile_units_emu.cpp compiled by g++)."""
import os
import subprocess

import numpy as np
import pytest

import zafx
from zafx import _lib

from conftest import ROOT

TILE = 32   # frames of one tile of k_imdct at W = 512, 1024, 2048
PER_SLOT = 4   # kImdctUnitsPerSlot: units per workgroup slot the segment length aims at


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: validation must come first."""
    def forbidden(*a, **k):
        raise AssertionError("the library was asked for a device before the input was validated")
    monkeypatch.setattr(_lib, "load", forbidden)


def test_imdct_ragged_is_exported_and_bound():
    assert callable(zafx.imdct_ragged) and callable(zafx.Plan.execute_imdct_ragged)
    assert "imdct_ragged" in zafx.__doc__
    res, args = _lib.SYMBOLS["zafx_execute_imdct_ragged"]
    assert len(args) == 7


KBD = zafx.kaiser_bessel_derived
BAD = [
    (5, "sequence of 2-D blocks"),                                                     # not a sequence
    (np.zeros((256, 10)), "sequence of 2-D blocks"),                                   # one block, not a batch
    ([np.zeros((256, 4)), np.zeros(256)], "block 1 .* must be 2-D"),                   # wrong rank
    ([np.zeros((256, 4)), np.zeros((256, 4)), np.zeros((2, 256, 4))], "block 2 .* must be 2-D"),
    ([np.zeros((256, 4)), np.zeros((256, 4), np.complex64)], "block 1 .* must be real"),
    ([np.array([["a"] * 3] * 256)], "block 0 .* must be real"),                        # not numeric
    ([np.zeros((256, 4)), np.zeros((255, 4))], "block 1 .* 256 coefficient rows"),     # row count != W / 2
    ([np.zeros((4, 256))], "block 0 .* 256 coefficient rows"),                         # a frame-major block in the reference layout
]


@pytest.mark.parametrize("blocks,msg", BAD)
def test_bad_batches_are_rejected_before_the_device(no_device, blocks, msg):
    for f64 in (False, True):
        with pytest.raises(ValueError, match=msg):
            zafx.imdct_ragged(blocks, KBD(512), f64=f64)


def test_frame_major_blocks_are_checked_along_their_own_axis(no_device):
    with pytest.raises(ValueError, match="block 1 .* 256 coefficient rows"):
        zafx.imdct_ragged([np.zeros((4, 256)), np.zeros((256, 4))], KBD(512), layout="TF")


def test_window_rules_are_those_of_imdct_batch(no_device):
    blocks = [np.zeros((256, 3))]
    with pytest.raises(ValueError, match="even window_length"):
        zafx.imdct_ragged(blocks, np.ones(511))
    with pytest.raises(ValueError, match="even window_length"):
        zafx.imdct_ragged([], np.ones(511))              # (the window is checked for an empty batch too)
    with pytest.raises(ValueError, match="even window_length"):
        zafx.imdct_ragged(blocks, np.ones(2))            # too short
    with pytest.raises(ValueError, match="2 ... 8192"):
        zafx.imdct_ragged(blocks, np.ones(8194))
    with pytest.raises(ValueError, match="1-D"):
        zafx.imdct_ragged(blocks, np.ones((2, 512)))
    with pytest.raises(ValueError, match="f64=True takes windows"):
        zafx.imdct_ragged(blocks, np.ones(4098), f64=True)


def test_lengths_are_checked_against_what_the_blocks_give(no_device):
    blocks = [np.zeros((256, 3)), np.zeros((256, 1))]    # 2 * 256 - 1 = 511 samples and none
    with pytest.raises(ValueError, match=r"lengths\[0\] = 512 exceeds the 511 samples"):
        zafx.imdct_ragged(blocks, KBD(512), lengths=[512, 0])
    with pytest.raises(ValueError, match=r"lengths\[1\] = 1 exceeds the 0 samples"):
        zafx.imdct_ragged(blocks, KBD(512), lengths=[511, 1])
    with pytest.raises(ValueError, match="one entry per block"):
        zafx.imdct_ragged(blocks, KBD(512), lengths=[5])
    with pytest.raises(ValueError, match="negative"):
        zafx.imdct_ragged(blocks, KBD(512), lengths=[5, -1])


def test_imdct_ragged_of_no_blocks_is_no_arrays(no_device):
    assert zafx.imdct_ragged([], KBD(2048)) == []
    assert zafx.imdct_ragged((), KBD(512), layout="TF", f64=True, lengths=[]) == []


# ------------------------------------------------------------------------------------------------------------------ the cutter and the deal
@pytest.fixture(scope="module")
def cutter(tmp_path_factory):
    exe = tmp_path_factory.mktemp("imdct_units") / "tile_units_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "tile_units_emu.cpp"), "-o", str(exe)], check=True)

    def run(frames, slots, grid=None):
        res = subprocess.run([str(exe), "imdct", str(TILE), str(slots), str(slots if grid is None else grid), "-"], input=" ".join(str(t) for t in frames),
                             capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-500:] + res.stderr[-500:]
        seg, grid_used, units, table = None, None, [], []
        for ln in res.stdout.split("\n"):
            if ln.startswith("S "):
                seg = int(ln[2:])
            elif ln.startswith("G "):
                grid_used = int(ln[2:])
            elif ln.startswith("U "):
                units.append(tuple(int(v) for v in ln[2:].split()))
            elif ln.startswith("D "):
                table.append(tuple(int(v) for v in ln[2:].split()))
        return seg, grid_used, units, table
    return run


def random_batches():
    rng = np.random.default_rng(7)
    yield "only empty outputs", [0, 1, 1, 0], 4
    yield "a single frame pair", [2], 1
    yield "three tiles against the floor of S", [3 * TILE] * 5, 512
    for k in range(24):
        n = int(rng.integers(1, 3001))
        hi = int(rng.choice([3, 70, 400, 4001]))
        frames = rng.integers(0, hi, n)
        if k % 3 == 0:
            frames[rng.integers(0, n)] = 4000
        yield f"random {k}", frames.tolist(), int(rng.integers(1, 513))


def test_cutter_and_deal_invariants(cutter):
    for what, frames, slots in random_batches():
        seg, grid, units, table = cutter(frames, slots)
        own = [0 if t <= 1 else -(-t // TILE) for t in frames]
        assert seg == max(3, -(-sum(own) // (PER_SLOT * slots))), what
        covered = [np.zeros(n, np.int32) for n in own]
        sizes, by_clip = [], {}
        for clip, a, b, tiles, t in units:
            assert t == frames[clip] and tiles == own[clip] and 0 <= a < b <= tiles, (what, clip, a, b)
            covered[clip][a:b] += 1
            whole = a == 0 and b == tiles
            assert whole == (tiles <= seg), (what, clip)               # a clip of at most S tiles is one unit, a longer one is cut
            assert whole or 2 <= b - a <= seg, (what, clip, a, b)      # no segment of a cut clip below two tiles or above S
            sizes.append(b - a)
            by_clip.setdefault(clip, []).append(b - a)
        for clip, c in enumerate(covered):                             # every tile of every clip in exactly one unit
            assert (c == 1).all(), (what, clip)
        assert set(by_clip) == {i for i, t in enumerate(frames) if t > 1}, what   # T <= 1: no unit
        assert all(max(s) - min(s) <= 1 for s in by_clip.values()), what          # near-equal segments
        assert sizes == sorted(sizes, reverse=True), what
        # the deal: the records with tiles are a permutation of the units; records without tiles only in the last round, in front
        assert grid == min(slots, len(units)), what
        real = [d for d in table if d[0] >= 0]
        assert sorted(real) == sorted(units), what
        holes = [i for i, d in enumerate(table) if d[0] < 0]
        if holes:
            rounds = len(table) // grid
            assert len(table) == rounds * grid and rounds % 2 == 0, what
            assert holes == list(range((rounds - 1) * grid, (rounds - 1) * grid + len(holes))), what
        else:
            assert len(table) == len(units), what
        # ... and fair.  Over a forward and a backward round two workgroups differ by at most the first minus the last size of the pair of
        # rounds, which telescopes to the longest unit over the whole descending table; a short last round adds one more unit at most.
        if units:
            load = np.zeros(grid, np.int64)
            for i, (clip, a, b, tiles, t) in enumerate(table):
                if clip >= 0:
                    load[i % grid] += b - a
            assert load.max() - load.min() <= 2 * max(sizes), (what, load.max(), load.min())


def test_the_measured_batch_gives_every_slot_its_units(cutter):
    """1024 blocks of clips of 5 - 15 s at W = 2048 on 256 slots: at least four units per slot."""
    frames = (-(-np.random.default_rng(0).integers(5 * 44100, 15 * 44100 + 1, 1024) // 1024) + 1).tolist()
    seg, grid, units, table = cutter(frames, 256)
    assert grid == 256 and seg >= 3
    assert len(units) >= 4 * 256
