"""Ragged batches of the inverse STFT on the host side (no GPU): the export and the binding of the new entry point, the validation that runs
before any device call, the empty batch, and the cutter and the deal that turn a batch of spectra into the table k_istft_ft16's RAGGED form
walks (istft_cut_units / deal_table, zafx_units.hpp; tests/host_emu/tile_units_emu.cpp compiled by g++ -- once more under AddressSanitizer and UBSan as a plain program)."""
import os
import subprocess

import numpy as np
import pytest

import zafx
from zafx import _lib

from conftest import ROOT
from oracle import zaf_oracle as orc

TILE = 16      # frames of one tile of k_istft_ft16
PER_SLOT = 4   # kIstftUnitsPerSlot: units per workgroup slot the segment length aims at


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test: validation must come first."""
    def forbidden(*a, **k):
        raise AssertionError("the library was asked for a device before the input was validated")
    monkeypatch.setattr(_lib, "load", forbidden)


def test_istft_ragged_is_exported_and_bound():
    assert callable(zafx.istft_ragged) and callable(zafx.Plan.execute_istft_ragged)
    assert "istft_ragged" in zafx.__doc__
    res, args = _lib.SYMBOLS["zafx_execute_istft_ragged"]
    assert len(args) == 7


HAM = zafx.hamming
C64 = np.complex64
BAD = [
    (5, "sequence of 2-D blocks"),                                                          # not a sequence
    (np.zeros((512, 10), C64), "sequence of 2-D blocks"),                                   # one block, not a batch
    ([np.zeros((512, 4), C64), np.zeros(512, C64)], "block 1 .* must be 2-D"),              # wrong rank
    ([np.zeros((512, 4), C64), np.zeros((512, 4)), np.zeros((2, 512, 4), C64)], "block 2 .* must be 2-D"),
    ([np.array([["a"] * 3] * 512)], "block 0 .* must be numeric"),                          # not numeric
    ([np.zeros((512, 4), C64), np.zeros((511, 4), C64)], "block 1 .* window_length = 512 spectrum rows"),
    ([np.zeros((257, 4), C64)], "block 0 .* window_length = 512 spectrum rows"),            # a one-sided block in a two-sided call
    ([np.zeros((4, 512), C64)], "block 0 .* window_length = 512 spectrum rows"),            # a frame-major block in the reference layout
]


@pytest.mark.parametrize("blocks,msg", BAD)
def test_bad_batches_are_rejected_before_the_device(no_device, blocks, msg):
    for f64 in (False, True):
        with pytest.raises(ValueError, match=msg):
            zafx.istft_ragged(blocks, HAM(512), 256, f64=f64)


def test_onesided_blocks_have_half_the_rows_plus_one(no_device):
    with pytest.raises(ValueError, match=r"block 1 .* window_length/2 \+ 1 = 257 spectrum rows"):
        zafx.istft_ragged([np.zeros((257, 4), C64), np.zeros((512, 4), C64)], HAM(512), 256, onesided=True)


def test_frame_major_blocks_are_checked_along_their_own_axis(no_device):
    with pytest.raises(ValueError, match="block 1 .* window_length = 512 spectrum rows"):
        zafx.istft_ragged([np.zeros((4, 512), C64), np.zeros((512, 4), C64)], HAM(512), 256, layout="TF")
    with pytest.raises(ValueError, match="block 0 .* 257 spectrum rows"):
        zafx.istft_ragged([np.zeros((257, 4), C64)], HAM(512), 256, layout="TF", onesided=True)


def test_window_and_step_rules_are_those_of_istft_batch(no_device):
    blocks = [np.zeros((512, 3), C64)]
    with pytest.raises(ValueError, match="must not exceed window_length"):
        zafx.istft_ragged(blocks, HAM(512), 513)
    with pytest.raises(ValueError, match="must not exceed window_length"):
        zafx.istft_ragged([], HAM(512), 513)              # (window and step are checked for an empty batch too)
    with pytest.raises(ValueError, match="onesided must be False or True"):
        zafx.istft_ragged(blocks, HAM(512), 256, onesided="magnitude")
    with pytest.raises(ValueError, match="1-D"):
        zafx.istft_ragged(blocks, np.ones((2, 512)), 256)
    with pytest.raises(ValueError, match="f64=True takes windows"):
        zafx.istft_ragged(blocks, np.ones(4098), 2049, f64=True)
    with pytest.raises(ValueError):
        zafx.istft_ragged(blocks, HAM(512), 0)
    with pytest.raises((ValueError, KeyError)):
        zafx.istft_ragged(blocks, HAM(512), 256, layout="XY")


def test_lengths_are_checked_against_what_the_blocks_give(no_device):
    blocks = [np.zeros((512, 3), C64), np.zeros((512, 1), C64)]    # 3 * 256 - 256 = 512 samples and none
    with pytest.raises(ValueError, match=r"lengths\[0\] = 513 exceeds the 512 samples"):
        zafx.istft_ragged(blocks, HAM(512), 256, lengths=[513, 0])
    with pytest.raises(ValueError, match=r"lengths\[1\] = 1 exceeds the 0 samples"):
        zafx.istft_ragged(blocks, HAM(512), 256, lengths=[512, 1])
    with pytest.raises(ValueError, match="one entry per block"):
        zafx.istft_ragged(blocks, HAM(512), 256, lengths=[5])
    with pytest.raises(ValueError, match="negative"):
        zafx.istft_ragged(blocks, HAM(512), 256, lengths=[5, -1])


def test_istft_ragged_of_no_blocks_is_no_arrays(no_device):
    assert zafx.istft_ragged([], HAM(2048), 1024) == []
    assert zafx.istft_ragged((), HAM(512), 128, layout="TF", onesided=True, f64=True, lengths=[]) == []


def test_imdct_ragged_still_rejects_complex_blocks(no_device):
    with pytest.raises(ValueError, match="block 1 .* must be real"):
        zafx.imdct_ragged([np.zeros((256, 4)), np.zeros((256, 4), C64)], zafx.kaiser_bessel_derived(512))
    with pytest.raises(ValueError, match="clip 0 .* must be real"):
        zafx.stft_ragged([np.zeros(100, C64)], HAM(512), 256)


# ------------------------------------------------------------------------------------------------------------------ the cutter and the deal
EMU = os.path.join(ROOT, "tests", "host_emu", "tile_units_emu.cpp")
INC = os.path.join(ROOT, "zaf-python_amd", "csrc")


def parse(stdout):
    seg, grid, lens, units, table = None, None, [], [], []
    for ln in stdout.split("\n"):
        if ln.startswith("S "):
            seg = int(ln[2:])
        elif ln.startswith("G "):
            grid = int(ln[2:])
        elif ln.startswith("L "):
            lens.append(int(ln[2:].split()[1]))
        elif ln.startswith("U "):
            units.append(tuple(int(v) for v in ln[2:].split()))
        elif ln.startswith("D "):
            table.append(tuple(int(v) for v in ln[2:].split()))
    return seg, grid, lens, units, table


@pytest.fixture(scope="module")
def cutter(tmp_path_factory):
    exe = tmp_path_factory.mktemp("istft_units") / "tile_units_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", INC, EMU, "-o", str(exe)], check=True)

    def run(frames, slots, w=2048, h=1024, grid=None):
        res = subprocess.run([str(exe), "istft", str(w), str(h), str(TILE), str(slots), str(slots if grid is None else grid), "-"],
                             input=" ".join(str(t) for t in frames), capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-500:] + res.stderr[-500:]
        return parse(res.stdout)
    return run


def random_batches():
    rng = np.random.default_rng(11)
    yield "only empty outputs", [0, 1, 1, 0], 4
    yield "a single frame pair", [2], 1
    yield "three tiles against the floor of S", [3 * TILE] * 5, 512
    yield "41 tiles each", [41 * TILE] * 3, 256
    for k in range(24):
        n = int(rng.integers(1, 3001))
        hi = int(rng.choice([3, 40, 200, 2001]))
        frames = rng.integers(0, hi, n)
        if k % 3 == 0:
            frames[rng.integers(0, n)] = 2000
        yield f"random {k}", frames.tolist(), int(rng.integers(1, 513))


def check_batch(what, frames, slots, w, h, result):
    seg, grid, lens, units, table = result
    out = [max(t * h - (w - h), 0) for t in frames]
    assert lens == out, what
    own = [-(-t // TILE) if o > 0 else 0 for t, o in zip(frames, out)]
    assert seg == max(3, -(-sum(own) // (PER_SLOT * slots))), what
    covered = [np.zeros(n, np.int32) for n in own]
    sizes, by_clip = [], {}
    for clip, a, b, tiles, t, out_len, tp in units:
        assert t == frames[clip] and tiles == own[clip] and 0 <= a < b <= tiles, (what, clip, a, b)
        assert out_len == out[clip] and tp == -(-t // 16) * 16, (what, clip)
        covered[clip][a:b] += 1
        whole = a == 0 and b == tiles
        assert whole == (tiles <= seg), (what, clip)               # a clip of at most S tiles is one unit, a longer one is cut
        assert whole or 2 <= b - a <= seg, (what, clip, a, b)      # no segment of a cut clip below two tiles or above S
        sizes.append(b - a)
        by_clip.setdefault(clip, []).append(b - a)
    for clip, c in enumerate(covered):                             # every tile of every clip in exactly one unit
        assert (c == 1).all(), (what, clip)
    assert set(by_clip) == {i for i, o in enumerate(out) if o > 0}, what      # no samples: no unit
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
    if units:   # ... and fair (the bound of test_imdct_ragged_host.py: the longest unit over a pair of rounds, one more for a short last round)
        load = np.zeros(grid, np.int64)
        for i, d in enumerate(table):
            if d[0] >= 0:
                load[i % grid] += d[2] - d[1]
        assert load.max() - load.min() <= 2 * max(sizes), (what, load.max(), load.min())


def test_cutter_and_deal_invariants(cutter):
    for k, (what, frames, slots) in enumerate(random_batches()):
        w, h = [(2048, 1024), (512, 128), (1024, 768), (256, 129)][k % 4]
        check_batch(what, frames, slots, w, h, cutter(frames, slots, w, h))


def test_spectra_without_output_give_no_unit(cutter):
    seg, grid, lens, units, table = cutter([1, 40, 1], 8, 512, 256)               # hop W/2: one frame gives nothing
    assert lens == [0, 40 * 256 - 256, 0] and {u[0] for u in units} == {1}
    seg, grid, lens, units, table = cutter([1, 2, 3, 4, 0], 8, 512, 128)          # hop W/4: up to three frames give nothing
    assert lens == [0, 0, 0, 128, 0] and [u[:5] for u in units] == [(3, 0, 1, 1, 4)] and table == units
    seg, grid, lens, units, table = cutter([1, 2, 3, 1], 8, 512, 128)
    assert units == [] and table == [] and grid == 0


def test_out_len_is_the_oracles(cutter):
    w = 64
    win = np.hamming(w)
    for h in (w // 4, w // 2, w // 2 + 1, 3 * w // 4, w):
        frames = list(range(1, 41))
        lens = cutter(frames, 4, w, h)[2]
        for t, n in zip(frames, lens):
            assert n == len(orc.istft(np.zeros((w, t), np.complex128), win, h)), (h, t)


def test_the_measured_batch_gives_every_slot_its_units(cutter):
    """1024 spectra of clips of 5 - 15 s at W = 2048, hop 1024, on 256 slots: at least four units per slot."""
    frames = (-(-np.random.default_rng(0).integers(5 * 44100, 15 * 44100 + 1, 1024) // 1024) + 1).tolist()
    seg, grid, lens, units, table = cutter(frames, 256)
    assert grid == 256 and seg >= 3
    assert len(units) >= 4 * 256


def test_cutter_under_the_sanitizers(tmp_path):
    """The same program built with AddressSanitizer and UBSan, run as it is (a plain host program)."""
    exe = tmp_path / "tile_units_emu_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", INC, EMU, "-o", str(exe)],
                   check=True)
    for k, (what, frames, slots) in enumerate(random_batches()):
        if k % 4 and k > 4:
            continue
        w, h = [(2048, 1024), (512, 128), (1024, 768), (256, 129)][k % 4]
        res = subprocess.run([str(exe), "istft", str(w), str(h), str(TILE), str(slots), str(slots), "-"], input=" ".join(str(t) for t in frames),
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and "ERROR" not in res.stderr and "runtime error" not in res.stderr, (what, res.stderr[-800:])
        check_batch(what, frames, slots, w, h, parse(res.stdout))
