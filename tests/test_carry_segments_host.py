"""carry_segments (zafx_units.hpp; no GPU): the number of segments the carry kernels of an equal-length batch cut every clip's tiles into --
k_stft_ft16c, k_istft_ft16 and its band forms, k_imdct, k_imdct_q, the carry forms of k_mdct_ft32 and the float64 inverses.  The function as
g++ compiles it (tests/host_emu/carry_segments_emu.cpp) against its own rule restated here: over grids from one workgroup to twice the
MI355X's compute units, 1 ... 40 clips of 1 ... 64 tiles."""
import math
import os
import subprocess

import pytest

from conftest import ROOT

GRIDS = (1, 2, 3, 6, 32, 64, 256, 512)
MAX_CLIPS, MAX_TILES = 40, 64


def build_emu(directory):
    exe = os.path.join(str(directory), "carry_segments_emu")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "carry_segments_emu.cpp"), "-o", exe], check=True)
    return exe


def carry_segments(exe, n_clips, tiles, grid):
    res = subprocess.run([exe, str(grid), "=", str(n_clips), str(tiles)], capture_output=True, text=True, check=True)
    return int(res.stdout.split()[2])


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{grid: {(n_clips, tiles): segs}} as the library's function gives it."""
    exe = build_emu(tmp_path_factory.mktemp("carry_segments"))
    out = {}
    for grid in GRIDS:
        res = subprocess.run([exe, str(grid), str(MAX_CLIPS), str(MAX_TILES)], capture_output=True, text=True, check=True)
        rows = [tuple(int(v) for v in ln.split()) for ln in res.stdout.splitlines()]
        assert len(rows) == MAX_CLIPS * MAX_TILES
        out[grid] = {(n, t): s for n, t, s in rows}
    return out


def admissible(tiles, segs):
    """No empty segment: the last of `segs` segments of ceil(tiles / segs) tiles still has one."""
    return segs == 1 or (segs - 1) * -(-tiles // segs) < tiles


def cost(n_clips, tiles, segs, grid):
    """What the function minimises: rounds of the grid times the tiles of a segment, a carry-only entry counted as half a tile."""
    return -(-n_clips * segs // grid) * (-(-tiles // segs) + (0.5 if segs > 1 else 0.0))


@pytest.mark.parametrize("grid", GRIDS)
def test_segments_are_in_range_and_none_is_empty(table, grid):
    for (n, t), segs in table[grid].items():
        assert 1 <= segs <= t, (grid, n, t, segs)
        assert (segs - 1) * math.ceil(t / segs) < t, (grid, n, t, segs)


@pytest.mark.parametrize("grid", GRIDS)
def test_whole_clips_when_the_clips_fill_the_grid_in_whole_rounds(table, grid):
    seen = 0
    for (n, t), segs in table[grid].items():
        if n >= grid and n % grid == 0:
            assert segs == 1, (grid, n, t, segs)
            seen += 1
    assert seen or grid > MAX_CLIPS


@pytest.mark.parametrize("grid", GRIDS)
def test_no_other_admissible_cut_is_cheaper(table, grid):
    for (n, t), segs in table[grid].items():
        best = min(cost(n, t, s, grid) for s in range(1, t + 1) if admissible(t, s))
        assert cost(n, t, segs, grid) <= best + 1e-9, (grid, n, t, segs, cost(n, t, segs, grid), best)


def test_the_cases_the_gpu_tests_lean_on(table):
    """3 clips x 5 tiles on 256 workgroups: one-tile units (what the small shapes of the contract suites run); 7 clips x 11 tiles on one workgroup:
    whole clips (tests/test_gpu_compute_units.py at a cap of 1)."""
    assert table[256][(3, 5)] == 5
    assert table[1][(7, 11)] == 1
    assert table[2][(7, 11)] == 1   # (two workgroups per compute unit: 4 rounds of 11 tiles against 7 rounds of 6.5)
    assert table[3][(7, 11)] == 3   # 7 rounds of 4.5 tiles against 3 rounds of 11: whole clips are not a given below the cap of 1
