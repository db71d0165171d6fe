"""The run-time tile queues of k_stft_ft16's DYN form on the host: the functions the kernel uses (zafx_fft.hpp), compiled by g++, hand every
tile out exactly once for tile counts and grid sizes around the edges (0, 1, 7, 255, 256, 257, 27 648 ...), and a Python model of the same
eight queues with stealing agrees."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.timeout(300)
def test_claim_functions_hand_every_tile_out_once(tmp_path):
    exe = tmp_path / "claim_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-DZAFX_HOST_EMU", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "claim_emu.cpp"), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr


def model(total, grid, order):
    """Eight queues over contiguous ranges (the first total % 8 one longer), one counter each; a workgroup draws from its XCD's queue
    (blockIdx & 7) and, once that is empty, from the next, round once.  `order(step, alive)` picks the workgroup that moves."""
    q, r = divmod(total, 8)
    length = [q + (x < r) for x in range(8)]
    first = [sum(length[:x]) for x in range(8)]
    counters = [0] * 8
    at = [b & 7 for b in range(grid)]
    done = [False] * grid
    handed = []
    step = 0
    while not all(done):
        alive = [b for b in range(grid) if not done[b]]
        b = order(step, alive)
        step += 1
        while True:
            v = counters[at[b]]
            counters[at[b]] += 1
            if v < length[at[b]]:
                handed.append(first[at[b]] + v)
                break
            at[b] = (at[b] + 1) & 7
            if at[b] == (b & 7):
                done[b] = True
                break
    return handed


@pytest.mark.parametrize("total", [0, 1, 7, 255, 256, 257, 27648])
@pytest.mark.parametrize("grid", [1, 7, 256, 257])
def test_model_of_eight_queues_with_stealing(total, grid):
    for order in (lambda s, alive: alive[0], lambda s, alive: alive[-1], lambda s, alive: alive[(s * 7919) % len(alive)]):
        assert sorted(model(total, grid, order)) == list(range(total))
