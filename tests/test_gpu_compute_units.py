"""Every persistent kernel on grids other than the MI355X's 256 compute units (-m gpu; the child process is tests/cu_probe.py).

Almost every launcher sizes its grid, its cut of the clips into carry segments or the slot count of a ragged launch from the plan's compute
units, and every other GPU test runs them at 256: small batches then get one tile per workgroup (the walk from tile to tile, the step from
a clip's partial last tile into the next clip's first, LDS reuse and prefetch never run), one-tile units with a carry-only entry in the
carry kernels, and ragged segments at their floor of three tiles.  ZAFX_COMPUTE_UNITS (include/zafx.h) caps the count a plan sees; here
every route runs uncapped and at caps of 32, 3 and 1 on 77 tiles (7 clips of ten whole tiles and a partial one; ragged: 9 clips of 0 ... 21
tiles), which is no multiple of any of these grids: at 32 some workgroups walk more tiles than others, at 3 and 1 every workgroup walks more
than ten, and at 1 the carry kernels take whole clips (carry_segments == 1, asserted on the host function) and the ragged cutters leave
their floor (asserted on the host cutters).

Per route and cap: (1) the plan reports min(cap, device) compute units; (2) the kernel is the one the table names, capped or not; (3) every
clip is the float64 oracle's within the suite's bounds (1e-5 STFT / MDCT family and DCT, 1e-4 mel / mfcc / CQT, 1e-12 float64), shapes exact;
(4) the output buffer is bit-identical to the uncapped plan's -- pad columns, the gaps between ragged clips and everything else the NaN fill
left included (a result does not depend on who computes a tile or where a segment starts); (5) a second launch
of the same plan gives the same bits (the claimed-tile form of k_stft_ft16: its counters came back to zero on a grid below its eight queues).

Measured on MI355X, 2026-10-19: 49 tests in 43 s, the slowest child (stft_ft16q) 2.1 s of wall time, none above 2 % of its limit.

One child per route, one after another, each under a time limit; a child that dies of anything but a Python error ends the module:
nothing more is launched."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CAPS = (None, 32, 3, 1)
OTHER_FORM = 2e-6   # two forms of one kernel on the same frames (tests/test_gpu_parity.py _run_padded): the bound of a route listed in CUT_DEPENDENT

# route of tests/cu_probe.py -> the kernel it must run at every cap (read off the launchers, as tests/test_gpu_windows.py and tests/test_gpu_arena.py do)
ROUTES = {
    "stft_ft16_claimed": "k_stft_ft16", "stft_ft16_static": "k_stft_ft16", "stft_ft16c": "k_stft_ft16c", "stft_ft16b": "k_stft_ft16b",
    "stft_ft16bc": "k_stft_ft16bc", "stft_ft16q": "k_stft_ft16q", "stft_tf": "k_stft_tf",
    "mel_ft16b": "k_mel_ft16b", "mel2_mel": "k_mel2", "mel2_mfcc": "k_mel2", "mel2_both": "k_mel2", "mel": "k_mel", "melfb": "k_melfb",
    "istft_ft16": "k_istft_ft16", "istft_ft16b": "k_istft_ft16b", "istft_ft16d": "k_istft_ft16d", "istft_ft8q": "k_istft_ft8q",
    "mdct_ft32_plain": "k_mdct_ft32", "mdct_ft32_carry": "k_mdct_ft32", "mdct_ft32b": "k_mdct_ft32b", "mdct_ft32bc": "k_mdct_ft32bc",
    "mdct_ft32q": "k_mdct_ft32q", "imdct": "k_imdct", "imdct_q": "k_imdct_q",
    "center": "k_center", "center_sides": "k_center",
    "cqt_tiny": "k_cqt", "cqt_8192": "k_cqt", "chroma_8192": "k_cqt", "cqt_split": "k_cqt",
    "dct": "k_dct", "dct_bsh": "k_dct_bsh", "dct_bs32": "k_dct_bs32",
    "stft_ragged": "k_stft_ft16_ragged", "mel2_ragged": "k_mel2_ragged", "mdct_ragged": "k_mdct_ft32_ragged",
    "imdct_ragged": "k_imdct_ragged", "istft_ragged": "k_istft_ragged", "center_ragged": "k_center_ragged",
    "stft_f64": "k_stft_ft8_f64", "mdct_f64": "k_mdct_ft16_f64", "mel_f64": "k_mel_ft8_f64", "istft_f64": "k_istft_ft8_f64",
    "imdct_f64": "k_imdct_ft16_f64", "cqt_f64": "k_cqt_ft_f64",
    "stft_f64_ragged": "k_stft_ft8_f64_ragged", "mdct_f64_ragged": "k_mdct_ft16_f64_ragged", "mel_f64_ragged": "k_mel_ft8_f64_ragged",
}
KERNELS = {
    "k_stft_ft16", "k_stft_ft16c", "k_stft_ft16b", "k_stft_ft16bc", "k_stft_ft16q", "k_stft_tf", "k_mel_ft16b", "k_mel2", "k_mel", "k_melfb",
    "k_istft_ft16", "k_istft_ft16b", "k_istft_ft16d", "k_istft_ft8q", "k_mdct_ft32", "k_mdct_ft32b", "k_mdct_ft32bc", "k_mdct_ft32q", "k_imdct",
    "k_imdct_q", "k_center", "k_cqt", "k_dct", "k_dct_bsh", "k_dct_bs32", "k_stft_ft16_ragged", "k_mel2_ragged", "k_mdct_ft32_ragged",
    "k_imdct_ragged", "k_istft_ragged", "k_center_ragged", "k_stft_ft8_f64", "k_mdct_ft16_f64", "k_mel_ft8_f64", "k_istft_ft8_f64",
    "k_imdct_ft16_f64", "k_cqt_ft_f64", "k_stft_ft8_f64_ragged", "k_mdct_ft16_f64_ragged", "k_mel_ft8_f64_ragged",
}
# Routes whose summation order legitimately depends on the cut: route -> the reason, from the kernel's code.  They are held to OTHER_FORM against
# the uncapped launch instead of to its bits.  None is: the one route that differed when this module first ran, istft_f64 (k_istft_ft8_f64: 18 366 /
# 20 705 / 26 103 of 609 280 samples at caps 32 / 3 / 1, 2.3e-16 normwise), formed a segment's left neighbour in a second copy of its arithmetic that
# the compiler contracted into other fused multiply-adds -- a bug, fixed in the kernel.
CUT_DEPENDENT = {}

CQT_ROUTES = {"cqt_tiny", "cqt_8192", "chroma_8192", "cqt_split", "cqt_f64"}   # the child builds a kernel matrix on the host first
RAGGED_FLOOR = {"imdct_ragged": 3, "istft_ragged": 3, "center_ragged": 29}    # kImdctMinSegment, kIstftMinSegment, 4 F - 3 at F = 8 (zafx_units.hpp)

_seen = {}      # route -> the kernels its caps reported
_died = []      # the child that ended on a signal or ran out of time: nothing is launched behind it


def limit(route):
    return 300 if route in CQT_ROUTES else 120


def build(directory, name):
    exe = os.path.join(str(directory), name)
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", name + ".cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def emus(tmp_path_factory):
    """The host functions the launchers cut a batch with, as g++ compiles them."""
    d = tmp_path_factory.mktemp("cu_emus")
    return {name: build(d, name) for name in ("carry_segments_emu", "tile_units_emu", "center_units_emu")}


def host_line(cmd, tag):
    res = subprocess.run([str(c) for c in cmd], capture_output=True, text=True, check=True)
    for ln in res.stdout.splitlines():
        if ln.startswith(tag):
            return [int(v) for v in ln[len(tag):].split()]
    raise AssertionError((cmd, res.stdout[:300]))


def run_child(route):
    """-> (the child's JSON lines, its return code or None when it ran out of time, the end of its stderr)."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "cu_probe.py"), route]
    try:
        res = subprocess.run(cmd, capture_output=True, timeout=limit(route))
        out, err, rc = res.stdout, res.stderr, res.returncode
    except subprocess.TimeoutExpired as exc:
        out, err, rc = exc.stdout or b"", exc.stderr or b"", None
    lines = []
    for ln in out.decode(errors="replace").splitlines():
        if ln.startswith("{"):
            lines.append(json.loads(ln))
    return lines, rc, err.decode(errors="replace")[-2000:]


def check_lines(route, lines, emus):
    """The assertions on one child's report."""
    ready = [ln for ln in lines if ln["stage"] == "ready"]
    done = [ln for ln in lines if ln["stage"] == "done"]
    assert len(ready) == 1 and [ln["cap"] for ln in done] == list(CAPS), (route, lines[-3:])
    assert lines[-1]["stage"] == "end" and lines[-1]["secs"] <= limit(route) / 2, (route, lines[-1])   # (more than half the limit: smaller inputs, not a longer limit)
    info, want = ready[0]["info"], ROUTES[route]
    assert ready[0]["kernel_expected"] == want
    # the shapes make the caps bite
    if "tiles_per_clip" in info:
        assert info["tiles"] == 77 and info["tiles_per_clip"] == 11, info
    if "carry" in info:   # whole clips per unit at a cap of 1, at one and at two workgroups per compute unit
        for grid in (1, 2):
            assert host_line([emus["carry_segments_emu"], grid, "="] + info["carry"], "")[2] == 1, (route, grid, info)
        assert host_line([emus["carry_segments_emu"], 256, "="] + info["carry"], "")[2] > 1, (route, info)   # (and cut on the whole device)
    if "clip_tiles" in info:
        assert info["clip_tiles"][1:] == [1, 2, 3, 5, 8, 11, 13, 21] and info["clip_tiles"][0] in (0, 1), info
    if route in ("imdct_ragged", "istft_ragged"):   # (slots at a cap of 1: one or two workgroups per compute unit; two gives the shorter segments)
        head = ["imdct", 32] if route == "imdct_ragged" else ["istft", 2048, 1024, 16]
        assert host_line([emus["tile_units_emu"]] + head + [2, 2] + info["frames"], "S ")[0] > RAGGED_FLOOR[route], (route, info)
        assert host_line([emus["tile_units_emu"]] + head + [512, 512] + info["frames"], "S ")[0] == RAGGED_FLOOR[route], (route, info)
    if route == "center_ragged":   # (at most four workgroups per compute unit)
        head = [emus["center_units_emu"], info["window"], info["tile_frames"]]
        assert host_line(head + [4] + info["lengths"], "S ")[0] > RAGGED_FLOOR[route], info
        assert host_line(head + [1024] + info["lengths"], "S ")[0] == RAGGED_FLOOR[route], info
    # the caps
    device = done[0]["device_compute_units"]
    for ln in done:
        cap = ln["cap"]
        print(f"{route} cap {cap}: {ln['compute_units']} of {ln['device_compute_units']} CUs, {ln['kernel']}, worst {ln['worst']:.3e}, "
              f"bits {'same' if ln['same_as_uncapped'] else 'DIFFER'}, {ln['secs']} s")
        assert ln["device_compute_units"] == device and ln["compute_units"] == (device if cap is None else min(cap, device)), (route, ln)   # (1)
        assert ln["kernel"] == want == done[0]["kernel"], (route, ln)                                                                       # (2)
        assert ln["shapes_ok"] and ln["clips"] == ln["refs"] and ln["written"] and ln["outside_untouched"], (route, ln)                     # (3)
        assert ln["worst"] <= ln["tol"], (route, ln)
        if route in CUT_DEPENDENT:                                                                                                          # (4)
            assert ln["same_as_uncapped"] or (ln["nan_mismatch"] == 0 and ln["normwise_to_uncapped"] <= OTHER_FORM), (route, ln)
        else:
            assert ln["same_as_uncapped"], (route, ln)
        assert ln["repeat_same"], (route, ln)                                                                                               # (5)
    return {ln["kernel"] for ln in done}


def _route_params():
    return [pytest.param(route, marks=pytest.mark.timeout(limit(route) + 60)) for route in ROUTES]


@pytest.mark.parametrize("route", _route_params())
def test_route_under_caps(route, emus):
    if _died:
        pytest.fail(f"not run: the child of route {_died[0]} died; nothing more is launched")
    lines, rc, err = run_child(route)
    if rc is None or rc < 0 or rc in (134, 139):
        _died.append(route)
    report = os.environ.get("ZAFX_CU_REPORT")   # a directory: every child's lines are kept there, whatever the assertions say
    if report:
        with open(os.path.join(report, route + ".jsonl"), "w") as f:
            f.write("".join(json.dumps(ln) + "\n" for ln in lines) + f"rc {rc}\n{err}\n")
    assert rc == 0, (route, "out of time" if rc is None else rc, [ln for ln in lines if ln["stage"] != "ready"][-3:], err)
    _seen[route] = check_lines(route, lines, emus)


def test_every_kernel_of_the_table_was_reported_by_name():
    """A route that fell back to another kernel without saying so fails its own test; this one holds the table itself: every launcher that
    takes the cap has a route, and the names the children reported are exactly the table's."""
    assert set(ROUTES.values()) == KERNELS
    if len(_seen) < len(ROUTES):
        pytest.fail(f"routes without a report (run the whole module): {sorted(set(ROUTES) - set(_seen))}")
    assert set().union(*_seen.values()) == KERNELS
