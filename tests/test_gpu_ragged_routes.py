"""Every branch of the ragged entry points on a batch of three clips of at most 33 frames (-m gpu): the batches of
tests/ragged_route_cases.py launch the kernel and write the bytes recorded in tests/golden/ragged_routes.json
(tests/golden/make_ragged_route_golden.py, run twice with the library of the commit before the ragged routing moved into
zaf-python_amd/csrc/zafx_routes.hpp: the two recordings agreed on every case), and the header compiled for the host
(tests/host_emu/routes_emu.cpp) names the same kernel for the same batch -- which ties the rule tests/test_routes_host.py checks on the CPU
to what ran.  The output hash is the only witness on the GPU of the `aligned` flag and of which path an integer batch took: neither shows
in the kernel's name.  A case recorded without a hash (its two recordings differed) is held to its name and flags alone."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN
import ragged_route_cases as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    return z


@pytest.fixture(scope="module")
def routes():
    with open(os.path.join(GOLDEN, "ragged_routes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def emu_kernels(tmp_path_factory):
    """The kernel routes_emu names for every case: the RAGGED form's, or `per-clip`.  An integer batch its one launch does not take is asked
    again as the float batch it becomes on the plan's staging array."""
    exe = tmp_path_factory.mktemp("routes") / "routes_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "routes_emu.cpp"), "-o", str(exe)], check=True)

    def ask(names, **kw):
        res = subprocess.run([str(exe)], input="\n".join(rr.call_line(rr.CASES[n], **kw) for n in names) + "\n", capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr[-2000:]
        lines = res.stdout.strip().split("\n")
        assert len(lines) == len(names)
        return {n: dict(f.split("=") for f in ln.split())["kernel"] for n, ln in zip(names, lines)}

    kernels = ask(list(rr.CASES))
    kernels.update(ask([n for n, k in kernels.items() if k == "none"], as_float=True))
    return kernels


def test_the_recorded_routes_are_the_cases(routes):
    assert list(routes) == list(rr.CASES)
    # the recorder's format: a hash of 64 hex digits, null for a case whose two recordings differed, the message for a refused call
    assert all(len(r) == 4 and r[0] and (r[1] is None or r[0] == "refused" or len(r[1]) == 64) for r in routes.values())


@pytest.mark.parametrize("name", list(rr.CASES))
def test_batch_runs_the_recorded_kernel_and_writes_the_recorded_bytes(zafx, routes, emu_kernels, name):
    got, want = rr.record(name), routes[name]
    print(name, got, emu_kernels[name])
    if want[1] is None:   # not reproducible when it was recorded: held to its name and flags alone
        got[1] = None
    assert got == want
    if want[0] == "refused":
        return
    if emu_kernels[name] == "per-clip":
        assert got[0].startswith("per-clip ") or (rr.is_inverse(rr.CASES[name]) and not got[0].endswith("_ragged"))
    else:
        assert emu_kernels[name] == got[0]
