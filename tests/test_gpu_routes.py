"""Every route of the float32 launchers on a call of a few frames (-m gpu): the calls of tests/route_cases.py launch the kernel and write the
bytes recorded in tests/golden/call_routes.json (tests/golden/make_route_golden.py, run twice on the commit before the route decisions moved
into zaf-python_amd/csrc/zafx_routes.hpp: the two recordings agreed on every case), and the header compiled for the host
(tests/host_emu/routes_emu.cpp) names the same kernel for the same call -- which ties the rule tests/test_routes_host.py checks on the CPU to
what ran."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN
import route_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    return z


@pytest.fixture(scope="module")
def routes():
    with open(os.path.join(GOLDEN, "call_routes.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def emu_kernels(tmp_path_factory):
    """The kernel routes_emu names for every case."""
    exe = tmp_path_factory.mktemp("routes") / "routes_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_emu", "routes_emu.cpp"), "-o", str(exe)], check=True)
    names = list(rc.CASES)
    res = subprocess.run([str(exe)], input="\n".join(rc.call_line(rc.CASES[n]) for n in names) + "\n", capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert len(lines) == len(names)
    return {n: dict(f.split("=") for f in ln.split())["kernel"] for n, ln in zip(names, lines)}


def test_the_recorded_routes_are_the_cases(routes):
    assert list(routes) == list(rc.CASES)
    assert all(len(r) == 2 and r[0] and r[1] and (r[0] == "refused" or len(r[1]) == 64) for r in routes.values())


@pytest.mark.parametrize("name", list(rc.CASES))
def test_call_runs_the_recorded_kernel_and_writes_the_recorded_bytes(zafx, routes, emu_kernels, name):
    got = rc.record(name)
    print(name, got, emu_kernels[name])
    assert got == routes[name]
    assert emu_kernels[name] == got[0]
