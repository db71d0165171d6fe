"""The owners of plan-owned memory (csrc/zafx_devbuf.hpp: DevBuf, PinnedBuf) over a counting allocator, no GPU: tests/host_emu/devbuf_emu.cpp is a
stand-alone program that asserts the contract -- upload frees the old block before it allocates, zero bytes and a failed allocation leave
the buffer null, reserve only grows, a moved-from buffer and a view free nothing, a destroyed struct of five buffers returns the count to
zero, the page-locked twin behaves the same.  Built with AddressSanitizer and UBSan where g++ can link them (a double free, a leak or a read
of a freed block ends the program), else without."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host_emu", "devbuf_emu.cpp")
BASE = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-DZAFX_HOST_EMU", "-I", os.path.join(ROOT, "zaf-python_amd", "csrc"), SRC]


def test_devbuf_contract_under_a_counting_allocator(tmp_path):
    exe = str(tmp_path / "devbuf_emu.bin")
    # (the runtimes linked statically: the program then runs whatever else the loader brings in first)
    sanitized = subprocess.run(BASE + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe],
                               capture_output=True, text=True)
    if sanitized.returncode != 0:   # (no sanitizer runtime to link on this machine: the assertions alone)
        print("built without sanitizers:", sanitized.stderr[-500:])
        subprocess.run(BASE + ["-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
