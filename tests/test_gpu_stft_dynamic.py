"""k_stft_ft16 with its tiles claimed at run time (the DYN form, the default route where every store of a tile is a whole line, and for
ragged batches) against the static split (ZAFX_STFT_DYNAMIC=0 at plan creation): bit-identical outputs, launch after launch of one plan
(the last workgroup of a launch puts the plan's counters back to zero), for tile counts below the grid and off the multiples of eight.

Every case runs in a child process of its own under a time limit: a workgroup that never leaves ends the test, not the card."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# tiles of the equal-length cases: 27 per clip of 432 frames, 28 per clip of 433
CASES = {"headline": 64 * 27, "padded433": 64 * 28, "few": 3 * 27, "odd": 21 * 27, "ragged": None}


@pytest.mark.timeout(400)
@pytest.mark.parametrize("case", list(CASES))
def test_claimed_tiles_equal_static_split(case):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dyn_probe.py"), case], capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    r = json.loads(res.stdout.decode().strip().splitlines()[-1])
    want = "k_stft_ft16_ragged" if case == "ragged" else "k_stft_ft16"
    assert r["kernels"] == {"static": want, "claimed": want}, r
    if CASES[case] is not None:
        assert r["tiles"] == CASES[case], r
        assert r["pitch"] % 16 == 0, r   # whole-line rows: the route that claims its tiles
    if case == "few":
        assert r["tiles"] < 256
    if case == "odd":
        assert r["tiles"] % 8 != 0
    assert r["written"] and r["static_repeatable"], r
    assert r["claimed_equal"] == [True, True, True], r   # the first launch, and two more of the same plan
