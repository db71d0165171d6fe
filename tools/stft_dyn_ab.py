#!/usr/bin/env python3
"""k_stft_ft16: tiles claimed at run time against the static split, in ONE process, from one input into ONE output buffer.

    python tools/stft_dyn_ab.py [--rounds 10] [--launches 20] [--out FILE]

Headline geometry (1024 clips x 10 s, W = 2048, hop 1024, two-sided, (W, T) layout).  Three plans: static A, static B
(ZAFX_STFT_DYNAMIC=0 at their creation) and claimed.  After about 240 untimed launches (the clocks of an idle device ramp), every round times
`--launches` launches of each plan, one HIP-event reading per launch, in the order A, claimed, B, and keeps the medians.  A against B is the
control pair: two plans that run the same kernel.  The noise floor is the largest |A - B| over the rounds; the claimed form counts as
faster only if its median is below BOTH static medians' mean by at least twice that floor in every round.  Results of different processes
are not comparable (the output lands elsewhere each time), which is why this is one process.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zaf-python_amd"))
import zafx  # noqa: E402
from zafx import _lib as _zlib  # noqa: E402
from zafx.core import Plan  # noqa: E402


def make_plan(dynamic):
    """A plan of its own (zafx.stft_plan caches): ZAFX_STFT_DYNAMIC is read when the plan is created."""
    os.environ["ZAFX_STFT_DYNAMIC"] = "1" if dynamic else "0"
    p = Plan(_zlib.STFT, 0, window_length=2048, step_length=1024, layout="FT", onesided=False)
    p.set_window(zafx.hamming(2048))
    del os.environ["ZAFX_STFT_DYNAMIC"]
    return p

B, N = 1024, 441000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    x = np.random.default_rng(0).standard_normal((8, N)).astype(np.float32)
    d_x = zafx.DeviceBuffer.from_host(np.tile(x, (B // 8, 1)))
    plans = [("static_a", make_plan(False)), ("claimed", make_plan(True)), ("static_b", make_plan(False))]
    d_out = zafx.DeviceBuffer(plans[0][1].out_shape(B, N), np.complex64)
    for i in range(240):
        plans[i % 3][1].execute(d_x, d_out, B, N)
        plans[i % 3][1].sync()
    rounds = []
    for r in range(args.rounds):
        med = {}
        for name, plan in plans:
            ms = []
            for _ in range(args.launches):
                plan.timer_start()
                plan.execute(d_x, d_out, B, N)
                ms.append(plan.timer_stop())
            med[name] = float(np.median(ms))
        rounds.append(med)
        print(f"round {r}: static A {med['static_a']:.4f}  claimed {med['claimed']:.4f}  static B {med['static_b']:.4f} ms   "
              f"|A - B| {abs(med['static_a'] - med['static_b']):.4f}   static - claimed {(med['static_a'] + med['static_b']) / 2 - med['claimed']:+.4f}")
    floor = max(abs(m["static_a"] - m["static_b"]) for m in rounds)
    gains = [(m["static_a"] + m["static_b"]) / 2 - m["claimed"] for m in rounds]
    faster = all(g >= 2 * floor for g in gains)
    stat = float(np.median([(m["static_a"] + m["static_b"]) / 2 for m in rounds]))
    print(f"noise floor (largest |A - B|) {floor:.4f} ms; static - claimed: min {min(gains):+.4f} median {float(np.median(gains)):+.4f} max {max(gains):+.4f} ms "
          f"({100 * float(np.median(gains)) / stat:+.2f} % of {stat:.4f} ms); claimed faster by twice the floor in every round: {faster}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"rounds": rounds, "noise_floor_ms": floor, "gains_ms": gains, "claimed_faster": faster,
                       "kernels": {n: p.last_kernel for n, p in plans}}, f, indent=1)


if __name__ == "__main__":
    main()
