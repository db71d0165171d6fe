"""Host time of one ragged call, end to end (call + sync), on batches small enough that the host's share shows: 1024 clips of 1 ... 33 frames.

    python tools/ragged_host_cost.py --one                         one process: the median of --calls calls of zafx_execute_ragged (STFT,
                                                                   W = 2048, rows of whole lines) and of zafx_execute_istft_ragged, as JSON
    python tools/ragged_host_cost.py --parent OLD.so [--rounds R]  R rounds of (OLD.so, this tree's library), a fresh process each, interleaved;
                                                                   prints both sets of medians, the parent's range and the verdict

What the ragged entry points do on the host -- the record loop, the route decision, the unit cut, the table upload -- is the only cost a change
of the routing code can move; the kernels are timed by tools/ragged_rates.py.  The margin is the parent's own run-to-run range in the same
session: this number has no other history."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "zaf-python_amd"))

N_CLIPS = 1024


def one(calls):
    import numpy as np
    import zafx
    r = np.random.default_rng(5)
    w, h = 2048, 1024
    frames = r.integers(1, 34, N_CLIPS).astype(np.int64)
    out = {}
    # forward: k_stft_ft16's RAGGED form
    plan = zafx.stft_plan(zafx.hamming(w), h, row_align=16)
    lengths = (frames - 1) * h
    offs = np.concatenate([[0], np.cumsum(lengths + 8)[:-1]]).astype(np.int64)
    d_in = zafx.DeviceBuffer.from_host(r.standard_normal(int(offs[-1] + lengths[-1] + 8)).astype(np.float32))
    d_out = zafx.DeviceBuffer((int(plan.ragged_layout(lengths)[0][-1]),), plan.out_dtype).fill_zero()
    # inverse: k_istft_ft16's RAGGED form
    iplan = zafx.istft_plan(zafx.hamming(w), h, row_align=4)
    pitch = (frames + 3) // 4 * 4
    ioffs = np.concatenate([[0], np.cumsum(w * pitch)[:-1]]).astype(np.int64)
    olen = np.maximum(frames * h - (w - h), 0)
    ooffs = np.concatenate([[0], np.cumsum(olen)[:-1]]).astype(np.int64)
    d_spec = zafx.DeviceBuffer((int(ioffs[-1] + w * pitch[-1]),), np.complex64).fill_zero()
    d_y = zafx.DeviceBuffer((int(ooffs[-1] + olen[-1]) + 8,), np.float32).fill_zero()
    runs = {"ragged": (plan, lambda: plan.execute_ragged(d_in, offs, lengths, d_out)),
            "istft_ragged": (iplan, lambda: iplan.execute_istft_ragged(d_spec, ioffs, frames, d_y, ooffs))}
    for name, (p, call) in runs.items():
        for _ in range(20):
            call()
        p.sync()
        times = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call()
            p.sync()
            times.append((time.perf_counter() - t0) * 1e6)
        out[name + "_us"] = round(statistics.median(times), 2)
        out[name + "_kernel"] = p.last_kernel
    for b in (d_in, d_out, d_spec, d_y):
        b.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.calls)))
        return 0
    res = {"parent": [], "this": []}
    sides = (("parent", os.path.abspath(a.parent)), ("this", None))
    for r in range(a.rounds):
        for side, lib in (sides if r % 2 == 0 else sides[::-1]):   # (who goes first alternates)
            env = dict(os.environ)
            env.pop("ZAFX_LIBRARY", None)
            if lib:
                env["ZAFX_LIBRARY"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", "--calls", str(a.calls)], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:   # (nothing more runs on the device after a failure)
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return p.returncode or 1
            res[side].append(json.loads(p.stdout.strip().split("\n")[-1]))
            print(side, res[side][-1], flush=True)
    ok = True
    for key in ("ragged_us", "istft_ragged_us"):
        old, new = [x[key] for x in res["parent"]], [x[key] for x in res["this"]]
        lo, hi, med = min(old), max(old), statistics.median(new)
        res[key] = {"parent": old, "this": new, "parent_range": [lo, hi], "this_median": med, "within": lo <= med <= hi, "not_slower": med <= hi}
        ok = ok and med <= hi
    print(json.dumps({k: v for k, v in res.items() if k.endswith("_us")}, indent=1))
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
