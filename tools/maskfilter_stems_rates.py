"""Rates of the mask filter with several masks per clip (k_maskfilter_stems) beside the S launches of k_maskfilter a caller ran before it
existed, in one process.

    python tools/maskfilter_stems_rates.py [--clips 1024] [--reps 30] [--stems 2,4] [--out FILE]
    python tools/maskfilter_stems_rates.py --only stems4 --reps 2      one case alone, no comparison: the command of a counter run

Workload: --clips mono clips x 441 000 samples (10 s at 44.1 kHz; 432 frames), Hamming 2048 / hop 1024, "TF" masks uniform in [0, 1],
everything device-resident (32 distinct noise clips and mask sets repeated over the batch).  Timed with the plan's HIP-event stopwatch, median
(min, max) of --reps readings after three warm-up readings (as tools/maskfilter_rates.py).  Per S and plan kind (filtered; filtered + rest):
  stemsS / stemsS_rest        one execute_masked_stems: masks (B, S, 432, 1025), output (B, S, N) / (B, S + 1, N)
  singlesS / singlesS_rest    S execute_masked launches of the same plan kind over the same clips, stem s's masks as a (B, 432, 1025) array of their
                              own, output (B, N) / (B, 2, N) per launch; all S in one reading.  With the rest this is a floor for the old way: each
                              launch leaves x - y_s, and the chain ((x - y_0) - y_1) - ... would take further passes.
Algorithmic bytes per sample: stems 4 + 4 S (+ 4 with the rest) and the masks' 4 S * 1025 / 1024; singles S * (4 + 4 (8 with the rest)) and the same
masks.  The stems call counts as faster when its median lies below the singles' median by more than the larger of the two (max - min) spreads;
exit status 1 when it does not at S = 4.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zaf-python_amd"))
import zafx  # noqa: E402

W, HOP, N, DISTINCT, HBM_PEAK = 2048, 1024, 441000, 32, 8.0e12


def timed(plan, launch, reps, warm=3):
    for _ in range(warm):
        launch()
    plan.sync()
    ms = []
    for _ in range(reps):
        plan.timer_start()
        launch()
        ms.append(plan.timer_stop())
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def replicated(small, one, clips, src_first=0, src_pitch=None):
    """Device array of `clips` items of `one` bytes: item i = the `one` bytes at src_first + (i % DISTINCT) * src_pitch of the device array `small`."""
    src_pitch = one if src_pitch is None else src_pitch
    big = zafx.DeviceBuffer((clips * one // 4,), np.float32)
    for i in range(clips):
        big.copy_from(small, nbytes=one, dst_offset=i * one, src_offset=src_first + (i % DISTINCT) * src_pitch)
    return big


def show(name, r):
    print(f"{name:14s} {r['median_ms']:8.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f})  {r['msamples_per_s']:9.0f} Msamples/s  "
          f"{r['hbm_fraction']:.3f} of HBM peak on {r['algorithmic_bytes_per_sample']:.2f} B per sample  [{r['kernel']}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--stems", type=lambda v: [int(t) for t in v.split(",") if t], default=[2, 4])
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="comma-separated case names (stems4, singles4_rest, ...); no comparison")
    a = ap.parse_args()
    b = a.clips
    only = [t for t in a.only.split(",") if t]
    window = zafx.hamming(W)
    plans = {rest: zafx.maskfilter_plan(window, rest=rest, layout="TF") for rest in (False, True)}
    rows, frames = plans[False].mask_dims(N)
    one_mask = rows * frames * 4
    host_x = zafx.DeviceBuffer.from_host(np.random.default_rng(1).standard_normal((DISTINCT, N), dtype=np.float32))
    d_x = replicated(host_x, N * 4, b)
    host_x.free()
    res = {"device": zafx.device_name(0), "clips": b, "samples": N, "window": W, "hop": HOP, "frames": frames, "reps": a.reps,
           "compute_units": plans[False].compute_units}
    slow = False
    for s in a.stems:
        small = zafx.DeviceBuffer.from_host(np.random.default_rng([2, s]).random((DISTINCT, s, frames, rows), dtype=np.float32))
        d_stems = replicated(small, s * one_mask, b)
        d_single = [replicated(small, one_mask, b, src_first=j * one_mask, src_pitch=s * one_mask) for j in range(s)]   # the same values, a (B, T, rows) array per stem
        small.free()
        for rest in (False, True):
            plan, tag = plans[rest], "_rest" if rest else ""
            mask_bytes = 4.0 * s * rows * frames / N
            cases = {}
            name = f"stems{s}{tag}"
            if not only or name in only:
                d_out = zafx.DeviceBuffer(plan.stems_out_shape(b, N, s), np.float32)
                r = timed(plan, lambda: plan.execute_masked_stems(d_x, d_stems, d_out, b, N, s), a.reps)
                d_out.free()
                r.update(kernel=plan.last_kernel, launches=1, algorithmic_bytes_per_sample=4 + 4 * s + (4 if rest else 0) + mask_bytes)
                cases[name] = r
            name = f"singles{s}{tag}"
            if not only or name in only:
                outs = [zafx.DeviceBuffer(plan.out_shape(b, N), np.float32) for _ in range(s)]

                def singles():
                    for j in range(s):
                        plan.execute_masked(d_x, d_single[j], outs[j], b, N)
                r = timed(plan, singles, a.reps)
                for o in outs:
                    o.free()
                r.update(kernel=plan.last_kernel, launches=s, algorithmic_bytes_per_sample=s * (4 + (8 if rest else 4)) + mask_bytes)
                cases[name] = r
            for name, r in cases.items():
                r["msamples_per_s"] = b * N / (r["median_ms"] * 1e3)
                r["hbm_fraction"] = b * N * r["algorithmic_bytes_per_sample"] / (r["median_ms"] * 1e-3) / HBM_PEAK
                show(name, r)
                res[name] = r
            if len(cases) == 2:
                st, si = cases[f"stems{s}{tag}"], cases[f"singles{s}{tag}"]
                spread = max(st["max_ms"] - st["min_ms"], si["max_ms"] - si["min_ms"])
                faster = si["median_ms"] - st["median_ms"] > spread
                res[f"stems{s}{tag}_over_singles"] = st["median_ms"] / si["median_ms"]
                res[f"stems{s}{tag}_faster"] = bool(faster)
                print(f"stems{s}{tag} / singles{s}{tag} = {st['median_ms'] / si['median_ms']:.3f}; larger spread {spread:.3f} ms: "
                      f"{'faster' if faster else 'NOT faster'}", flush=True)
                slow = slow or (s == 4 and not faster)
        d_stems.free()
        for d in d_single:
            d.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if slow:
        print("FAILED: at S = 4 the stems call is not faster than S launches of k_maskfilter", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
