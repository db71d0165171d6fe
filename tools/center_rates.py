"""Rates of the center / sides kernel (k_center) beside the launches a caller would otherwise assemble, in one process.

    python tools/center_rates.py [--clips 1024] [--reps 20] [--out FILE]
    python tools/center_rates.py --ragged [--reps 30] [--per-slot 4,8,16] [--out FILE]

Workload: --clips stereo clips x 441 000 sample frames (10 s at 44.1 kHz), Hamming 2048 / hop 1024, device-resident (32 distinct noise
clips repeated over the batch).  Timed with the plan's HIP-event stopwatch, one launch per reading, median (min, max) of --reps readings
after three warm-up launches (as tools/ragged_rates.py):
  center         ZAFX_CENTER        16 algorithmic bytes per sample frame (8 read, 8 written)
  center_sides   ZAFX_CENTER_SIDES  24 (8 read, 16 written)
  assembled      two one-sided STFT launches (left, right) and two one-sided ISTFT launches of the same geometry on the mono halves of
                 the same data -- a floor for what a caller assembles from those kernels: it leaves out the de-interleave, the mask
                 pass over the two spectra and the re-interleave.
Fractions of HBM peak are taken on the algorithmic bytes against 8 TB/s (MI355X).

--ragged (the recipe of tools/ragged_rates.py): 1024 stereo clips of 5-15 s at 44.1 kHz, Hamming 2048 / 1024, center and center + sides:
  ragged   one execute_center_ragged of the clips packed back to back (k_center_ragged; the cutting of the units and the table's upload included)
  padded   the same clips padded with zeros to the longest, as one execute of the equal-length kernel
  equal    1024 clips of 10 s as one execute (the rate per sample frame to compare with)
one launch per reading, median (min, max) of --reps readings after warm-up.  --per-slot: also times the ragged call with the cutter aiming at
these numbers of units per workgroup slot (ZAFX_CENTER_UNITS_PER_SLOT) instead of the library's own.  Exit status 1 when a ragged call is not
faster than its padded twin.
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


def replicated(host, clips):
    """(DISTINCT, ...) host array -> (clips, ...) device array, clip i = host[i % DISTINCT]."""
    small = zafx.DeviceBuffer.from_host(host)
    big = zafx.DeviceBuffer((clips,) + host.shape[1:], host.dtype)
    one = host[0].nbytes
    for i in range(clips):
        big.copy_from(small, nbytes=one, dst_offset=i * one, src_offset=(i % DISTINCT) * one)
    small.free()
    return big


def ragged_main(a):
    fs, clips = 44100, 1024
    lengths = np.random.default_rng(0).integers(5 * fs, 15 * fs + 1, clips).astype(np.int64)
    longest, total = int(lengths.max()), int(lengths.sum())
    in_offsets = np.zeros(clips, np.int64)
    in_offsets[1:] = np.cumsum(lengths)[:-1]
    window = zafx.hamming(W)
    small = zafx.DeviceBuffer.from_host(np.random.default_rng(1).standard_normal((DISTINCT, longest, 2), dtype=np.float32))
    # clip i = the first lengths[i] sample frames of noise clip i % DISTINCT, in all three arrays
    d_rag = zafx.DeviceBuffer((total, 2), np.float32)
    d_pad = zafx.DeviceBuffer((clips, longest, 2), np.float32)
    d_pad.fill_zero()
    d_eq = zafx.DeviceBuffer((clips, N, 2), np.float32)
    for i in range(clips):
        src, n = (i % DISTINCT) * longest * 8, int(lengths[i])
        d_rag.copy_from(small, nbytes=n * 8, dst_offset=int(in_offsets[i]) * 8, src_offset=src)
        d_pad.copy_from(small, nbytes=n * 8, dst_offset=i * longest * 8, src_offset=src)
        d_eq.copy_from(small, nbytes=N * 8, dst_offset=i * N * 8, src_offset=src)
    small.free()
    res = {"device": zafx.device_name(0), "clips": clips, "window": W, "hop": HOP, "sample_frames": total, "longest": longest, "reps": a.reps,
           "padded_over_ragged_sample_frames": clips * longest / total}
    print(f"{clips} clips, {total} sample frames in all, longest {longest}: the padded batch holds {clips * longest / total:.3f} x as many", flush=True)
    slow = False
    for name, sides in (("center", False), ("center_sides", True)):
        plan = zafx.center_plan(window, sides=sides)
        blocks = 2 if sides else 1
        r = {}
        out = zafx.DeviceBuffer((blocks * total, 2), np.float32)
        variants = [("ragged", None)] + [(f"ragged_per_slot_{v}", v) for v in a.per_slot]
        for key, per_slot in variants:
            if per_slot is None:
                os.environ.pop("ZAFX_CENTER_UNITS_PER_SLOT", None)
            else:
                os.environ["ZAFX_CENTER_UNITS_PER_SLOT"] = str(per_slot)
            r[key] = timed(plan, lambda: plan.execute_center_ragged(d_rag, in_offsets, lengths, out, blocks * in_offsets), a.reps)
            r[key]["kernel"] = plan.last_kernel
        os.environ.pop("ZAFX_CENTER_UNITS_PER_SLOT", None)
        out.free()
        for key, buf, n in (("padded", d_pad, longest), ("equal", d_eq, N)):
            out = zafx.DeviceBuffer(plan.out_shape(clips, n), np.float32)
            r[key] = timed(plan, lambda: plan.execute(buf, out, clips, n), a.reps)
            r[key]["kernel"] = plan.last_kernel
            out.free()
        frames = dict({key: total for key, _ in variants}, padded=total, equal=clips * N)
        for key, v in r.items():
            v["msample_frames_per_s"] = frames[key] / (v["median_ms"] * 1e3)
            print(f"{name:13s} {key:20s} {v['median_ms']:8.3f} ms ({v['min_ms']:.3f}-{v['max_ms']:.3f})  {v['msample_frames_per_s']:9.0f} Msample-frames/s  [{v['kernel']}]",
                  flush=True)
        r["ragged_over_padded"] = r["ragged"]["median_ms"] / r["padded"]["median_ms"]
        r["ragged_rate_over_equal_rate"] = r["ragged"]["msample_frames_per_s"] / r["equal"]["msample_frames_per_s"]
        print(f"{name:13s} ragged / padded {r['ragged_over_padded']:.3f}, rate per sample frame ragged / equal {r['ragged_rate_over_equal_rate']:.3f}", flush=True)
        slow = slow or not r["ragged"]["median_ms"] < r["padded"]["median_ms"]
        res[name] = r
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if slow:
        print("FAILED: a ragged call is not faster than the same clips padded to the longest", flush=True)
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--out", default="")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--per-slot", type=lambda v: [int(t) for t in v.split(",") if t], default=[])
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 30 if a.ragged else 20
    if a.ragged:
        return ragged_main(a)
    b = a.clips
    window = zafx.hamming(W)
    x = np.random.default_rng(1).standard_normal((DISTINCT, N, 2), dtype=np.float32)
    d_x = replicated(x, b)
    res = {"device": zafx.device_name(0), "clips": b, "sample_frames": N, "window": W, "hop": HOP, "reps": a.reps}
    frames = b * N
    for name, sides, nbytes in (("center", False, 16), ("center_sides", True, 24)):
        plan = zafx.center_plan(window, sides=sides)
        d_out = zafx.DeviceBuffer(plan.out_shape(b, N), plan.out_dtype)
        r = timed(plan, lambda: plan.execute(d_x, d_out, b, N), a.reps)
        r["kernel"] = plan.last_kernel
        r["msample_frames_per_s"] = frames / (r["median_ms"] * 1e3)
        r["hbm_fraction"] = frames * nbytes / (r["median_ms"] * 1e-3) / HBM_PEAK
        res[name] = r
        d_out.free()
        print(f"{name:13s} {r['median_ms']:8.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f})  {r['msample_frames_per_s']:9.0f} Msample-frames/s  "
              f"{r['hbm_fraction']:.3f} of HBM peak on {nbytes} B per sample frame  [{r['kernel']}]", flush=True)
    d_x.free()
    # the assembly's transforms: one-sided STFT of each channel, one-sided ISTFT of each (masked) spectrum
    fwd, inv = zafx.stft_plan(window, HOP, onesided=True, row_align=16), zafx.istft_plan(window, HOP, onesided=True, row_align=16)
    t = fwd.out_dims(N)[1]
    mono = [replicated(np.ascontiguousarray(x[:, :, c]), b) for c in (0, 1)]
    spec = [zafx.DeviceBuffer(fwd.out_shape(b, N), fwd.out_dtype) for _ in (0, 1)]
    back = [zafx.DeviceBuffer(inv.out_shape(b, t), inv.out_dtype) for _ in (0, 1)]
    total = 0.0
    for name, plan, launch in (("stft_left", fwd, lambda: fwd.execute(mono[0], spec[0], b, N)), ("stft_right", fwd, lambda: fwd.execute(mono[1], spec[1], b, N)),
                               ("istft_left", inv, lambda: inv.execute(spec[0], back[0], b, t)), ("istft_right", inv, lambda: inv.execute(spec[1], back[1], b, t))):
        r = timed(plan, launch, a.reps)
        r["kernel"] = plan.last_kernel
        res[name] = r
        total += r["median_ms"]
        print(f"{name:13s} {r['median_ms']:8.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f})  [{r['kernel']}]", flush=True)
    res["assembled_ms"] = total
    res["center_sides_over_assembled"] = res["center_sides"]["median_ms"] / total
    print(f"assembled     {total:8.3f} ms (two STFT + two ISTFT launches);  center_sides / assembled = {res['center_sides_over_assembled']:.3f}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
