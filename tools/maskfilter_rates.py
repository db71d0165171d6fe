"""Rates of the mask filter kernel (k_maskfilter) in its mask layouts, beside the launches a caller would otherwise assemble, in one process.

    python tools/maskfilter_rates.py [--clips 1024] [--reps 30] [--out FILE]
    python tools/maskfilter_rates.py --only ft_rest --reps 2      one case alone, no comparison: the command of a counter run
                                                                  (rocprofv3 --pmc FETCH_SIZE -- python tools/maskfilter_rates.py --only ...)
    python tools/maskfilter_rates.py --ragged [--reps 30] [--per-slot 4,8,16] [--out FILE]

Workload: --clips mono clips x 441 000 samples (10 s at 44.1 kHz; 432 frames), Hamming 2048 / hop 1024, masks uniform in [0, 1], everything
device-resident (32 distinct noise clips and masks repeated over the batch).  Timed with the plan's HIP-event stopwatch, one launch per
reading, median (min, max) of --reps readings after three warm-up launches (as tools/center_rates.py):
  ft / ft_rest        ZAFX_MASKFILTER / _REST, mask (B, 1025, 432) compact
  ft433 / ft433_rest  the same with one more hop of samples: 433 frames, rows that start anywhere in a 128-byte line
  fta / fta_rest      mask rows at row_align = 32 (pitch 448): every row starts a line
  tf / tf_rest        mask (B, 432, 1025)
  assembled           the one-sided STFT launch plus the one-sided ISTFT launch of the same geometry on the same clips -- a floor for what a
                      caller assembles from those kernels: the mask pass over the spectrum between them does not exist on the device.
Algorithmic bytes per sample: 4 in, 4 out (8 with the rest) and the mask's 4 * 1025 / 1024; fractions of HBM peak against 8 TB/s (MI355X).
Exit status 1 when the fused call in its best layout is not faster than the assembled floor measured beside it.

--ragged (the recipe of tools/ragged_rates.py and tools/center_rates.py --ragged): 1024 mono clips of 5-15 s at 44.1 kHz, Hamming 2048 / 1024,
masks uniform in [0, 1], TF and FT, filtered and filtered + rest:
  ragged    one execute_masked_ragged of the clips and masks packed back to back (k_maskfilter_ragged; the cutting of the units and the table's
            upload included)
  padded    the same clips padded with zeros to the longest, with masks of the longest's shape, as one execute_masked
  per_clip  one execute_masked per clip on the plan's stream, all 1024 in one reading
median (min, max) of --reps readings after warm-up.  --per-slot: also times the ragged call with the cutter aiming at these numbers of units
per workgroup slot (ZAFX_MASKFILTER_UNITS_PER_SLOT) instead of the library's own.  Exit status 1 when a ragged call is not faster than its
padded twin.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zaf-python_amd"))
import zafx  # noqa: E402
from zafx import _lib  # noqa: E402

W, HOP, N, DISTINCT, HBM_PEAK = 2048, 1024, 441000, 32, 8.0e12
# name: (rest, layout, row_align, samples)
CASES = {"ft": (False, "FT", 0, N), "ft_rest": (True, "FT", 0, N), "ft433": (False, "FT", 0, N + HOP), "ft433_rest": (True, "FT", 0, N + HOP),
         "fta": (False, "FT", 32, N), "fta_rest": (True, "FT", 32, N), "tf": (False, "TF", 0, N), "tf_rest": (True, "TF", 0, N)}


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


class View:
    """`count` float32 at element `first` of a float32 DeviceBuffer, to hand to execute_masked (nothing to free)."""

    def __init__(self, buf, first, count):
        import ctypes
        self.ptr, self.dtype, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + 4 * first), np.dtype(np.float32), 4 * count, (count,)


def ragged_main(a):
    fs, clips = 44100, 1024
    lengths = np.random.default_rng(0).integers(5 * fs, 15 * fs + 1, clips).astype(np.int64)
    longest, total = int(lengths.max()), int(lengths.sum())
    in_offsets = np.zeros(clips, np.int64)
    in_offsets[1:] = np.cumsum(lengths)[:-1]
    window = zafx.hamming(W)
    res = {"device": zafx.device_name(0), "clips": clips, "window": W, "hop": HOP, "samples": total, "longest": longest, "reps": a.reps,
           "padded_over_ragged_samples": clips * longest / total}
    print(f"{clips} clips, {total} samples in all, longest {longest}: the padded batch holds {clips * longest / total:.3f} x as many", flush=True)
    # clip i = the first lengths[i] samples of noise clip i % DISTINCT, packed and padded
    small = zafx.DeviceBuffer.from_host(np.random.default_rng(1).standard_normal((DISTINCT, longest), dtype=np.float32))
    d_rag = zafx.DeviceBuffer((total,), np.float32)
    d_pad = zafx.DeviceBuffer((clips, longest), np.float32)
    d_pad.fill_zero()
    for i in range(clips):
        src, n = (i % DISTINCT) * longest * 4, int(lengths[i])
        d_rag.copy_from(small, nbytes=n * 4, dst_offset=int(in_offsets[i]) * 4, src_offset=src)
        d_pad.copy_from(small, nbytes=n * 4, dst_offset=i * longest * 4, src_offset=src)
    small.free()
    slow = False
    for layout in ("TF", "FT"):
        # a mask is uniform noise whatever its shape: mask i = the first elements of noise mask i % DISTINCT, in both arrays
        probe = zafx.maskfilter_plan(window, layout=layout)
        mask_offsets = probe.mask_ragged_layout(lengths)
        one_pad = int(np.prod(probe.mask_shape(1, longest)))
        noise = zafx.DeviceBuffer.from_host(np.random.default_rng(2).random((DISTINCT, one_pad), dtype=np.float32))
        m_rag = zafx.DeviceBuffer((int(mask_offsets[-1]),), np.float32)
        m_pad = zafx.DeviceBuffer((clips, one_pad), np.float32)
        for i in range(clips):
            src = (i % DISTINCT) * one_pad * 4
            m_rag.copy_from(noise, nbytes=int(mask_offsets[i + 1] - mask_offsets[i]) * 4, dst_offset=int(mask_offsets[i]) * 4, src_offset=src)
            m_pad.copy_from(noise, nbytes=one_pad * 4, dst_offset=i * one_pad * 4, src_offset=src)
        noise.free()
        for rest in (False, True):
            name = layout.lower() + ("_rest" if rest else "")
            plan = zafx.maskfilter_plan(window, rest=rest, layout=layout)
            blocks = 2 if rest else 1
            r = {}
            out = zafx.DeviceBuffer((blocks * total,), np.float32)
            out_offsets = blocks * in_offsets
            variants = [("ragged", None)] + [(f"ragged_per_slot_{v}", v) for v in a.per_slot]
            for key, per_slot in variants:
                if per_slot is None:
                    os.environ.pop("ZAFX_MASKFILTER_UNITS_PER_SLOT", None)
                else:
                    os.environ["ZAFX_MASKFILTER_UNITS_PER_SLOT"] = str(per_slot)
                r[key] = timed(plan, lambda: plan.execute_masked_ragged(d_rag, in_offsets, lengths, m_rag, mask_offsets, out, out_offsets), a.reps)
                r[key]["kernel"] = plan.last_kernel
            os.environ.pop("ZAFX_MASKFILTER_UNITS_PER_SLOT", None)
            views = [(View(d_rag, int(o), int(n)), View(m_rag, int(mo), int(me - mo)), View(out, int(blocks * o), int(blocks * n)), int(n))
                     for o, n, mo, me in zip(in_offsets, lengths, mask_offsets[:-1], mask_offsets[1:])]

            lib = _lib.load()

            def per_clip():   # (the library's entry point itself: the Python method's checks cost more than the launch)
                for v_in, v_mask, v_out, n in views:
                    _lib.check(lib.zafx_execute_masked(plan.handle, v_in.ptr, v_mask.ptr, v_out.ptr, 1, n), "zafx_execute_masked")
            r["per_clip"] = timed(plan, per_clip, a.reps, warm=1)
            r["per_clip"]["kernel"] = plan.last_kernel
            out.free()
            out = zafx.DeviceBuffer(plan.out_shape(clips, longest), np.float32)
            r["padded"] = timed(plan, lambda: plan.execute_masked(d_pad, m_pad, out, clips, longest), a.reps)
            r["padded"]["kernel"] = plan.last_kernel
            out.free()
            for key, v in r.items():
                v["msamples_per_s"] = total / (v["median_ms"] * 1e3)
                print(f"{name:8s} {key:20s} {v['median_ms']:8.3f} ms ({v['min_ms']:.3f}-{v['max_ms']:.3f})  {v['msamples_per_s']:9.0f} Msamples/s  [{v['kernel']}]", flush=True)
            r["ragged_over_padded"] = r["ragged"]["median_ms"] / r["padded"]["median_ms"]
            r["per_clip_over_ragged"] = r["per_clip"]["median_ms"] / r["ragged"]["median_ms"]
            print(f"{name:8s} ragged / padded {r['ragged_over_padded']:.3f}, per clip / ragged {r['per_clip_over_ragged']:.2f}", flush=True)
            slow = slow or not r["ragged"]["median_ms"] < r["padded"]["median_ms"]
            res[name] = r
        m_rag.free(), m_pad.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if slow:
        print("FAILED: a ragged call is not faster than the same clips padded to the longest", flush=True)
        sys.exit(1)


def run_case(name, window, b, reps, clips_of):
    rest, layout, row_align, n = CASES[name]
    plan = zafx.maskfilter_plan(window, rest=rest, layout=layout, row_align=row_align)
    rows, frames = plan.mask_dims(n)
    shape = plan.mask_shape(DISTINCT, n)
    m = np.random.default_rng(2).random(shape, dtype=np.float32)   # (the row padding too: it is never read)
    d_x, d_m = clips_of(n), replicated(m, b)
    d_out = zafx.DeviceBuffer(plan.out_shape(b, n), np.float32)
    r = timed(plan, lambda: plan.execute_masked(d_x, d_m, d_out, b, n), reps)
    d_m.free(), d_out.free()
    nbytes = 4 + (8 if rest else 4) + 4.0 * rows * frames / n
    r.update(kernel=plan.last_kernel, samples=n, frames=frames, mask_pitch=plan.row_pitch(n), msamples_per_s=b * n / (r["median_ms"] * 1e3),
             algorithmic_bytes_per_sample=nbytes, hbm_fraction=b * n * nbytes / (r["median_ms"] * 1e-3) / HBM_PEAK)
    print(f"{name:11s} {r['median_ms']:8.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f})  {r['msamples_per_s']:9.0f} Msamples/s  "
          f"{r['hbm_fraction']:.3f} of HBM peak on {nbytes:.2f} B per sample  T={frames} pitch={r['mask_pitch']}  [{r['kernel']}]", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="comma-separated case names; no assembled comparison")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--per-slot", type=lambda v: [int(t) for t in v.split(",") if t], default=[])
    a = ap.parse_args()
    if a.ragged:
        return ragged_main(a)
    b = a.clips
    window = zafx.hamming(W)
    x = np.random.default_rng(1).standard_normal((DISTINCT, N + HOP), dtype=np.float32)
    cache = {}

    def clips_of(n):
        if n not in cache:
            cache[n] = replicated(np.ascontiguousarray(x[:, :n]), b)
        return cache[n]
    names = [t for t in a.only.split(",") if t] or list(CASES)
    res = {"device": zafx.device_name(0), "clips": b, "samples": N, "window": W, "hop": HOP, "reps": a.reps}
    for name in names:
        res[name] = run_case(name, window, b, a.reps, clips_of)
    slow = False
    if not a.only:
        # the assembly's transforms: one-sided STFT, one-sided ISTFT of the (masked) spectrum
        fwd, inv = zafx.stft_plan(window, HOP, onesided=True, row_align=16), zafx.istft_plan(window, HOP, onesided=True, row_align=16)
        t = fwd.out_dims(N)[1]
        spec = zafx.DeviceBuffer(fwd.out_shape(b, N), fwd.out_dtype)
        back = zafx.DeviceBuffer(inv.out_shape(b, t), inv.out_dtype)
        total = 0.0
        for name, plan, launch in (("stft", fwd, lambda: fwd.execute(clips_of(N), spec, b, N)), ("istft", inv, lambda: inv.execute(spec, back, b, t))):
            r = timed(plan, launch, a.reps)
            r["kernel"] = plan.last_kernel
            res[name] = r
            total += r["median_ms"]
            print(f"{name:11s} {r['median_ms']:8.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f})  [{r['kernel']}]", flush=True)
        best = min((k for k in CASES if not CASES[k][0] and CASES[k][3] == N), key=lambda k: res[k]["median_ms"])
        res["assembled_ms"], res["best_layout"] = total, best
        res["best_over_assembled"] = res[best]["median_ms"] / total
        res["ft_over_tf"] = res["ft"]["median_ms"] / res["tf"]["median_ms"]
        print(f"assembled   {total:8.3f} ms (one STFT + one ISTFT launch, no mask pass);  {best} / assembled = {res['best_over_assembled']:.3f};  "
              f"ft / tf = {res['ft_over_tf']:.3f}", flush=True)
        slow = not res[best]["median_ms"] < total
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if slow:
        print("FAILED: the fused call in its best layout is not faster than the assembled floor", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
