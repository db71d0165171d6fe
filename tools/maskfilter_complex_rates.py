"""Rates of the mask filter under complex masks (k_maskfilter_complex, k_maskfilter_complex_ragged) beside what a caller has without it, in one
process.

    python tools/maskfilter_complex_rates.py [--clips 1024] [--reps 30] [--out FILE] [--no-equal] [--no-ragged]

Equal-length: --clips mono clips x 441 000 samples (10 s at 44.1 kHz; 432 frames), Hamming 2048 / hop 1024, complex64 masks uniform in the unit
disc, (B, 432, 1025), everything device-resident (32 distinct noise clips and masks repeated over the batch).  Timed with the plan's HIP-event
stopwatch, one launch per reading, median (min, max) of --reps readings after three warm-up launches (as tools/maskfilter_rates.py):
  complex / complex_rest   execute_masked_complex on a ZAFX_MASKFILTER / _REST plan of ZAFX_LAYOUT_TF
  real / real_rest         execute_masked with real masks (B, 432, 1025) on the same plans and clips: the ratio is reported, not barred
  assembled_ft / _tf       the one-sided STFT launch plus the one-sided ISTFT launch of the same geometry on the same clips, spectrum in the
                           reference layout on whole lines (row_align 16: the floor of tools/maskfilter_rates.py) and frame-major -- a floor
                           for what a caller assembles: the mask pass over the 3.6 GB spectrum between them does not exist on the device.
Algorithmic bytes per sample: 4 in, 4 out (8 with the rest), 8 * 1025 / 1024 of mask; fractions of HBM peak against 8 TB/s (MI355X).

Ragged: 1024 mono clips of 5-15 s at 44.1 kHz (the recipe of tools/maskfilter_rates.py --ragged), filtered and filtered + rest:
  ragged    one execute_masked_complex_ragged of the clips and masks packed back to back (the cutting of the units and the table's upload included)
  padded    the same clips padded with zeros to the longest, with masks of the longest's shape, as one execute_masked_complex
  per_clip  one zafx_execute_masked_complex per clip on the plan's stream, all 1024 in one reading
  real_ragged  execute_masked_ragged with real TF masks on the same clips (reported)

Verdicts by the project's rule for "faster": the median lies below the baseline's by more than the larger of the two (max - min) spreads.  Barred:
complex against the faster assembled floor; ragged against padded and against per_clip.  Exit status 0 either way; the verdicts are in the JSON.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zaf-python_amd"))
import zafx  # noqa: E402
from zafx import _lib  # noqa: E402

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


def faster(a, b):
    """a's median below b's by more than the larger of the two spreads."""
    return bool(b["median_ms"] - a["median_ms"] > max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"]))


def show(name, r, extra=""):
    print(f"{name:24s} {r['median_ms']:8.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f})  {extra}  [{r.get('kernel', '')}]", flush=True)


def replicated(host, clips):
    """(DISTINCT, ...) host array -> (clips, ...) device array, clip i = host[i % DISTINCT]."""
    small = zafx.DeviceBuffer.from_host(host)
    big = zafx.DeviceBuffer((clips,) + host.shape[1:], host.dtype)
    one = host[0].nbytes
    for i in range(clips):
        big.copy_from(small, nbytes=one, dst_offset=i * one, src_offset=(i % DISTINCT) * one)
    small.free()
    return big


def disc(rng, shape):
    return (np.sqrt(rng.random(shape)) * np.exp(2j * np.pi * rng.random(shape))).astype(np.complex64)


class View:
    """`count` elements of `dtype` at element `first` of a DeviceBuffer of that dtype (nothing to free)."""

    def __init__(self, buf, first, count, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        self.ptr, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + self.dtype.itemsize * first), self.dtype.itemsize * count, (count,)


def equal_main(a, res):
    b, window = a.clips, zafx.hamming(W)
    d_x = replicated(np.random.default_rng(1).standard_normal((DISTINCT, N), dtype=np.float32), b)
    probe = zafx.maskfilter_plan(window, layout="TF")
    rows, frames = probe.mask_dims(N)
    shape = probe.mask_shape(DISTINCT, N)
    d_mc = replicated(disc(np.random.default_rng(2), shape), b)
    d_mr = replicated(np.random.default_rng(2).random(shape, dtype=np.float32), b)
    for rest in (False, True):
        plan = zafx.maskfilter_plan(window, rest=rest, layout="TF")
        d_out = zafx.DeviceBuffer(plan.out_shape(b, N), np.float32)
        for name, launch, mask_bytes in (("complex", lambda: plan.execute_masked_complex(d_x, d_mc, d_out, b, N), 8.0),
                                         ("real", lambda: plan.execute_masked(d_x, d_mr, d_out, b, N), 4.0)):
            r = timed(plan, launch, a.reps)
            nbytes = 4 + (8 if rest else 4) + mask_bytes * rows * frames / N
            r.update(kernel=plan.last_kernel, msamples_per_s=b * N / (r["median_ms"] * 1e3), algorithmic_bytes_per_sample=nbytes,
                     hbm_fraction=b * N * nbytes / (r["median_ms"] * 1e-3) / HBM_PEAK)
            key = name + ("_rest" if rest else "")
            res[key] = r
            show(key, r, f"{r['msamples_per_s']:9.0f} Msamples/s  {r['hbm_fraction']:.3f} of HBM peak on {nbytes:.2f} B per sample")
        d_out.free()
    d_mc.free(), d_mr.free()
    for tag, kw in (("ft", dict(row_align=16)), ("tf", dict(layout="TF"))):
        fwd, inv = zafx.stft_plan(window, HOP, onesided=True, **kw), zafx.istft_plan(window, HOP, onesided=True, **kw)
        t = fwd.out_dims(N)[1]
        spec = zafx.DeviceBuffer(fwd.out_shape(b, N), fwd.out_dtype)
        back = zafx.DeviceBuffer(inv.out_shape(b, t), inv.out_dtype)
        parts = {}
        for name, plan, launch in (("stft", fwd, lambda: fwd.execute(d_x, spec, b, N)), ("istft", inv, lambda: inv.execute(spec, back, b, t))):
            r = timed(plan, launch, a.reps)
            r["kernel"] = plan.last_kernel
            parts[name] = r
            show(f"{tag} {name}", r)
        # the sum of two launches: medians, minima and maxima add (the spread of the sum is at most the sum of the spreads)
        total = {k: parts["stft"][k] + parts["istft"][k] for k in ("median_ms", "min_ms", "max_ms")}
        res[f"assembled_{tag}"] = dict(total, stft=parts["stft"], istft=parts["istft"])
        show(f"assembled_{tag}", total, "one STFT + one ISTFT launch, no mask pass")
        spec.free(), back.free()
    d_x.free()
    floor = min(("assembled_ft", "assembled_tf"), key=lambda k: res[k]["median_ms"])
    res["floor"] = floor
    res["complex_over_floor"] = res["complex"]["median_ms"] / res[floor]["median_ms"]
    res["complex_over_real"] = res["complex"]["median_ms"] / res["real"]["median_ms"]
    res["complex_rest_over_real_rest"] = res["complex_rest"]["median_ms"] / res["real_rest"]["median_ms"]
    res["complex_faster_than_floor"] = faster(res["complex"], res[floor])
    print(f"complex / {floor} = {res['complex_over_floor']:.3f} ({'faster' if res['complex_faster_than_floor'] else 'NOT faster'} by the rule);  "
          f"complex / real = {res['complex_over_real']:.3f}, with rest {res['complex_rest_over_real_rest']:.3f}", flush=True)


def ragged_main(a, res):
    fs, clips = 44100, 1024
    lengths = np.random.default_rng(0).integers(5 * fs, 15 * fs + 1, clips).astype(np.int64)
    longest, total = int(lengths.max()), int(lengths.sum())
    in_offsets = np.zeros(clips, np.int64)
    in_offsets[1:] = np.cumsum(lengths)[:-1]
    window = zafx.hamming(W)
    res.update(ragged_clips=clips, ragged_samples=total, longest=longest, padded_over_ragged_samples=clips * longest / total)
    print(f"{clips} clips, {total} samples in all, longest {longest}: the padded batch holds {clips * longest / total:.3f} x as many", flush=True)
    small = zafx.DeviceBuffer.from_host(np.random.default_rng(1).standard_normal((DISTINCT, longest), dtype=np.float32))
    d_rag = zafx.DeviceBuffer((total,), np.float32)
    d_pad = zafx.DeviceBuffer((clips, longest), np.float32)
    d_pad.fill_zero()
    for i in range(clips):
        src, n = (i % DISTINCT) * longest * 4, int(lengths[i])
        d_rag.copy_from(small, nbytes=n * 4, dst_offset=int(in_offsets[i]) * 4, src_offset=src)
        d_pad.copy_from(small, nbytes=n * 4, dst_offset=i * longest * 4, src_offset=src)
    small.free()
    probe = zafx.maskfilter_plan(window, layout="TF")
    mask_offsets = probe.mask_ragged_layout(lengths)
    one_pad = int(np.prod(probe.mask_shape(1, longest)))
    masks = {}
    for dtype, noise in ((np.complex64, disc(np.random.default_rng(2), (DISTINCT, one_pad))), (np.float32, np.random.default_rng(2).random((DISTINCT, one_pad), dtype=np.float32))):
        size = np.dtype(dtype).itemsize
        d_noise = zafx.DeviceBuffer.from_host(noise)
        m_rag = zafx.DeviceBuffer((int(mask_offsets[-1]),), dtype)
        m_pad = zafx.DeviceBuffer((clips, one_pad), dtype) if dtype is np.complex64 else None
        for i in range(clips):
            src = (i % DISTINCT) * one_pad * size
            m_rag.copy_from(d_noise, nbytes=int(mask_offsets[i + 1] - mask_offsets[i]) * size, dst_offset=int(mask_offsets[i]) * size, src_offset=src)
            if m_pad is not None:
                m_pad.copy_from(d_noise, nbytes=one_pad * size, dst_offset=i * one_pad * size, src_offset=src)
        d_noise.free()
        masks[dtype] = (m_rag, m_pad)
    (mc_rag, mc_pad), (mr_rag, _) = masks[np.complex64], masks[np.float32]
    lib = _lib.load()
    for rest in (False, True):
        name = "ragged" + ("_rest" if rest else "")
        plan = zafx.maskfilter_plan(window, rest=rest, layout="TF")
        blocks = 2 if rest else 1
        out = zafx.DeviceBuffer((blocks * total,), np.float32)
        out_offsets = blocks * in_offsets
        r = {}
        r["ragged"] = timed(plan, lambda: plan.execute_masked_complex_ragged(d_rag, in_offsets, lengths, mc_rag, mask_offsets, out, out_offsets), a.reps)
        r["ragged"]["kernel"] = plan.last_kernel
        r["real_ragged"] = timed(plan, lambda: plan.execute_masked_ragged(d_rag, in_offsets, lengths, mr_rag, mask_offsets, out, out_offsets), a.reps)
        r["real_ragged"]["kernel"] = plan.last_kernel
        views = [(View(d_rag, int(o), int(n)), View(mc_rag, int(mo), int(me - mo), np.complex64), View(out, int(blocks * o), int(blocks * n)), int(n))
                 for o, n, mo, me in zip(in_offsets, lengths, mask_offsets[:-1], mask_offsets[1:])]

        def per_clip():   # (the library's entry point itself: the Python method's checks cost more than the launch)
            for v_in, v_mask, v_out, n in views:
                _lib.check(lib.zafx_execute_masked_complex(plan.handle, v_in.ptr, v_mask.ptr, v_out.ptr, 1, n), "zafx_execute_masked_complex")
        r["per_clip"] = timed(plan, per_clip, a.reps, warm=1)
        r["per_clip"]["kernel"] = plan.last_kernel
        out.free()
        out = zafx.DeviceBuffer(plan.out_shape(clips, longest), np.float32)
        r["padded"] = timed(plan, lambda: plan.execute_masked_complex(d_pad, mc_pad, out, clips, longest), a.reps)
        r["padded"]["kernel"] = plan.last_kernel
        out.free()
        for key, v in r.items():
            v["msamples_per_s"] = total / (v["median_ms"] * 1e3)
            show(f"{name} {key}", v, f"{v['msamples_per_s']:9.0f} Msamples/s")
        r["ragged_over_padded"] = r["ragged"]["median_ms"] / r["padded"]["median_ms"]
        r["per_clip_over_ragged"] = r["per_clip"]["median_ms"] / r["ragged"]["median_ms"]
        r["ragged_over_real_ragged"] = r["ragged"]["median_ms"] / r["real_ragged"]["median_ms"]
        r["faster_than_padded"], r["faster_than_per_clip"] = faster(r["ragged"], r["padded"]), faster(r["ragged"], r["per_clip"])
        print(f"{name}: ragged / padded {r['ragged_over_padded']:.3f} ({'faster' if r['faster_than_padded'] else 'NOT faster'}), per clip / ragged "
              f"{r['per_clip_over_ragged']:.2f} ({'faster' if r['faster_than_per_clip'] else 'NOT faster'}), ragged / real ragged {r['ragged_over_real_ragged']:.3f}", flush=True)
        res[name] = r
    for buf in (d_rag, d_pad, mc_rag, mc_pad, mr_rag):
        buf.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-equal", action="store_true")
    ap.add_argument("--no-ragged", action="store_true")
    a = ap.parse_args()
    res = {"device": zafx.device_name(0), "clips": a.clips, "samples": N, "window": W, "hop": HOP, "reps": a.reps}
    if not a.no_equal:
        equal_main(a, res)
    if not a.no_ragged:
        ragged_main(a, res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
