"""Rates of the stereo mask filter (k_maskfilter_stereo, k_maskfilter_stereo_ragged) beside what a caller has without it, in one process.

    python tools/maskfilter_stereo_rates.py [--clips 1024] [--reps 30] [--out FILE] [--no-equal] [--no-ragged]

Equal-length: --clips interleaved stereo clips x 441 000 sample frames (10 s at 44.1 kHz; 432 frames), Hamming 2048 / hop 1024, float32 masks
uniform in [0, 1], (B, 432, 1025) for both channels or (B, 432, 2, 1025), one per channel, everything device-resident (32 distinct noise clips
and masks repeated over the batch).  Timed with the plan's HIP-event stopwatch, median (min, max) of --reps readings after three warm-up
readings (as tools/maskfilter_complex_rates.py):
  shared / shared_rest            execute_masked_stereo with mask_channels 1 on a ZAFX_MASKFILTER / _REST plan of ZAFX_LAYOUT_TF
  per_channel / per_channel_rest  the same with mask_channels 2
  center / center_sides           (a) k_center on the same clips (ZAFX_CENTER / ZAFX_CENTER_SIDES): the same walk, masks computed instead of read
  planar_1 / planar_2 (+ _rest)   (b) TWO execute_masked launches (k_maskfilter, TF) in one reading on planar copies of the two channels, the same
                                  mask twice (planar_1, beside `shared`) or a mask each (planar_2, beside `per_channel`): a floor for what a
                                  caller assembles today -- the de-interleave in front and the re-interleave behind are not in it.
The ratios to (a) and (b) are reported, not barred.  Algorithmic bytes per sample frame: 8 in, 8 out (16 with the rest), 4 or 8 x 1025 / 1024 of
mask; fractions of HBM peak against 8 TB/s (MI355X).

Ragged: 1024 stereo clips of 5-15 s at 44.1 kHz (the recipe of tools/maskfilter_rates.py --ragged), for mask_channels 1 and 2, filtered and
filtered + rest:
  ragged    one execute_masked_stereo_ragged of the clips and masks packed back to back (the cutting of the units and the table's upload included)
  padded    the same clips padded with zeros to the longest, with masks of the longest's shape, as one execute_masked_stereo
  per_clip  one zafx_execute_masked_stereo per clip on the plan's stream, all 1024 in one reading

Verdicts by the project's rule for "faster": the median lies below the baseline's by more than the larger of the two (max - min) spreads.  Barred:
ragged against padded and against per_clip, per kind.  Exit status 0 either way; the verdicts are in the JSON.
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
    print(f"{name:28s} {r['median_ms']:8.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f})  {extra}  [{r.get('kernel', '')}]", flush=True)


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
    """`count` float32 at element `first` of a float32 DeviceBuffer (nothing to free)."""

    def __init__(self, buf, first, count):
        self.dtype = np.dtype(np.float32)
        self.ptr, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + 4 * first), 4 * count, (count,)


def equal_main(a, res):
    b, window = a.clips, zafx.hamming(W)
    noise = np.random.default_rng(1).standard_normal((DISTINCT, N, 2), dtype=np.float32)
    d_x = replicated(noise, b)
    d_l, d_r = replicated(np.ascontiguousarray(noise[:, :, 0]), b), replicated(np.ascontiguousarray(noise[:, :, 1]), b)
    probe = zafx.maskfilter_plan(window, layout="TF")
    rows, frames = probe.mask_dims(N)
    g = np.random.default_rng(2)
    d_m1 = replicated(g.random(probe.stereo_mask_shape(DISTINCT, N, 1), dtype=np.float32), b)
    d_m1b = replicated(g.random(probe.stereo_mask_shape(DISTINCT, N, 1), dtype=np.float32), b)
    d_m2 = replicated(g.random(probe.stereo_mask_shape(DISTINCT, N, 2), dtype=np.float32), b)
    for rest in (False, True):
        tag = "_rest" if rest else ""
        plan = zafx.maskfilter_plan(window, rest=rest, layout="TF")
        d_out = zafx.DeviceBuffer(plan.stereo_out_shape(b, N), np.float32)
        for name, mc, d_m in (("shared", 1, d_m1), ("per_channel", 2, d_m2)):
            r = timed(plan, lambda: plan.execute_masked_stereo(d_x, d_m, d_out, b, N, mc), a.reps)
            nbytes = 8 + (16 if rest else 8) + 4.0 * mc * rows * frames / N
            r.update(kernel=plan.last_kernel, msample_frames_per_s=b * N / (r["median_ms"] * 1e3), algorithmic_bytes_per_sample_frame=nbytes,
                     hbm_fraction=b * N * nbytes / (r["median_ms"] * 1e-3) / HBM_PEAK)
            res[name + tag] = r
            show(name + tag, r, f"{r['msample_frames_per_s']:9.0f} Msample frames/s  {r['hbm_fraction']:.3f} of HBM peak on {nbytes:.2f} B per sample frame")
        d_out.free()
        # (b) two mono launches on planar channels in one reading
        o_l, o_r = zafx.DeviceBuffer(plan.out_shape(b, N), np.float32), zafx.DeviceBuffer(plan.out_shape(b, N), np.float32)
        for name, m_r in (("planar_1", d_m1), ("planar_2", d_m1b)):
            def two():
                plan.execute_masked(d_l, d_m1, o_l, b, N)
                plan.execute_masked(d_r, m_r, o_r, b, N)
            r = timed(plan, two, a.reps)
            r["kernel"] = "2 x " + plan.last_kernel
            res[name + tag] = r
            show(name + tag, r, "two k_maskfilter launches on planar channels")
        o_l.free(), o_r.free()
        # (a) k_center on the same clips
        cplan = zafx.center_plan(window, sides=rest)
        c_out = zafx.DeviceBuffer(cplan.out_shape(b, N), np.float32)
        r = timed(cplan, lambda: cplan.execute(d_x, c_out, b, N), a.reps)
        r["kernel"] = cplan.last_kernel
        key = "center_sides" if rest else "center"
        res[key] = r
        show(key, r, "k_center on the same clips")
        c_out.free()
        for name, planar in (("shared", "planar_1"), ("per_channel", "planar_2")):
            res[f"{name}{tag}_over_center"] = res[name + tag]["median_ms"] / res[key]["median_ms"]
            res[f"{name}{tag}_over_planar"] = res[name + tag]["median_ms"] / res[planar + tag]["median_ms"]
            res[f"{name}{tag}_faster_than_planar"] = faster(res[name + tag], res[planar + tag])
            print(f"{name + tag}: / {key} = {res[f'{name}{tag}_over_center']:.3f}, / {planar + tag} = {res[f'{name}{tag}_over_planar']:.3f} "
                  f"({'faster' if res[f'{name}{tag}_faster_than_planar'] else 'not faster'} by the rule; reported, not barred)", flush=True)
    for buf in (d_x, d_l, d_r, d_m1, d_m1b, d_m2):
        buf.free()


def ragged_main(a, res):
    fs, clips = 44100, 1024
    lengths = np.random.default_rng(0).integers(5 * fs, 15 * fs + 1, clips).astype(np.int64)
    longest, total = int(lengths.max()), int(lengths.sum())
    in_offsets = np.zeros(clips, np.int64)
    in_offsets[1:] = np.cumsum(lengths)[:-1]
    window = zafx.hamming(W)
    res.update(ragged_clips=clips, ragged_sample_frames=total, longest=longest, padded_over_ragged_sample_frames=clips * longest / total)
    print(f"{clips} clips, {total} sample frames in all, longest {longest}: the padded batch holds {clips * longest / total:.3f} x as many", flush=True)
    small = zafx.DeviceBuffer.from_host(np.random.default_rng(1).standard_normal((DISTINCT, longest, 2), dtype=np.float32))
    d_rag = zafx.DeviceBuffer((total, 2), np.float32)
    d_pad = zafx.DeviceBuffer((clips, longest, 2), np.float32)
    d_pad.fill_zero()
    for i in range(clips):
        src, n = (i % DISTINCT) * longest * 8, int(lengths[i])
        d_rag.copy_from(small, nbytes=n * 8, dst_offset=int(in_offsets[i]) * 8, src_offset=src)
        d_pad.copy_from(small, nbytes=n * 8, dst_offset=i * longest * 8, src_offset=src)
    small.free()
    probe = zafx.maskfilter_plan(window, layout="TF")
    lib = _lib.load()
    for mc in (1, 2):
        mask_offsets, _ = probe.stereo_ragged_layout(lengths, mc)
        one_pad = int(np.prod(probe.stereo_mask_shape(1, longest, mc)))
        d_noise = zafx.DeviceBuffer.from_host(np.random.default_rng(2).random((DISTINCT, one_pad), dtype=np.float32))
        m_rag, m_pad = zafx.DeviceBuffer((int(mask_offsets[-1]),), np.float32), zafx.DeviceBuffer((clips, one_pad), np.float32)
        for i in range(clips):
            src = (i % DISTINCT) * one_pad * 4
            m_rag.copy_from(d_noise, nbytes=int(mask_offsets[i + 1] - mask_offsets[i]) * 4, dst_offset=int(mask_offsets[i]) * 4, src_offset=src)
            m_pad.copy_from(d_noise, nbytes=one_pad * 4, dst_offset=i * one_pad * 4, src_offset=src)
        d_noise.free()
        for rest in (False, True):
            name = f"ragged_{mc}" + ("_rest" if rest else "")
            plan = zafx.maskfilter_plan(window, rest=rest, layout="TF")
            blocks = 2 if rest else 1
            out = zafx.DeviceBuffer((blocks * total, 2), np.float32)
            out_offsets = blocks * in_offsets
            r = {}
            r["ragged"] = timed(plan, lambda: plan.execute_masked_stereo_ragged(d_rag, in_offsets, lengths, m_rag, mask_offsets, out, out_offsets, mc), a.reps)
            r["ragged"]["kernel"] = plan.last_kernel
            views = [(View(d_rag, 2 * int(o), 2 * int(n)), View(m_rag, int(mo), int(me - mo)), View(out, 2 * int(blocks * o), 2 * int(blocks * n)), int(n))
                     for o, n, mo, me in zip(in_offsets, lengths, mask_offsets[:-1], mask_offsets[1:])]

            def per_clip():   # (the library's entry point itself: the Python method's checks cost more than the launch)
                for v_in, v_mask, v_out, n in views:
                    _lib.check(lib.zafx_execute_masked_stereo(plan.handle, v_in.ptr, v_mask.ptr, v_out.ptr, 1, n, mc), "zafx_execute_masked_stereo")
            r["per_clip"] = timed(plan, per_clip, a.reps, warm=1)
            r["per_clip"]["kernel"] = plan.last_kernel
            out.free()
            out = zafx.DeviceBuffer(plan.stereo_out_shape(clips, longest), np.float32)
            r["padded"] = timed(plan, lambda: plan.execute_masked_stereo(d_pad, m_pad, out, clips, longest, mc), a.reps)
            r["padded"]["kernel"] = plan.last_kernel
            out.free()
            for key, v in r.items():
                v["msample_frames_per_s"] = total / (v["median_ms"] * 1e3)
                show(f"{name} {key}", v, f"{v['msample_frames_per_s']:9.0f} Msample frames/s")
            r["ragged_over_padded"] = r["ragged"]["median_ms"] / r["padded"]["median_ms"]
            r["per_clip_over_ragged"] = r["per_clip"]["median_ms"] / r["ragged"]["median_ms"]
            r["faster_than_padded"], r["faster_than_per_clip"] = faster(r["ragged"], r["padded"]), faster(r["ragged"], r["per_clip"])
            print(f"{name}: ragged / padded {r['ragged_over_padded']:.3f} ({'MET' if r['faster_than_padded'] else 'MISSED'}), per clip / ragged "
                  f"{r['per_clip_over_ragged']:.2f} ({'MET' if r['faster_than_per_clip'] else 'MISSED'})", flush=True)
            res[name] = r
        m_rag.free(), m_pad.free()
    d_rag.free(), d_pad.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-equal", action="store_true")
    ap.add_argument("--no-ragged", action="store_true")
    a = ap.parse_args()
    res = {"device": zafx.device_name(0), "clips": a.clips, "sample_frames": N, "window": W, "hop": HOP, "reps": a.reps}
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
