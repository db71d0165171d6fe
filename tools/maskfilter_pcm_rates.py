"""Rates of the mask filter on 16-bit PCM (k_maskfilter_pcm, k_maskfilter_stereo_pcm and their ragged forms) beside the float kernels and beside
what a PCM caller had without them, in one process.

    python tools/maskfilter_pcm_rates.py [--clips 1024] [--reps 30] [--out FILE] [--no-equal] [--no-ragged]

Equal-length: --clips clips x 441 000 sample frames (10 s at 44.1 kHz; 432 frames), Hamming 2048 / hop 1024, int16 noise in +-20000, float32 "TF"
masks uniform in [0, 1], everything device-resident (32 distinct clips and masks repeated over the batch).  Timed with the plan's HIP-event
stopwatch, median (min, max) of --reps readings after three warm-up readings (as tools/maskfilter_stereo_rates.py).  Per form -- mono, stereo
under one mask (stereo_1), stereo under a mask per channel (stereo_2) --, filtered and + rest:
  <form>[_rest]_i16   execute_masked_pcm, int16 in, int16 out
  <form>[_rest]_f32   execute_masked_pcm, int16 in, float32 out
  <form>[_rest]_float the unchanged float kernel (execute_masked on a "TF" plan / execute_masked_stereo) on the same clips as float32 = int16 / 32768
  mono[_rest]_convert zafx_pcm_to_float followed by execute_masked in one reading: what a mono PCM caller had (for stereo there was no device
                      path: zafx_pcm_to_float averages the channels)
Targets: <form>_i16 takes no longer than <form>_float (it moves fewer bytes and adds only conversions): met when the float kernel is not faster
by the project's rule; mono_f32 is faster than mono_convert by that rule.  The rule: a's median lies below b's by more than the larger of the
two (max - min) spreads.  Algorithmic bytes per sample frame and fractions of HBM peak (8 TB/s, MI355X) are reported with each.

Ragged: 1024 clips of 5-15 s at 44.1 kHz (the recipe of tools/maskfilter_rates.py --ragged), per form, filtered and + rest, int16 out:
  ragged_i16    one execute_masked_pcm_ragged of the clips and masks packed back to back (the cut of the units and the table's upload included)
  ragged_float  the float kernel's ragged launch on the same clips as float32
  padded_i16    the same clips padded with zeros to the longest, with masks of the longest's shape, as one execute_masked_pcm
Exit status 0 either way; the verdicts are in the JSON.
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
FORMS = (("mono", 1, 1), ("stereo_1", 2, 1), ("stereo_2", 2, 2))


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


def pcm_noise(shape):
    return np.random.default_rng(1).integers(-20000, 20001, shape).astype(np.int16)


def mask_and_out_shapes(plan, b, n, ch, mc):
    if ch == 1:
        return plan.mask_shape(b, n), plan.out_shape(b, n)
    return plan.stereo_mask_shape(b, n, mc), plan.stereo_out_shape(b, n)


def float_launch(plan, ch, mc, d_x, d_m, d_out, b, n):
    if ch == 1:
        return lambda: plan.execute_masked(d_x, d_m, d_out, b, n)
    return lambda: plan.execute_masked_stereo(d_x, d_m, d_out, b, n, mc)


def rate(r, plan, frames_total, nbytes):
    r.update(kernel=plan.last_kernel, msample_frames_per_s=frames_total / (r["median_ms"] * 1e3), algorithmic_bytes_per_sample_frame=nbytes,
             hbm_fraction=frames_total * nbytes / (r["median_ms"] * 1e-3) / HBM_PEAK)
    return r


def equal_main(a, res):
    b, window = a.clips, zafx.hamming(W)
    probe = zafx.maskfilter_plan(window, layout="TF")
    rows, frames = probe.mask_dims(N)
    for form, ch, mc in FORMS:
        pcm = pcm_noise((DISTINCT, N) + ((2,) if ch == 2 else ()))
        d_pcm, d_flt = replicated(pcm, b), replicated(pcm.astype(np.float32) / np.float32(32768), b)
        d_m = replicated(np.random.default_rng(2).random(mask_and_out_shapes(probe, DISTINCT, N, ch, mc)[0], dtype=np.float32), b)
        mask_bytes = 4.0 * mc * rows * frames / N
        for rest in (False, True):
            tag = form + ("_rest" if rest else "")
            plan = zafx.maskfilter_plan(window, rest=rest, layout="TF")
            shape = mask_and_out_shapes(plan, b, N, ch, mc)[1]
            blocks = 2 if rest else 1
            for suffix, dt, d_in in (("i16", np.int16, d_pcm), ("f32", np.float32, d_pcm), ("float", np.float32, d_flt)):
                d_out = zafx.DeviceBuffer(shape, dt)
                if suffix == "float":
                    launch = float_launch(plan, ch, mc, d_in, d_m, d_out, b, N)
                else:
                    launch = lambda: plan.execute_masked_pcm(d_in, d_m, d_out, b, N, ch, mc)   # noqa: E731
                nbytes = ch * ((4 if suffix == "float" else 2) + blocks * np.dtype(dt).itemsize) + mask_bytes
                r = rate(timed(plan, launch, a.reps), plan, b * N, nbytes)
                res[f"{tag}_{suffix}"] = r
                show(f"{tag}_{suffix}", r, f"{r['msample_frames_per_s']:9.0f} Msample frames/s  {r['hbm_fraction']:.3f} of HBM peak on {nbytes:.2f} B per sample frame")
                if ch == 1 and suffix == "float":   # what a mono PCM caller had: convert, then filter
                    d_stage = zafx.DeviceBuffer((b, N), np.float32)

                    def convert_then_filter():
                        plan.pcm_to_float(d_pcm, d_stage, b, N, 1)
                        plan.execute_masked(d_stage, d_m, d_out, b, N)
                    r = timed(plan, convert_then_filter, a.reps)
                    r["kernel"] = "zafx_pcm_to_float + " + plan.last_kernel
                    res[f"{tag}_convert"] = r
                    show(f"{tag}_convert", r, "zafx_pcm_to_float, then the float kernel")
                    d_stage.free()
                d_out.free()
            i16, f32, flt = res[f"{tag}_i16"], res[f"{tag}_f32"], res[f"{tag}_float"]
            v = {"i16_over_float": i16["median_ms"] / flt["median_ms"], "f32_over_float": f32["median_ms"] / flt["median_ms"],
                 "i16_faster_than_float": faster(i16, flt), "float_faster_than_i16": faster(flt, i16), "f32_faster_than_float": faster(f32, flt),
                 "float_faster_than_f32": faster(flt, f32)}
            v["target_i16_no_longer_than_float"] = "MISSED" if v["float_faster_than_i16"] else "MET"
            line = f"{tag}: i16 / float {v['i16_over_float']:.3f} (target {v['target_i16_no_longer_than_float']}), f32 / float {v['f32_over_float']:.3f}"
            if ch == 1:
                conv = res[f"{tag}_convert"]
                v["f32_over_convert"], v["i16_over_convert"] = f32["median_ms"] / conv["median_ms"], i16["median_ms"] / conv["median_ms"]
                v["target_f32_faster_than_convert"] = "MET" if faster(f32, conv) else "MISSED"
                line += f", f32 / convert-then-filter {v['f32_over_convert']:.3f} (target {v['target_f32_faster_than_convert']}), i16 / convert-then-filter {v['i16_over_convert']:.3f}"
            res[f"{tag}_verdicts"] = v
            print(line, flush=True)
        for buf in (d_pcm, d_flt, d_m):
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
    probe = zafx.maskfilter_plan(window, layout="TF")
    for form, ch, mc in FORMS:
        tail = (2,) if ch == 2 else ()
        pcm = pcm_noise((DISTINCT, longest) + tail)
        small, small_f = zafx.DeviceBuffer.from_host(pcm), zafx.DeviceBuffer.from_host(pcm.astype(np.float32) / np.float32(32768))
        d_rag, d_rag_f = zafx.DeviceBuffer((total,) + tail, np.int16), zafx.DeviceBuffer((total,) + tail, np.float32)
        d_pad = zafx.DeviceBuffer((clips, longest) + tail, np.int16)
        d_pad.fill_zero()
        for i in range(clips):
            src, n = (i % DISTINCT) * longest, int(lengths[i])
            d_rag.copy_from(small, nbytes=n * 2 * ch, dst_offset=int(in_offsets[i]) * 2 * ch, src_offset=src * 2 * ch)
            d_rag_f.copy_from(small_f, nbytes=n * 4 * ch, dst_offset=int(in_offsets[i]) * 4 * ch, src_offset=src * 4 * ch)
            d_pad.copy_from(small, nbytes=n * 2 * ch, dst_offset=i * longest * 2 * ch, src_offset=src * 2 * ch)
        small.free(), small_f.free()
        mask_offsets = probe.mask_ragged_layout(lengths) if ch == 1 else probe.stereo_ragged_layout(lengths, mc)[0]
        one_pad = int(np.prod(mask_and_out_shapes(probe, 1, longest, ch, mc)[0]))
        d_noise = zafx.DeviceBuffer.from_host(np.random.default_rng(2).random((DISTINCT, one_pad), dtype=np.float32))
        m_rag, m_pad = zafx.DeviceBuffer((int(mask_offsets[-1]),), np.float32), zafx.DeviceBuffer((clips, one_pad), np.float32)
        for i in range(clips):
            src = (i % DISTINCT) * one_pad * 4
            m_rag.copy_from(d_noise, nbytes=int(mask_offsets[i + 1] - mask_offsets[i]) * 4, dst_offset=int(mask_offsets[i]) * 4, src_offset=src)
            m_pad.copy_from(d_noise, nbytes=one_pad * 4, dst_offset=i * one_pad * 4, src_offset=src)
        d_noise.free()
        for rest in (False, True):
            name = f"ragged_{form}" + ("_rest" if rest else "")
            plan = zafx.maskfilter_plan(window, rest=rest, layout="TF")
            blocks = 2 if rest else 1
            out_offsets = blocks * in_offsets
            r = {}
            out = zafx.DeviceBuffer((blocks * total,) + tail, np.int16)
            r["ragged_i16"] = timed(plan, lambda: plan.execute_masked_pcm_ragged(d_rag, in_offsets, lengths, m_rag, mask_offsets, out, out_offsets, ch, mc), a.reps)
            r["ragged_i16"]["kernel"] = plan.last_kernel
            out.free()
            out = zafx.DeviceBuffer((blocks * total,) + tail, np.float32)
            if ch == 1:
                launch = lambda: plan.execute_masked_ragged(d_rag_f, in_offsets, lengths, m_rag, mask_offsets, out, out_offsets)   # noqa: E731
            else:
                launch = lambda: plan.execute_masked_stereo_ragged(d_rag_f, in_offsets, lengths, m_rag, mask_offsets, out, out_offsets, mc)   # noqa: E731
            r["ragged_float"] = timed(plan, launch, a.reps)
            r["ragged_float"]["kernel"] = plan.last_kernel
            out.free()
            out = zafx.DeviceBuffer(mask_and_out_shapes(plan, clips, longest, ch, mc)[1], np.int16)
            r["padded_i16"] = timed(plan, lambda: plan.execute_masked_pcm(d_pad, m_pad, out, clips, longest, ch, mc), a.reps)
            r["padded_i16"]["kernel"] = plan.last_kernel
            out.free()
            for key in ("ragged_i16", "ragged_float", "padded_i16"):
                r[key]["msample_frames_per_s"] = total / (r[key]["median_ms"] * 1e3)
                show(f"{name} {key}", r[key], f"{r[key]['msample_frames_per_s']:9.0f} Msample frames/s")
            r["i16_over_float"] = r["ragged_i16"]["median_ms"] / r["ragged_float"]["median_ms"]
            r["ragged_over_padded"] = r["ragged_i16"]["median_ms"] / r["padded_i16"]["median_ms"]
            r["float_faster_than_i16"], r["i16_faster_than_float"] = faster(r["ragged_float"], r["ragged_i16"]), faster(r["ragged_i16"], r["ragged_float"])
            r["target_i16_no_longer_than_float"] = "MISSED" if r["float_faster_than_i16"] else "MET"
            r["faster_than_padded"] = faster(r["ragged_i16"], r["padded_i16"])
            print(f"{name}: i16 / float {r['i16_over_float']:.3f} (target {r['target_i16_no_longer_than_float']}), ragged / padded {r['ragged_over_padded']:.3f} "
                  f"({'faster' if r['faster_than_padded'] else 'not faster'} by the rule)", flush=True)
            res[name] = r
        for buf in (d_rag, d_rag_f, d_pad, m_rag, m_pad):
            buf.free()


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
