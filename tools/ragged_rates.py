"""Rates of ragged batches (zafx_execute_ragged) against the padded batch and an equal-length batch, in one process.

    python tools/ragged_rates.py [--reps 30] [--out FILE] [--kinds stft,mel,mfcc,mel+mfcc,mdct,mdct_any,imdct,istft,mel_pcm,mfcc_pcm,stft_pcm,mdct_pcm,stft64,mdct64,mel64,mfcc64]
                                 [--imdct-k 2,4,8,12,16,24]
                                 [--istft-k 2,4,8,12,16,24]

Batch: 1024 clips, lengths uniform in 5-15 s at 44.1 kHz (even, so that the aligned loads apply as they do for the equal-length batch),
window 2048, hop 1024.  For the STFT (two-sided, the headline's kind), mel (128 filters), mfcc (20 coefficients) and the one-pass mel + mfcc:
  ragged   one execute_ragged of the 1024 clips (the table's upload included)
  padded   the same clips padded to the longest as one execute
  equal    1024 clips of 10 s as one execute
each timed with the plan's HIP-event stopwatch, one launch per reading, median (min, max) of --reps readings after warm-up.  All outputs are
DeviceBuffers (zafx_alloc) with rows on the 128-byte line grid, so placement treats the three alike; Msamples/s counts the clips' own samples.

The `mdct` row: the same 1024 clips with lengths rounded down to multiples of 4 (the 16-byte loads of k_mdct_ft32), Kaiser-Bessel-derived
window of 2048 samples, rows padded to whole lines; `mdct_any`: those lengths plus 0 ... 3 samples each (the 4-byte loads).  Next to ragged and padded it times `per_clip`: the same execute_ragged with
ZAFX_RAGGED_MDCT_NATIVE=0 in the environment, which keeps the batch on one zafx_execute per clip -- what every MDCT batch ran before the
RAGGED form of the kernel existed.

The `imdct` row (not in the default kinds): the (1024, T_i) coefficient blocks of those clips, T_i = ceil(N_i / 1024) + 1, rows padded to
whole lines, as the ragged MDCT leaves them.  `ragged`: one execute_imdct_ragged, cutting and table upload included (k_imdct_ragged);
`padded`: every block padded to the longest as one execute (k_imdct); `per_clip`: the same execute_imdct_ragged with
ZAFX_RAGGED_IMDCT_NATIVE=0, one zafx_execute per block -- the only way before the RAGGED form existed.  --imdct-k: the ragged reading again
for these units per workgroup slot of the cutting rule (ZAFX_IMDCT_UNITS_PER_SLOT), the sweep the shipped constant was chosen from.

The `istft` rows (not in the default kinds; `istft`: two-sided, `istft_onesided`: rows 0 ... W/2): the spectra of those clips, Hamming 2048 / hop
1024, rows padded to whole lines -- written on the device by the ragged STFT (and by the STFT of the padded batch), as a caller who edits spectra
has them.  `ragged`: one execute_istft_ragged, cutting and table upload included (k_istft_ragged); `padded`: every spectrum padded to the
longest as one execute (k_istft_ft16); `per_clip`: the same execute_istft_ragged with ZAFX_RAGGED_ISTFT_NATIVE=0, one zafx_execute per
spectrum.  The three are read in turn, one launch of each per round, --reps rounds after three warm-up rounds (every shape and route warmed),
median (min, max).  --istft-k: the ragged reading again for these units per workgroup slot (ZAFX_ISTFT_UNITS_PER_SLOT).  With `istft` among
the kinds the tool exits with status 1 unless the one launch is faster than both alternatives for both spectrum kinds.

The `mel_pcm`, `mfcc_pcm`, `stft_pcm` (two-sided) and `mdct_pcm` rows (not in the default kinds): the same 1024 clips as int16 mono that is
already on the device, clip starts on multiples of 64 sample frames (`mdct_pcm`: lengths rounded down to multiples of 4).  `native`: one
execute_ragged_pcm, the integers in the kernel's own loads; `convert_first`: the same call with ZAFX_RAGGED_PCM_NATIVE=0 in the environment --
k_pcm_to_float over the packed array into the plan's staging (in groups under the scratch budget: two at this size), then execute_ragged, what
the library's primitives amounted to before the RAGGED x PCM forms; `padded`: execute_pcm on the clips padded to the longest.  Whole-call
times, the three read in turn, one launch of each per round, --reps rounds after three warm-up rounds, median (min, max).  With one of these
among the kinds the tool exits with status 1 unless `native`'s median is below both alternatives' for every such kind (margin zero: the native
launch moves strictly fewer bytes and is one launch fewer).

The `stft64` (two-sided), `mdct64`, `mel64` and `mfcc64` rows (not in the default kinds): the same 1024 clips as float64, float64 plans on
whole-line rows (Hamming 2048 / hop 1024, KBD 2048 for the MDCT, 128 filters, 20 coefficients).  `ragged`: one execute_ragged, table
upload included (k_stft_ft8_f64_ragged, k_mdct_ft16_f64_ragged, k_mel_ft8_f64_ragged); `padded`: the clips padded to the longest as one
execute of the equal-length tiled kernel; `per_clip`: the same execute_ragged with ZAFX_RAGGED_F64_NATIVE=0, one zafx_execute per clip --
what every float64 batch ran before the RAGGED forms existed.  The three are read in turn, one launch of each per round, --reps rounds
after three warm-up rounds, median (min, max); a kind's outputs are freed before the next kind's are allocated (the padded two-sided
complex128 STFT alone is about 22 GB).  With one of these among the kinds the tool exits with status 1 unless `ragged`'s median is below
both alternatives' for every such kind (margin zero: the one launch moves strictly fewer bytes than the padded one and is about 1000
launches fewer than the per-clip route).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zaf-python_amd"))
import zafx  # noqa: E402

FS, W, HOP, CLIPS = 44100, 2048, 1024, 1024


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


def inputs(lengths):
    """The three input arrays, filled once with noise and shared by every kind: the packed ragged batch, the padded batch, the 10 s batch."""
    rng = np.random.default_rng(1)
    in_offsets = np.zeros(len(lengths), np.int64)
    slots = (lengths + 31) // 32 * 32
    in_offsets[1:] = np.cumsum(slots)[:-1]
    bufs = {}
    for key, shape in (("ragged", (int(slots.sum()),)), ("padded", (CLIPS, int(lengths.max()))), ("equal", (CLIPS, 10 * FS))):
        bufs[key] = zafx.DeviceBuffer(shape, np.float32)
        bufs[key].upload(rng.standard_normal(shape, dtype=np.float32))   # (the ragged gaps hold noise too: the kernels never read them)
    return in_offsets, bufs


def measure(name, plan, lengths, in_offsets, bufs, reps):
    offs, frames, pitch = plan.ragged_layout(lengths)
    out = zafx.DeviceBuffer((int(offs[-1]),), plan.out_dtype)
    res = {}
    res["ragged"] = timed(plan, lambda: plan.execute_ragged(bufs["ragged"], in_offsets, lengths, out), reps)
    res["ragged_kernel"] = plan.last_kernel
    out.free()
    for key, n in (("padded", int(lengths.max())), ("equal", 10 * FS)):
        o = zafx.DeviceBuffer(plan.out_shape(CLIPS, n), plan.out_dtype)
        res[key] = timed(plan, lambda: plan.execute(bufs[key], o, CLIPS, n), reps)
        res[key + "_kernel"] = plan.last_kernel
        o.free()
    samples = {"ragged": int(lengths.sum()), "padded": int(lengths.sum()), "equal": CLIPS * 10 * FS}
    for key in ("ragged", "padded", "equal"):
        res[key]["msamples_per_s"] = samples[key] / (res[key]["median_ms"] * 1e3)
    res["ragged_over_padded"] = res["ragged"]["median_ms"] / res["padded"]["median_ms"]
    res["ragged_rate_over_equal_rate"] = res["ragged"]["msamples_per_s"] / res["equal"]["msamples_per_s"]
    r, p, e = res["ragged"], res["padded"], res["equal"]
    print(f"{name:9s} ragged {r['median_ms']:7.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f}) {r['msamples_per_s']:8.0f} Ms/s [{res['ragged_kernel']}] | "
          f"padded {p['median_ms']:7.3f} ms ({p['min_ms']:.3f}-{p['max_ms']:.3f}) [{res['padded_kernel']}] | equal {e['median_ms']:7.3f} ms "
          f"({e['min_ms']:.3f}-{e['max_ms']:.3f}) {e['msamples_per_s']:8.0f} Ms/s [{res['equal_kernel']}] | ragged / padded "
          f"{res['ragged_over_padded']:.3f}, rate ragged / equal {res['ragged_rate_over_equal_rate']:.3f}", flush=True)
    return res


def measure_mdct(name, lengths, reps):
    """ragged / padded / per-clip of the MDCT on one plan, with input arrays of its own: lengths that are multiples of 4 ("mdct": 16-byte
    loads), or ("mdct_any") the same lengths plus 0 ... 3 samples each, seeded: 4-byte loads, the ordinary case of real audio."""
    lengths = lengths - lengths % 4
    if name == "mdct_any":
        lengths = lengths + np.random.default_rng(2).integers(0, 4, len(lengths))
        lengths[np.argmax(lengths)] |= 1   # (the padded batch off the 16-byte form as well)
    plan = zafx.mdct_plan(zafx.kaiser_bessel_derived(W), row_align=32)
    rng = np.random.default_rng(1)
    slots = (lengths + 31) // 32 * 32
    in_offsets = np.zeros(len(lengths), np.int64)
    in_offsets[1:] = np.cumsum(slots)[:-1]
    nmax = int(lengths.max())
    packed = zafx.DeviceBuffer((int(slots.sum()),), np.float32)
    packed.upload(rng.standard_normal(packed.shape, dtype=np.float32))
    offs, frames, pitch = plan.ragged_layout(lengths)
    out = zafx.DeviceBuffer((int(offs[-1]),), plan.out_dtype)
    res = {"samples": int(lengths.sum()), "longest": nmax}
    res["ragged"] = timed(plan, lambda: plan.execute_ragged(packed, in_offsets, lengths, out), reps)
    res["ragged_kernel"] = plan.last_kernel
    os.environ["ZAFX_RAGGED_MDCT_NATIVE"] = "0"
    try:
        res["per_clip"] = timed(plan, lambda: plan.execute_ragged(packed, in_offsets, lengths, out), reps)
        res["per_clip_kernel"] = plan.last_kernel
    finally:
        del os.environ["ZAFX_RAGGED_MDCT_NATIVE"]
    out.free()
    packed.free()
    padded = zafx.DeviceBuffer((CLIPS, nmax), np.float32)
    padded.upload(rng.standard_normal(padded.shape, dtype=np.float32))
    o = zafx.DeviceBuffer(plan.out_shape(CLIPS, nmax), plan.out_dtype)
    res["padded"] = timed(plan, lambda: plan.execute(padded, o, CLIPS, nmax), reps)
    res["padded_kernel"] = plan.last_kernel
    o.free()
    padded.free()
    for key in ("ragged", "padded", "per_clip"):
        res[key]["msamples_per_s"] = res["samples"] / (res[key]["median_ms"] * 1e3)
    res["ragged_over_padded"] = res["ragged"]["median_ms"] / res["padded"]["median_ms"]
    res["per_clip_over_ragged"] = res["per_clip"]["median_ms"] / res["ragged"]["median_ms"]
    r, p, c = res["ragged"], res["padded"], res["per_clip"]
    print(f"{name:9s} ragged {r['median_ms']:7.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f}) {r['msamples_per_s']:8.0f} Ms/s [{res['ragged_kernel']}] | "
          f"padded {p['median_ms']:7.3f} ms ({p['min_ms']:.3f}-{p['max_ms']:.3f}) [{res['padded_kernel']}] | per clip {c['median_ms']:7.3f} ms "
          f"({c['min_ms']:.3f}-{c['max_ms']:.3f}) [{res['per_clip_kernel']}] | ragged / padded {res['ragged_over_padded']:.3f}, "
          f"per clip / ragged {res['per_clip_over_ragged']:.1f}", flush=True)
    return res


def measure_imdct(lengths, reps, sweep):
    """ragged / padded / per-clip of the IMDCT on one plan: noise coefficients (the pad columns included -- they are never used)."""
    m = W // 2
    plan = zafx.mdct_plan(zafx.kaiser_bessel_derived(W), inverse=True, row_align=32)
    frames = -(-lengths // m) + 1
    pitch = (frames + 31) // 32 * 32
    in_offsets = np.zeros(len(frames), np.int64)
    in_offsets[1:] = np.cumsum(m * pitch)[:-1]
    out_len = m * (frames - 1) - 1
    out_offsets = np.zeros(len(frames), np.int64)
    out_offsets[1:] = np.cumsum((out_len + 31) // 32 * 32)[:-1]
    rng = np.random.default_rng(1)
    tmax = int(frames.max())
    coefs = zafx.DeviceBuffer((int((m * pitch).sum()),), np.float32)
    coefs.upload(rng.standard_normal(coefs.shape, dtype=np.float32))
    out = zafx.DeviceBuffer((int(out_offsets[-1] + out_len[-1]) + 32,), np.float32)
    res = {"samples": int(out_len.sum()), "frames": int(frames.sum()), "longest_frames": tmax}
    call = lambda: plan.execute_imdct_ragged(coefs, in_offsets, frames, out, out_offsets)   # noqa: E731
    res["ragged"] = timed(plan, call, reps)
    res["ragged_kernel"] = plan.last_kernel
    res["units_per_slot_sweep"] = {}
    for k in sweep:
        os.environ["ZAFX_IMDCT_UNITS_PER_SLOT"] = str(k)
        try:
            res["units_per_slot_sweep"][str(k)] = timed(plan, call, reps)
        finally:
            del os.environ["ZAFX_IMDCT_UNITS_PER_SLOT"]
    os.environ["ZAFX_RAGGED_IMDCT_NATIVE"] = "0"
    try:
        res["per_clip"] = timed(plan, call, reps)
        res["per_clip_kernel"] = plan.last_kernel
    finally:
        del os.environ["ZAFX_RAGGED_IMDCT_NATIVE"]
    out.free()
    coefs.free()
    padded = zafx.DeviceBuffer((CLIPS, m, plan.row_pitch(tmax)), np.float32)
    padded.upload(rng.standard_normal(padded.shape, dtype=np.float32))
    o = zafx.DeviceBuffer(plan.out_shape(CLIPS, tmax), plan.out_dtype)
    res["padded"] = timed(plan, lambda: plan.execute(padded, o, CLIPS, tmax), reps)
    res["padded_kernel"] = plan.last_kernel
    o.free()
    padded.free()
    for key in ("ragged", "padded", "per_clip"):
        res[key]["msamples_per_s"] = res["samples"] / (res[key]["median_ms"] * 1e3)
    res["ragged_over_padded"] = res["ragged"]["median_ms"] / res["padded"]["median_ms"]
    res["per_clip_over_ragged"] = res["per_clip"]["median_ms"] / res["ragged"]["median_ms"]
    r, p, c = res["ragged"], res["padded"], res["per_clip"]
    print(f"imdct     ragged {r['median_ms']:7.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f}) {r['msamples_per_s']:8.0f} Ms/s [{res['ragged_kernel']}] | "
          f"padded {p['median_ms']:7.3f} ms ({p['min_ms']:.3f}-{p['max_ms']:.3f}) [{res['padded_kernel']}] | per clip {c['median_ms']:7.3f} ms "
          f"({c['min_ms']:.3f}-{c['max_ms']:.3f}) [{res['per_clip_kernel']}] | ragged / padded {res['ragged_over_padded']:.3f}, "
          f"per clip / ragged {res['per_clip_over_ragged']:.1f}", flush=True)
    for k, t in res["units_per_slot_sweep"].items():
        print(f"imdct     units per slot {k:>3s}: ragged {t['median_ms']:7.3f} ms ({t['min_ms']:.3f}-{t['max_ms']:.3f})", flush=True)
    return res


def timed_in_turn(plan, launches, reps, warm=3):
    """The launches (name -> callable) read in turn, one of each per round: what shares the device disturbs them alike."""
    ms = {k: [] for k in launches}
    for r in range(warm + reps):
        for k, launch in launches.items():
            plan.timer_start()
            launch()
            t = plan.timer_stop()
            if r >= warm:
                ms[k].append(t)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for k, v in ms.items()}


def with_env(name, value, call):
    def run():
        os.environ[name] = value
        try:
            call()
        finally:
            del os.environ[name]
    return run


def measure_istft(name, onesided, lengths, reps, sweep):
    """ragged / padded / per-clip of the ISTFT on one plan.  The spectra are made on the device: the ragged STFT of noise clips writes the
    blocks where the ragged ISTFT reads them, the STFT of the clips padded to the longest writes the padded batch."""
    window = zafx.hamming(W)
    fwd = zafx.stft_plan(window, HOP, onesided=onesided, row_align=16)
    plan = zafx.istft_plan(window, HOP, onesided=onesided, row_align=16)
    rows = W // 2 + 1 if onesided else W
    rng = np.random.default_rng(1)
    slots = (lengths + 31) // 32 * 32
    clip_offsets = np.zeros(len(lengths), np.int64)
    clip_offsets[1:] = np.cumsum(slots)[:-1]
    clips = zafx.DeviceBuffer((int(slots.sum()),), np.float32)
    clips.upload(rng.standard_normal(clips.shape, dtype=np.float32))
    offs, frames, pitch = fwd.ragged_layout(lengths)
    in_offsets = np.ascontiguousarray(offs[:-1], dtype=np.int64)
    assert all(plan.row_pitch(int(t)) == int(p) for t, p in zip(frames[:8], pitch[:8]))
    spec = zafx.DeviceBuffer((int(offs[-1]),), np.complex64)
    fwd.execute_ragged(clips, clip_offsets, lengths, spec)
    fwd.sync()
    clips.free()
    out_len = np.maximum(frames * HOP - (W - HOP), 0)
    out_offsets = np.zeros(len(frames), np.int64)
    out_offsets[1:] = np.cumsum((out_len + 31) // 32 * 32)[:-1]
    out = zafx.DeviceBuffer((int(out_offsets[-1] + out_len[-1]) + 32,), np.float32)
    nmax, tmax = int(lengths.max()), int(frames.max())
    padded_clips = zafx.DeviceBuffer((CLIPS, nmax), np.float32)
    padded_clips.upload(rng.standard_normal(padded_clips.shape, dtype=np.float32))
    padded = zafx.DeviceBuffer((CLIPS, rows, plan.row_pitch(tmax)), np.complex64)
    fwd.execute(padded_clips, padded, CLIPS, nmax)
    fwd.sync()
    padded_clips.free()
    o = zafx.DeviceBuffer(plan.out_shape(CLIPS, tmax), plan.out_dtype)
    res = {"samples": int(out_len.sum()), "frames": int(frames.sum()), "longest_frames": tmax, "spectrum_rows": rows}
    call = lambda: plan.execute_istft_ragged(spec, in_offsets, frames, out, out_offsets)   # noqa: E731
    kernels = {}

    def noting(key, launch):
        def run():
            launch()
            kernels[key] = plan.last_kernel
        return run
    launches = {"ragged": noting("ragged", call), "padded": noting("padded", lambda: plan.execute(padded, o, CLIPS, tmax)),
                "per_clip": noting("per_clip", with_env("ZAFX_RAGGED_ISTFT_NATIVE", "0", call))}
    res.update(timed_in_turn(plan, launches, reps))
    for key in launches:
        res[key + "_kernel"] = kernels[key]
    if sweep:
        res["units_per_slot_sweep"] = timed_in_turn(plan, {str(k): with_env("ZAFX_ISTFT_UNITS_PER_SLOT", str(k), call) for k in sweep}, reps)
    for b in (spec, out, padded, o):
        b.free()
    for key in ("ragged", "padded", "per_clip"):
        res[key]["msamples_per_s"] = res["samples"] / (res[key]["median_ms"] * 1e3)
    res["ragged_over_padded"] = res["ragged"]["median_ms"] / res["padded"]["median_ms"]
    res["per_clip_over_ragged"] = res["per_clip"]["median_ms"] / res["ragged"]["median_ms"]
    res["ragged_is_fastest"] = bool(res["ragged"]["median_ms"] < min(res["padded"]["median_ms"], res["per_clip"]["median_ms"]))
    r, p, c = res["ragged"], res["padded"], res["per_clip"]
    print(f"{name:9s} ragged {r['median_ms']:7.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f}) {r['msamples_per_s']:8.0f} Ms/s [{res['ragged_kernel']}] | "
          f"padded {p['median_ms']:7.3f} ms ({p['min_ms']:.3f}-{p['max_ms']:.3f}) [{res['padded_kernel']}] | per clip {c['median_ms']:7.3f} ms "
          f"({c['min_ms']:.3f}-{c['max_ms']:.3f}) [{res['per_clip_kernel']}] | ragged / padded {res['ragged_over_padded']:.3f}, "
          f"per clip / ragged {res['per_clip_over_ragged']:.1f}", flush=True)
    for k, t in res.get("units_per_slot_sweep", {}).items():
        print(f"{name:9s} units per slot {k:>3s}: ragged {t['median_ms']:7.3f} ms ({t['min_ms']:.3f}-{t['max_ms']:.3f})", flush=True)
    return res


PCM_KINDS = ("mel_pcm", "mfcc_pcm", "stft_pcm", "mdct_pcm")


def measure_pcm(name, plan, lengths, reps):
    """native / convert-first / padded of one kind on int16 mono that is already on the device (zafx_execute_ragged_pcm).  The gaps of the packed
    array and the padding of the padded batch hold noise too: the kernels never read the former, and the latter costs what zeros cost."""
    if name == "mdct_pcm":
        lengths = lengths - lengths % 4
    rng = np.random.default_rng(1)
    slots = (lengths + 63) // 64 * 64
    in_offsets = np.zeros(len(lengths), np.int64)
    in_offsets[1:] = np.cumsum(slots)[:-1]
    nmax = int(lengths.max())
    packed = zafx.DeviceBuffer((int(slots.sum()),), np.int16)
    packed.upload(rng.integers(-32768, 32767, packed.shape, dtype=np.int16, endpoint=True))
    padded = zafx.DeviceBuffer((CLIPS, nmax), np.int16)
    padded.upload(rng.integers(-32768, 32767, padded.shape, dtype=np.int16, endpoint=True))
    offs, frames, pitch = plan.ragged_layout(lengths)
    out = zafx.DeviceBuffer((int(offs[-1]),), plan.out_dtype)
    o = zafx.DeviceBuffer(plan.out_shape(CLIPS, nmax), plan.out_dtype)
    call = lambda: plan.execute_ragged_pcm(packed, in_offsets, lengths, out, 1)   # noqa: E731
    kernels = {}

    def noting(key, launch):
        def run():
            launch()
            kernels[key] = plan.last_kernel
        return run
    launches = {"native": noting("native", call), "convert_first": noting("convert_first", with_env("ZAFX_RAGGED_PCM_NATIVE", "0", call)),
                "padded": noting("padded", lambda: plan.execute_pcm(padded, o, CLIPS, nmax, 1))}
    res = {"samples": int(lengths.sum()), "longest": nmax}
    res.update(timed_in_turn(plan, launches, reps))
    for b in (packed, padded, out, o):
        b.free()
    for key in launches:
        res[key + "_kernel"] = kernels[key]
        res[key]["msamples_per_s"] = res["samples"] / (res[key]["median_ms"] * 1e3)
    res["convert_first_over_native"] = res["convert_first"]["median_ms"] / res["native"]["median_ms"]
    res["padded_over_native"] = res["padded"]["median_ms"] / res["native"]["median_ms"]
    res["native_is_fastest"] = bool(res["native"]["median_ms"] < min(res["convert_first"]["median_ms"], res["padded"]["median_ms"]))
    n, c, p = res["native"], res["convert_first"], res["padded"]
    print(f"{name:9s} native {n['median_ms']:7.3f} ms ({n['min_ms']:.3f}-{n['max_ms']:.3f}) {n['msamples_per_s']:8.0f} Ms/s [{res['native_kernel']}] | "
          f"convert first {c['median_ms']:7.3f} ms ({c['min_ms']:.3f}-{c['max_ms']:.3f}) [{res['convert_first_kernel']}] | padded {p['median_ms']:7.3f} ms "
          f"({p['min_ms']:.3f}-{p['max_ms']:.3f}) [{res['padded_kernel']}] | convert first / native {res['convert_first_over_native']:.3f}, "
          f"padded / native {res['padded_over_native']:.3f}", flush=True)
    return res


F64_KINDS = ("stft64", "mdct64", "mel64", "mfcc64")


def inputs_f64(lengths):
    """The two float64 input arrays the four float64 kinds share: the packed ragged batch and the batch padded to the longest clip.  Noise
    throughout (the gaps and the padding too: the kernels never read the former, the latter costs what zeros cost), drawn as float32."""
    rng = np.random.default_rng(1)
    slots = (lengths + 31) // 32 * 32
    in_offsets = np.zeros(len(lengths), np.int64)
    in_offsets[1:] = np.cumsum(slots)[:-1]
    bufs = {}
    for key, shape in (("ragged", (int(slots.sum()),)), ("padded", (CLIPS, int(lengths.max())))):
        bufs[key] = zafx.DeviceBuffer(shape, np.float64)
        bufs[key].upload(rng.standard_normal(shape, dtype=np.float32).astype(np.float64))
    return in_offsets, bufs


def measure_f64(name, plan, lengths, in_offsets, bufs, reps):
    """ragged / padded / per-clip of one float64 kind on one plan (zafx_execute_ragged on the tiled float64 kernels' RAGGED forms)."""
    nmax = int(lengths.max())
    offs, frames, pitch = plan.ragged_layout(lengths)
    out = zafx.DeviceBuffer((int(offs[-1]),), plan.out_dtype)
    o = zafx.DeviceBuffer(plan.out_shape(CLIPS, nmax), plan.out_dtype)
    call = lambda: plan.execute_ragged(bufs["ragged"], in_offsets, lengths, out)   # noqa: E731
    kernels = {}

    def noting(key, launch):
        def run():
            launch()
            kernels[key] = plan.last_kernel
        return run
    launches = {"ragged": noting("ragged", call), "padded": noting("padded", lambda: plan.execute(bufs["padded"], o, CLIPS, nmax)),
                "per_clip": noting("per_clip", with_env("ZAFX_RAGGED_F64_NATIVE", "0", call))}
    res = {"samples": int(lengths.sum()), "longest": nmax, "ragged_output_bytes": int(offs[-1]) * plan.out_dtype.itemsize,
           "padded_output_bytes": int(np.prod(plan.out_shape(CLIPS, nmax), dtype=np.int64)) * plan.out_dtype.itemsize}
    res.update(timed_in_turn(plan, launches, reps))
    out.free()
    o.free()
    for key in launches:
        res[key + "_kernel"] = kernels[key]
        res[key]["msamples_per_s"] = res["samples"] / (res[key]["median_ms"] * 1e3)
    res["padded_over_ragged"] = res["padded"]["median_ms"] / res["ragged"]["median_ms"]
    res["per_clip_over_ragged"] = res["per_clip"]["median_ms"] / res["ragged"]["median_ms"]
    res["ragged_is_fastest"] = bool(res["ragged"]["median_ms"] < min(res["padded"]["median_ms"], res["per_clip"]["median_ms"]))
    r, p, c = res["ragged"], res["padded"], res["per_clip"]
    print(f"{name:9s} ragged {r['median_ms']:7.3f} ms ({r['min_ms']:.3f}-{r['max_ms']:.3f}) {r['msamples_per_s']:8.0f} Ms/s [{res['ragged_kernel']}] | "
          f"padded {p['median_ms']:7.3f} ms ({p['min_ms']:.3f}-{p['max_ms']:.3f}) [{res['padded_kernel']}] | per clip {c['median_ms']:7.3f} ms "
          f"({c['min_ms']:.3f}-{c['max_ms']:.3f}) [{res['per_clip_kernel']}] | padded / ragged {res['padded_over_ragged']:.3f}, "
          f"per clip / ragged {res['per_clip_over_ragged']:.1f}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--kinds", default="stft,mel,mfcc,mel+mfcc,mdct,mdct_any")
    ap.add_argument("--imdct-k", default="2,4,8,12,16,24")
    ap.add_argument("--istft-k", default="2,4,8,12,16,24")
    a = ap.parse_args()
    kinds = a.kinds.split(",")
    rng = np.random.default_rng(0)
    lengths = rng.integers(5 * FS, 15 * FS + 1, CLIPS).astype(np.int64)
    lengths -= lengths % 2
    window = zafx.hamming(W)
    fb = zafx.melfilterbank(FS, W, 128)
    plans = {
        "stft": zafx.stft_plan(window, HOP, row_align=16),
        "mel": zafx.mel_plan(window, HOP, fb, row_align=32),
        "mfcc": zafx.mel_plan(window, HOP, fb, 20, row_align=32),
        "mel+mfcc": zafx.mel_plan(window, HOP, fb, 20, row_align=32, also_mel=True),
    }
    result = {"device": zafx.device_name(0), "clips": CLIPS, "window": W, "hop": HOP, "samples": int(lengths.sum()),
              "longest": int(lengths.max()), "reps": a.reps}
    if any(k in plans for k in kinds):
        in_offsets, bufs = inputs(lengths)
        for name, plan in plans.items():
            if name in kinds:
                result[name] = measure(name, plan, lengths, in_offsets, bufs, a.reps)
        for b in bufs.values():
            b.free()
    for name in ("mdct", "mdct_any"):
        if name in kinds:
            result[name] = measure_mdct(name, lengths, a.reps)
    if "imdct" in kinds:
        result["imdct"] = measure_imdct(lengths, a.reps, [int(k) for k in a.imdct_k.split(",") if k])
    fastest = True
    if "istft" in kinds:
        sweep = [int(k) for k in a.istft_k.split(",") if k]
        for name, onesided in (("istft", False), ("istft_onesided", True)):
            result[name] = measure_istft(name, onesided, lengths, a.reps, sweep)
            fastest = fastest and result[name]["ragged_is_fastest"]
    pcm_plans = {"mel_pcm": plans["mel"], "mfcc_pcm": plans["mfcc"], "stft_pcm": plans["stft"]}
    pcm_fastest = True
    for name in PCM_KINDS:
        if name in kinds:
            plan = pcm_plans[name] if name in pcm_plans else zafx.mdct_plan(zafx.kaiser_bessel_derived(W), row_align=32)
            result[name] = measure_pcm(name, plan, lengths, a.reps)
            pcm_fastest = pcm_fastest and result[name]["native_is_fastest"]
    f64_fastest = True
    if any(k in F64_KINDS for k in kinds):
        kbd = zafx.kaiser_bessel_derived(W)
        f64_plans = {"stft64": lambda: zafx.stft_plan(window, HOP, f64=True, row_align=8), "mdct64": lambda: zafx.mdct_plan(kbd, row_align=16, f64=True),
                     "mel64": lambda: zafx.mel_plan(window, HOP, fb, row_align=16, f64=True), "mfcc64": lambda: zafx.mel_plan(window, HOP, fb, 20, row_align=16, f64=True)}
        in_offsets, bufs = inputs_f64(lengths)
        for name in F64_KINDS:
            if name in kinds:
                result[name] = measure_f64(name, f64_plans[name](), lengths, in_offsets, bufs, a.reps)
                f64_fastest = f64_fastest and result[name]["ragged_is_fastest"]
        for b in bufs.values():
            b.free()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    if not fastest:
        print("the one launch of the ragged ISTFT is not faster than both alternatives")
    if not pcm_fastest:
        print("a ragged PCM kind's native launch is not faster than both alternatives (convert first, padded)")
    if not f64_fastest:
        print("a float64 kind's one ragged launch is not faster than both alternatives (padded, per clip)")
    if not (fastest and pcm_fastest and f64_fastest):
        sys.exit(1)


if __name__ == "__main__":
    main()
