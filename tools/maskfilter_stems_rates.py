"""Rates of the mask filter with several masks per clip (k_maskfilter_stems) beside the S launches of k_maskfilter a caller ran before it
existed, in one process.

    python tools/maskfilter_stems_rates.py [--clips 1024] [--reps 30] [--stems 2,4] [--out FILE]
    python tools/maskfilter_stems_rates.py --only stems4 --reps 2      one case alone, no comparison: the command of a counter run
    python tools/maskfilter_stems_rates.py --ragged [--reps 30] [--stems 2,4] [--per-slot 4,6,8,12] [--out FILE]

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

--ragged (the recipe of tools/maskfilter_rates.py --ragged: 1024 mono clips of 5-15 s at 44.1 kHz, Hamming 2048 / 1024, "TF" masks uniform in
[0, 1], everything resident), per S and plan kind:
  ragged    one execute_masked_stems_ragged of the clips, masks and output blocks packed back to back (k_maskfilter_stems_ragged; the cutting of
            the units and the table's upload included)
  padded    the same clips padded with zeros to the longest, with masks of the longest's shape, as one execute_masked_stems
  singles   S execute_masked_ragged calls (k_maskfilter_ragged) over the same clips, call s with the clips' masks s where they lie, all S in
            one reading
median (min, max) of --reps readings after warm-up.  --per-slot: at the last S of --stems, also times the ragged call with the cutter aiming
at these numbers of units per workgroup slot (ZAFX_MASKFILTER_UNITS_PER_SLOT) instead of the library's own.  The ragged call counts as faster
than a baseline when its median lies below the baseline's by more than the larger of the two (max - min) spreads; the verdicts are printed and
stored, the exit status is 0 either way.
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


def ragged_main(a):
    fs, clips = 44100, 1024
    lengths = np.random.default_rng(0).integers(5 * fs, 15 * fs + 1, clips).astype(np.int64)
    longest, total = int(lengths.max()), int(lengths.sum())
    in_offsets = np.zeros(clips, np.int64)
    in_offsets[1:] = np.cumsum(lengths)[:-1]
    window = zafx.hamming(W)
    plans = {rest: zafx.maskfilter_plan(window, rest=rest, layout="TF") for rest in (False, True)}
    res = {"device": zafx.device_name(0), "clips": clips, "window": W, "hop": HOP, "samples": total, "longest": longest, "reps": a.reps,
           "padded_over_ragged_samples": clips * longest / total, "compute_units": plans[False].compute_units}
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
    rows, frames_pad = plans[False].mask_dims(longest)
    one_pad = rows * frames_pad
    one_offsets = plans[False].mask_ragged_layout(lengths)   # one mask per clip: element counts
    one = np.diff(one_offsets)

    def verdict(r, base):
        x, y = r["ragged"], r[base]
        spread = max(x["max_ms"] - x["min_ms"], y["max_ms"] - y["min_ms"])
        r[f"ragged_over_{base}"] = x["median_ms"] / y["median_ms"]
        r[f"faster_than_{base}"] = bool(y["median_ms"] - x["median_ms"] > spread)
        return f"ragged / {base} {r[f'ragged_over_{base}']:.3f} (larger spread {spread:.3f} ms: {'faster' if r[f'faster_than_{base}'] else 'NOT faster'})"

    for s in a.stems:
        # a mask is uniform noise whatever its shape: mask (i, j) = the first elements of noise mask (i % DISTINCT, j), in both arrays
        noise = zafx.DeviceBuffer.from_host(np.random.default_rng([2, s]).random((DISTINCT, s, one_pad), dtype=np.float32))
        mask_offsets, _ = plans[False].stems_ragged_layout(lengths, s)
        m_rag = zafx.DeviceBuffer((int(mask_offsets[-1]),), np.float32)
        m_pad = zafx.DeviceBuffer((clips, s, one_pad), np.float32)
        for i in range(clips):
            m_pad.copy_from(noise, nbytes=s * one_pad * 4, dst_offset=i * s * one_pad * 4, src_offset=(i % DISTINCT) * s * one_pad * 4)
            for j in range(s):
                m_rag.copy_from(noise, nbytes=int(one[i]) * 4, dst_offset=(int(mask_offsets[i]) + j * int(one[i])) * 4,
                                src_offset=((i % DISTINCT) * s + j) * one_pad * 4)
        noise.free()
        for rest in (False, True):
            plan, name = plans[rest], f"s{s}" + ("_rest" if rest else "")
            blocks = s + (1 if rest else 0)
            r = {}
            out = zafx.DeviceBuffer((blocks * total,), np.float32)
            out_offsets = blocks * in_offsets
            variants = [("ragged", None)] + [(f"ragged_per_slot_{v}", v) for v in (a.per_slot if s == a.stems[-1] else [])]
            for key, per_slot in variants:
                if per_slot is None:
                    os.environ.pop("ZAFX_MASKFILTER_UNITS_PER_SLOT", None)
                else:
                    os.environ["ZAFX_MASKFILTER_UNITS_PER_SLOT"] = str(per_slot)
                r[key] = timed(plan, lambda: plan.execute_masked_stems_ragged(d_rag, in_offsets, lengths, m_rag, mask_offsets, out, out_offsets, s), a.reps)
                r[key]["kernel"] = plan.last_kernel
            os.environ.pop("ZAFX_MASKFILTER_UNITS_PER_SLOT", None)
            out.free()
            # (b) S calls of the ragged one-mask kind: call j reads the clips' masks j where they lie, and writes an output array of its own
            one_blocks = 2 if rest else 1
            outs = [zafx.DeviceBuffer((one_blocks * total,), np.float32) for _ in range(s)]
            offs = [np.ascontiguousarray(mask_offsets[:-1] + j * one) for j in range(s)]

            def singles():
                for j in range(s):
                    plan.execute_masked_ragged(d_rag, in_offsets, lengths, m_rag, offs[j], outs[j], one_blocks * in_offsets)
            r["singles"] = timed(plan, singles, a.reps)
            r["singles"]["kernel"] = plan.last_kernel
            for o in outs:
                o.free()
            # (a) padded to the longest
            out = zafx.DeviceBuffer(plan.stems_out_shape(clips, longest, s), np.float32)
            r["padded"] = timed(plan, lambda: plan.execute_masked_stems(d_pad, m_pad, out, clips, longest, s), a.reps)
            r["padded"]["kernel"] = plan.last_kernel
            out.free()
            for key, v in r.items():
                v["msamples_per_s"] = total / (v["median_ms"] * 1e3)
                print(f"{name:8s} {key:20s} {v['median_ms']:8.3f} ms ({v['min_ms']:.3f}-{v['max_ms']:.3f})  {v['msamples_per_s']:9.0f} Msamples/s  [{v['kernel']}]", flush=True)
            print(f"{name:8s} {verdict(r, 'padded')}; {verdict(r, 'singles')}", flush=True)
            res[name] = r
        m_rag.free(), m_pad.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--stems", type=lambda v: [int(t) for t in v.split(",") if t], default=[2, 4])
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="comma-separated case names (stems4, singles4_rest, ...); no comparison")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--per-slot", type=lambda v: [int(t) for t in v.split(",") if t], default=[])
    a = ap.parse_args()
    if a.ragged:
        return ragged_main(a)
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
