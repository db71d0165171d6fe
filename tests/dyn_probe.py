"""Child process of tests/test_gpu_stft_dynamic.py: one case of k_stft_ft16 with its tiles claimed at run time (the default) against the
static split (ZAFX_STFT_DYNAMIC=0 at plan creation), in one process and into buffers of one shape.  Prints one JSON line.

    python tests/dyn_probe.py headline|padded433|ragged|few|odd
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zaf-python_amd"))
import zafx  # noqa: E402
from zafx import _lib  # noqa: E402
from zafx.core import Plan  # noqa: E402

W, HOP = 2048, 1024


def make_plan(dynamic, row_align=0):
    """A plan of its own (not the cached one of zafx.stft_plan): the switch is read when the plan is created."""
    old = os.environ.get("ZAFX_STFT_DYNAMIC")
    os.environ["ZAFX_STFT_DYNAMIC"] = "1" if dynamic else "0"
    try:
        p = Plan(_lib.STFT, 0, window_length=W, step_length=HOP, layout="FT", onesided=False, row_align=row_align)
        p.set_window(zafx.hamming(W))
    finally:
        if old is None:
            del os.environ["ZAFX_STFT_DYNAMIC"]
        else:
            os.environ["ZAFX_STFT_DYNAMIC"] = old
    return p


def equal_case(n_clips, n_samples, row_align):
    x = np.random.default_rng([7, n_clips, n_samples]).standard_normal((n_clips, n_samples)).astype(np.float32)
    d_x = zafx.DeviceBuffer.from_host(x)
    outs, kernels = {}, {}
    for name, dynamic in (("static", False), ("claimed", True)):
        plan = make_plan(dynamic, row_align)
        shape = plan.out_shape(n_clips, n_samples)
        runs = []
        for _ in range(3):   # three launches in a row of one plan: the counters came back to zero each time
            d_out = zafx.DeviceBuffer(shape, np.complex64)
            d_out.upload(np.full(shape, np.nan + 0j, np.complex64))
            plan.execute(d_x, d_out, n_clips, n_samples)
            plan.sync()
            runs.append(d_out.download())
            d_out.free()
        outs[name], kernels[name] = runs, plan.last_kernel
    frames = plan.out_dims(n_samples)[1]
    tiles = n_clips * ((frames + 15) // 16)
    return outs, kernels, {"tiles": tiles, "frames": frames, "pitch": plan.row_pitch(n_samples)}


def ragged_case():
    rng = np.random.default_rng(11)
    lengths = (rng.integers(5 * 22050, 15 * 22050, 37) * 2).astype(np.int64)
    slots = (lengths + 31) // 32 * 32
    in_offsets = np.zeros(len(lengths), np.int64)
    in_offsets[1:] = np.cumsum(slots)[:-1]
    d_x = zafx.DeviceBuffer((int(slots.sum()),), np.float32)
    d_x.upload(rng.standard_normal(int(slots.sum()), dtype=np.float32))
    outs, kernels = {}, {}
    for name, dynamic in (("static", False), ("claimed", True)):
        plan = make_plan(dynamic, row_align=16)
        offs, frames, _ = plan.ragged_layout(lengths)
        runs = []
        for _ in range(3):
            d_out = zafx.DeviceBuffer((int(offs[-1]),), np.complex64)
            d_out.upload(np.full(int(offs[-1]), np.nan + 0j, np.complex64))
            plan.execute_ragged(d_x, in_offsets, lengths, d_out)
            plan.sync()
            runs.append(d_out.download())
            d_out.free()
        outs[name], kernels[name] = runs, plan.last_kernel
    return outs, kernels, {"tiles": int(((frames + 15) // 16).sum())}


CASES = {
    "headline": lambda: equal_case(64, 441000, 0),       # the benchmark's geometry (T = 432: rows are whole lines) on a reduced batch
    "padded433": lambda: equal_case(64, 442000, 16),     # T = 433 on rows padded to whole lines
    "few": lambda: equal_case(3, 441000, 0),             # 81 tiles: fewer than workgroups
    "odd": lambda: equal_case(21, 441000, 0),            # 567 tiles: not a multiple of eight, nor of the grid
    "ragged": ragged_case,
}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


if __name__ == "__main__":
    outs, kernels, info = CASES[sys.argv[1]]()
    ref = outs["static"][0]
    res = dict(info, case=sys.argv[1], kernels=kernels,
               static_repeatable=all(np.array_equal(bits(r), bits(ref)) for r in outs["static"]),
               claimed_equal=[bool(np.array_equal(bits(r), bits(ref))) for r in outs["claimed"]],
               written=bool(np.isfinite(ref.view(np.float32)).mean() > 0.9))
    got = outs["claimed"][0]
    if not res["claimed_equal"][0]:   # what differs, for the record
        a, b = got.view(np.float32), ref.view(np.float32)
        both = np.isfinite(a) & np.isfinite(b)
        res.update(words_differing=int((a.view(np.uint32) != b.view(np.uint32)).sum()), words=int(a.size),
                   nan_only_in_claimed=int((~np.isfinite(a) & np.isfinite(b)).sum()),
                   max_abs_diff=float(np.max(np.abs(a[both] - b[both]))) if both.any() else None)
    print(json.dumps(res))
