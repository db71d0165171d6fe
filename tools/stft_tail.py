#!/usr/bin/env python3
"""When do the workgroups of k_stft_ft16 finish?  (library built with -DZAFX_PROF: tools/build_prof.sh)

    ZAFX_LIBRARY=tools/bin/libzafx_prof.so python tools/stft_tail.py [--buffers 7] [--launches 5] [--out FILE]

Headline geometry (1024 clips x 10 s, W = 2048, hop 1024, two-sided, (W, T) layout).  Thread 0 of every workgroup leaves its XCD
(blockIdx.x & 7, what xcd_order assumes), the tiles it ran and the chip-wide 100-MHz clock at its start, its first store and behind its last
tile.  For the static split (ZAFX_STFT_DYNAMIC=0) and for the tiles claimed at run time, over `--buffers` output buffers held at once (the
placement of the 7.25 GB decides the kernel's time: DESIGN.md section 3), the tool prints per XCD and over all workgroups the earliest,
median and latest finish in microseconds from the launch's first start, and the share of the launch between the earliest and the latest
finish -- the time during which fewer than all CUs feed the HBM write queues.  Per buffer the median launch (by its span) is reported;
the summary names the fastest and the slowest buffer of each form.
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
from zafx import _lib as _zlib  # noqa: E402
from zafx.core import Plan  # noqa: E402


def make_plan(dynamic):
    """A plan of its own (zafx.stft_plan caches): ZAFX_STFT_DYNAMIC is read when the plan is created."""
    os.environ["ZAFX_STFT_DYNAMIC"] = "1" if dynamic else "0"
    p = Plan(_zlib.STFT, 0, window_length=2048, step_length=1024, layout="FT", onesided=False)
    p.set_window(zafx.hamming(2048))
    del os.environ["ZAFX_STFT_DYNAMIC"]
    return p

B, N = 1024, 441000
TICK_US = 0.01   # wall_clock64: 100 MHz


def launch_stats(words, n_wg):
    w = np.array(words[: 4 * n_wg], np.uint64).reshape(n_wg, 4)
    xcd, tiles = (w[:, 0] & np.uint64(7)).astype(int), (w[:, 0] >> np.uint64(8)).astype(int)
    t0 = w[:, 1].min()
    start, first, end = ((w[:, i] - t0).astype(np.int64) * TICK_US for i in (1, 2, 3))
    span = float(end.max())
    rows = {}
    for name, sel in [("all", np.ones(n_wg, bool))] + [(f"xcd{x}", xcd == x) for x in range(8)]:
        e = end[sel]
        rows[name] = {"earliest_us": float(e.min()), "median_us": float(np.median(e)), "latest_us": float(e.max()),
                      "tiles_min": int(tiles[sel].min()), "tiles_max": int(tiles[sel].max())}
    return {"span_us": span, "tail_share": float((end.max() - end.min()) / span), "last_start_us": float(start.max()),
            "first_store_median_us": float(np.median(first)), "tiles_total": int(tiles.sum()), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    lib = _lib.load()
    if not hasattr(lib, "zafx_debug_stft_tail_bind"):
        raise SystemExit("needs the ZAFX_PROF library: tools/build_prof.sh, then ZAFX_LIBRARY=tools/bin/libzafx_prof.so")
    x = np.random.default_rng(0).standard_normal((8, N)).astype(np.float32)
    d_x = zafx.DeviceBuffer.from_host(np.tile(x, (B // 8, 1)))
    plans = {"static": make_plan(False), "claimed": make_plan(True)}
    shape = plans["static"].out_shape(B, N)
    bufs = [zafx.DeviceBuffer(shape, np.complex64) for _ in range(args.buffers)]
    n_wg = 256
    words = (ctypes.c_ulonglong * (4 * n_wg))()
    for _ in range(60):   # clocks up
        plans["static"].execute(d_x, bufs[0], B, N)
    plans["static"].sync()
    report = {"buffers": args.buffers, "launches": args.launches, "forms": {}}
    for form, plan in plans.items():
        per_buf = []
        for bi, buf in enumerate(bufs):
            for _ in range(6):
                plan.execute(d_x, buf, B, N)
            plan.sync()
            stats = []
            for _ in range(args.launches):
                assert lib.zafx_debug_stft_tail_bind(plan.handle, 1) == 0
                plan.timer_start()
                plan.execute(d_x, buf, B, N)
                ms = plan.timer_stop()
                assert lib.zafx_debug_stft_tail_read(plan.handle, words, 4 * n_wg) == 0
                st = launch_stats(list(words), n_wg)
                st["event_ms"] = ms
                assert st["tiles_total"] == B * 27, st["tiles_total"]
                stats.append(st)
            assert lib.zafx_debug_stft_tail_bind(plan.handle, 0) == 0
            stats.sort(key=lambda s: s["span_us"])
            med = stats[len(stats) // 2]
            med["buffer"] = bi
            med["tail_share_all_launches"] = [round(s["tail_share"], 4) for s in stats]
            per_buf.append(med)
        per_buf.sort(key=lambda s: s["span_us"])
        report["forms"][form] = {"kernel": plan.last_kernel, "fastest": per_buf[0], "slowest": per_buf[-1],
                                 "all_spans_us": [round(s["span_us"], 1) for s in per_buf],
                                 "all_tail_shares": [round(s["tail_share"], 4) for s in per_buf]}
        for tag in ("fastest", "slowest"):
            s = report["forms"][form][tag]
            print(f"{form:8s} {tag} buffer ({s['buffer']}): span {s['span_us']:.1f} us (event {s['event_ms'] * 1e3:.1f}), last start {s['last_start_us']:.1f}, "
                  f"first store (median) {s['first_store_median_us']:.1f}, earliest-to-latest finish = {100 * s['tail_share']:.2f} % of the launch")
            for name, r in s["rows"].items():
                print(f"    {name:5s} finish earliest {r['earliest_us']:8.1f}  median {r['median_us']:8.1f}  latest {r['latest_us']:8.1f} us   tiles per workgroup {r['tiles_min']}-{r['tiles_max']}")
        print(f"{form:8s} spans of all buffers (us): {report['forms'][form]['all_spans_us']}  tail shares: {report['forms'][form]['all_tail_shares']}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
