"""Writes tests/golden/maskfilter_messages.json: what the host side of the four mask-filter kinds (real, stems, complex, stereo) says when it
refuses a call, as whole strings -- this project's own output, recorded so that a change of the host path can be held to "no message moved"
(tests/test_maskfilter_messages_host.py replays the catalogue below and compares).

Two layers.  python: every public function of the family (the four one-clip functions, their *_batch and *_ragged forms, the four
pack_ragged_*masks) on a handful of refused calls each, with zafx._lib.load replaced by a function that raises -- a call that passes every
check is recorded as reaching the library, nothing needs a device.  routes: the stdout of the four tests/host_emu/*_routes_emu programs
(zafx_routes.hpp compiled by g++) on a fixed input covering, per form, a call taken, another kind, layout and count, a clip at and above
the bound and a refused clip in the middle of a batch.

Run from the repository root:  python tests/golden/make_maskfilter_messages_golden.py"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "zaf-python_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "maskfilter_messages.json")
CSRC = os.path.join(ROOT, "zaf-python_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "host_emu")

KINDS = ("", "_stems", "_complex", "_stereo")
PYTHON_FUNCTIONS = tuple(f"maskfilter{k}{form}" for form in ("", "_batch", "_ragged") for k in KINDS) + (
    "pack_ragged_masks", "pack_ragged_stems_masks", "pack_ragged_complex_masks", "pack_ragged_stereo_masks")
ROUTES_EMUS = ("maskfilter_stems_routes_emu", "maskfilter_stems_ragged_routes_emu", "maskfilter_complex_routes_emu", "maskfilter_stereo_routes_emu")

W, H, ROWS = 256, 128, 129
N = 300                    # samples (sample frames) of the equal-length clips: 4 frames
LENGTHS = (300, 1, 500)    # of the ragged clips: 4, 2 and 5 frames


def frames(n):
    return (n + H - 1) // H + 1


def clip(kind, n, dtype=np.float32):
    return np.zeros((n, 2) if kind == "_stereo" else (n,), dtype)


def mask(kind, n, layout, count=None, short=0, dtype=np.float32):
    """One clip's mask(s) in `layout`; count: stems, or the stereo kind's mask_channels (1: a shared mask); short: frames left out."""
    t = frames(n) - short
    shape = (ROWS, t) if layout == "FT" else (t, ROWS)
    if kind == "_stems":
        shape = (2 if count is None else count,) + shape
    if kind == "_stereo" and count == 2:
        shape = (2,) + shape if layout == "FT" else (t, 2, ROWS)
    return np.zeros(shape, dtype)


def other(layout):
    return "TF" if layout == "FT" else "FT"


def single_cases(z, kind):
    f = getattr(z, "maskfilter" + kind)
    w = np.hamming(W)
    x, m = clip(kind, N), mask(kind, N, "FT")
    yield "taken", lambda: f(x, w, H, m)
    yield "signal of wrong rank", lambda: f(np.zeros((2, 3, 4), np.float32), w, H, m)
    yield "mono signal to stereo or stereo to mono", lambda: f(clip("" if kind == "_stereo" else "_stereo", N), w, H, m)
    yield "complex signal", lambda: f(clip(kind, N, np.complex64), w, H, m)
    yield "mask of wrong rank", lambda: f(x, w, H, np.zeros((2, 2, 2, ROWS, 4), np.float32))
    yield "1-D mask", lambda: f(x, w, H, np.zeros(ROWS, np.float32))
    yield "mask one frame short", lambda: f(x, w, H, mask(kind, N, "FT", short=1))
    yield "mask in the other layout", lambda: f(x, w, H, mask(kind, N, "TF"))
    yield "non-numeric mask", lambda: f(x, w, H, mask(kind, N, "FT").astype(str))
    yield "complex mask", lambda: f(x, w, H, mask(kind, N, "FT", dtype=np.complex64))
    yield "bad step_length", lambda: f(x, w, 64, m)
    yield "step_length zero", lambda: f(x, w, 0, m)
    yield "window not a power of two", lambda: f(x, np.hamming(300), 150, m)
    yield "window too long", lambda: f(x, np.hamming(4096), 2048, m)
    yield "2-D window", lambda: f(x, np.zeros((2, W)), H, m)
    if kind == "_stems":
        yield "0 stems", lambda: f(x, w, H, mask(kind, N, "FT", 0))
        yield "9 stems", lambda: f(x, w, H, mask(kind, N, "FT", 9))
    if kind == "_stereo":
        yield "taken, a mask per channel", lambda: f(x, w, H, mask(kind, N, "FT", 2))
        yield "4-D stereo mask", lambda: f(x, w, H, np.zeros((2, 2, ROWS, 4), np.float32))
        yield "three masks", lambda: f(x, w, H, np.zeros((3, ROWS, 4), np.float32))


def batch_cases(z, kind):
    f = getattr(z, "maskfilter" + kind + "_batch")
    w = np.hamming(W)
    b = 2
    out_shape = {"": (b, N), "_stems": (b, 2, N), "_complex": (b, N), "_stereo": (b, N, 2)}[kind]
    rest_shape = {"": (b, 2, N), "_stems": (b, 3, N), "_complex": (b, 2, N), "_stereo": (b, 2, N, 2)}[kind]
    for layout in ("FT", "TF"):
        x = np.stack([clip(kind, N)] * b)
        m = np.stack([mask(kind, N, layout)] * b)
        tag = f"{layout}: "
        yield tag + "taken", lambda x=x, m=m, layout=layout: f(x, w, m, layout=layout)
        yield tag + "taken with rest and out", lambda x=x, m=m, layout=layout: f(x, w, m, rest=True, layout=layout, out=np.empty(rest_shape, np.float32))
        yield tag + "clips of wrong rank", lambda m=m, layout=layout: f(np.zeros((b, N, 2, 2), np.float32), w, m, layout=layout)
        yield tag + "one clip, no batch axis", lambda m=m, layout=layout: f(clip(kind, N), w, m, layout=layout)
        yield tag + "stereo clips with three channels", lambda m=m, layout=layout: f(np.zeros((b, N, 3), np.float32), w, m, layout=layout)
        yield tag + "complex clips", lambda m=m, layout=layout: f(np.stack([clip(kind, N, np.complex64)] * b), w, m, layout=layout)
        yield tag + "complex masks", lambda x=x, m=m, layout=layout: f(x, w, m.astype(np.complex64), layout=layout)
        yield tag + "non-numeric masks", lambda x=x, m=m, layout=layout: f(x, w, m.astype(str), layout=layout)
        yield tag + "non-numeric masks of wrong shape", lambda x=x, layout=layout: f(x, w, np.array(["a", "b"]), layout=layout)
        yield tag + "masks one frame short", lambda x=x, layout=layout: f(x, w, np.stack([mask(kind, N, layout, short=1)] * b), layout=layout)
        yield tag + "masks in the other layout", lambda x=x, layout=layout: f(x, w, np.stack([mask(kind, N, other(layout))] * b), layout=layout)
        yield tag + "masks of three clips for two", lambda x=x, layout=layout: f(x, w, np.stack([mask(kind, N, layout)] * 3), layout=layout)
        yield tag + "2-D masks", lambda x=x, layout=layout: f(x, w, np.zeros((b, ROWS), np.float32), layout=layout)
        yield tag + "5-D masks", lambda x=x, layout=layout: f(x, w, np.zeros((b, 2, 2, ROWS, 4), np.float32), layout=layout)
        yield tag + "out of wrong shape", lambda x=x, m=m, layout=layout: f(x, w, m, layout=layout, out=np.empty(rest_shape, np.float32))
        yield tag + "out of wrong shape with rest", lambda x=x, m=m, layout=layout: f(x, w, m, rest=True, layout=layout, out=np.empty(out_shape, np.float32))
        yield tag + "float64 out", lambda x=x, m=m, layout=layout: f(x, w, m, layout=layout, out=np.empty(out_shape, np.float64))
        yield tag + "out not contiguous", lambda x=x, m=m, layout=layout: f(x, w, m, layout=layout, out=np.empty(out_shape[::-1], np.float32).T)
        yield tag + "read-only out", lambda x=x, m=m, layout=layout: f(x, w, m, layout=layout, out=np.broadcast_to(np.float32(0), out_shape))
        yield tag + "bad step_length", lambda x=x, m=m, layout=layout: f(x, w, m, step_length=64, layout=layout)
        yield tag + "window not a power of two", lambda x=x, m=m, layout=layout: f(x, np.hamming(300), m, layout=layout)
        yield tag + "empty batch", lambda layout=layout: f(np.stack([clip(kind, N)] * b)[:0], w, np.stack([mask(kind, N, layout)] * b)[:0], layout=layout)
        yield tag + "clips of no samples", lambda layout=layout: f(np.stack([clip(kind, 0)] * b), w, np.stack([mask(kind, 0, layout)] * b), layout=layout)
        if kind == "_stems":
            yield tag + "0 stems", lambda x=x, layout=layout: f(x, w, np.stack([mask(kind, N, layout, 0)] * b), layout=layout)
            yield tag + "9 stems", lambda x=x, layout=layout: f(x, w, np.stack([mask(kind, N, layout, 9)] * b), layout=layout)
            yield tag + "3-D masks", lambda x=x, layout=layout: f(x, w, np.stack([mask("", N, layout)] * b), layout=layout)
        if kind == "_stereo":
            yield tag + "taken, a mask per channel", lambda x=x, layout=layout: f(x, w, np.stack([mask(kind, N, layout, 2)] * b), layout=layout)
            yield tag + "a mask per channel, one frame short", lambda x=x, layout=layout: f(x, w, np.stack([mask(kind, N, layout, 2, short=1)] * b), layout=layout)
            yield tag + "a mask per channel in the other layout", lambda x=x, layout=layout: f(x, w, np.stack([mask(kind, N, other(layout), 2)] * b), layout=layout)
            yield tag + "three masks per clip", lambda x=x, layout=layout: f(x, w, np.zeros((b, 3, ROWS, 4), np.float32), layout=layout)
            yield tag + "boolean masks", lambda x=x, m=m, layout=layout: f(x, w, m.astype(bool), layout=layout)
    yield "unknown layout", lambda: f(np.stack([clip(kind, N)] * b), w, np.stack([mask(kind, N, "FT")] * b), layout="XY")


def mask_batch_cases(kind, call):
    """Refused mask batches, for pack_ragged_*masks and through maskfilter_*_ragged alike; call(masks, lengths, layout)."""
    for layout in ("FT", "TF"):
        ms = [mask(kind, n, layout) for n in LENGTHS]
        tag = f"{layout}: "
        yield tag + "taken", lambda ms=ms, layout=layout: call(ms, LENGTHS, layout)
        yield tag + "one array where a sequence is wanted", lambda ms=ms, layout=layout: call(ms[0], LENGTHS[:1], layout)
        yield tag + "one 1-D array", lambda layout=layout: call(np.zeros(ROWS, np.float32), LENGTHS[:1], layout)
        yield tag + "one stacked array of one more dimension", lambda ms=ms, layout=layout: call(np.stack([ms[0]] * 3), (N, N, N), layout)
        yield tag + "not a sequence", lambda layout=layout: call(7, LENGTHS, layout)
        yield tag + "masks and lengths of different counts", lambda ms=ms, layout=layout: call(ms[:2], LENGTHS, layout)
        yield tag + "no masks for three clips", lambda layout=layout: call([], LENGTHS, layout)
        yield tag + "mask 1 of the wrong shape", lambda ms=ms, layout=layout: call([ms[0], ms[0], ms[2]], LENGTHS, layout)
        yield tag + "mask 2 one frame short", lambda ms=ms, layout=layout: call(ms[:2] + [mask(kind, LENGTHS[2], layout, short=1)], LENGTHS, layout)
        yield tag + "mask 0 in the other layout", lambda ms=ms, layout=layout: call([mask(kind, LENGTHS[0], other(layout))] + ms[1:], LENGTHS, layout)
        yield tag + "mask 1 of wrong rank", lambda ms=ms, layout=layout: call([ms[0], np.zeros(ROWS, np.float32), ms[2]], LENGTHS, layout)
        yield tag + "mask 0 of wrong rank", lambda ms=ms, layout=layout: call([np.zeros((2, 2, 2, ROWS), np.float32)] + ms[1:], LENGTHS, layout)
        yield tag + "mask 2 non-numeric", lambda ms=ms, layout=layout: call(ms[:2] + [ms[2].astype(str)], LENGTHS, layout)
        yield tag + "mask 1 complex", lambda ms=ms, layout=layout: call([ms[0], ms[1].astype(np.complex64), ms[2]], LENGTHS, layout)
        if kind == "_stems":
            yield tag + "a stem count that differs between clips", lambda ms=ms, layout=layout: call([ms[0], mask(kind, LENGTHS[1], layout, 3), ms[2]], LENGTHS, layout)
            yield tag + "0 stems", lambda layout=layout: call([mask(kind, n, layout, 0) for n in LENGTHS], LENGTHS, layout)
            yield tag + "9 stems", lambda layout=layout: call([mask(kind, n, layout, 9) for n in LENGTHS], LENGTHS, layout)
        if kind == "_stereo":
            yield tag + "taken, a mask per channel", lambda layout=layout: call([mask(kind, n, layout, 2) for n in LENGTHS], LENGTHS, layout)
            yield tag + "mask 1 shared, mask 0 per channel", lambda ms=ms, layout=layout: call([mask(kind, LENGTHS[0], layout, 2)] + ms[1:], LENGTHS, layout)
            yield tag + "mask 1 per channel, one frame short", lambda layout=layout: call(
                [mask(kind, n, layout, 2, short=int(i == 1)) for i, n in enumerate(LENGTHS)], LENGTHS, layout)
            yield tag + "mask 0 per channel in the other layout", lambda layout=layout: call(
                [mask(kind, n, other(layout) if i == 0 else layout, 2) for i, n in enumerate(LENGTHS)], LENGTHS, layout)


def ragged_cases(z, kind):
    f = getattr(z, "maskfilter" + kind + "_ragged")
    w = np.hamming(W)
    xs = [clip(kind, n) for n in LENGTHS]
    ms = [mask(kind, n, "FT") for n in LENGTHS]
    yield from mask_batch_cases(kind, lambda masks, lengths, layout: f([clip(kind, n) for n in lengths], w, masks, layout=layout))
    yield "taken with rest", lambda: f(xs, w, ms, rest=True)
    yield "clips: one array where a sequence is wanted", lambda: f(xs[0], w, ms)
    yield "clips: not a sequence", lambda: f(7, w, ms)
    yield "clips: none", lambda: f([], w, [])
    yield "clip 1 of wrong rank", lambda: f([xs[0], np.zeros((2, 2, 2), np.float32), xs[2]], w, ms)
    yield "clip 1 mono for stereo or stereo for mono", lambda: f([xs[0], clip("" if kind == "_stereo" else "_stereo", LENGTHS[1]), xs[2]], w, ms)
    yield "clip 2 with three channels", lambda: f(xs[:2] + [np.zeros((LENGTHS[2], 3), np.float32)], w, ms)
    yield "clip 2 complex", lambda: f(xs[:2] + [clip(kind, LENGTHS[2], np.complex64)], w, ms)
    yield "clip 0 non-numeric", lambda: f([xs[0].astype(str)] + xs[1:], w, ms)
    yield "bad step_length", lambda: f(xs, w, ms, step_length=64)
    yield "window not a power of two", lambda: f(xs, np.hamming(300), ms)
    yield "unknown layout", lambda: f(xs, w, ms, layout="XY")


def pack_cases(z, kind):
    f = getattr(z, f"pack_ragged{kind}_masks")
    yield from mask_batch_cases(kind, lambda masks, lengths, layout: f(masks, lengths, W, layout))
    ms = [mask(kind, n, "FT") for n in LENGTHS]
    yield "negative length", lambda: f(ms, (300, -1, 500), W)
    yield "2-D lengths", lambda: f(ms, np.zeros((3, 1), np.int64), W)
    yield "fractional lengths", lambda: f(ms, (300.5, 1, 500), W)
    yield "unknown layout", lambda: f(ms, LENGTHS, W, "XY")
    yield "empty batch", lambda: f([], [], W)
    if kind == "":
        yield "negative row_align", lambda: f(ms, LENGTHS, W, "FT", -1)
        yield "row_align with TF", lambda: f([mask(kind, n, "TF") for n in LENGTHS], LENGTHS, W, "TF", 16)
        yield "taken with row_align", lambda: f(ms, LENGTHS, W, "FT", 16)


class LibraryReached(Exception):
    """What a call raises that passed every check of the Python layer: it asked for the library."""


def python_catalogue(z):
    """{function name: [(case, thunk)]} over PYTHON_FUNCTIONS."""
    cat = {}
    for kind in KINDS:
        cat["maskfilter" + kind] = list(single_cases(z, kind))
        cat["maskfilter" + kind + "_batch"] = list(batch_cases(z, kind))
        cat["maskfilter" + kind + "_ragged"] = list(ragged_cases(z, kind))
        cat[f"pack_ragged{kind}_masks"] = list(pack_cases(z, kind))
    return cat


def record_python(entries):
    """[(case, thunk)] -> [{"case", "type", "message"}] with zafx._lib.load replaced by a function that raises LibraryReached; a call that
    returns is recorded by the shapes of what it returned."""
    from zafx import _lib

    def describe(r):
        if isinstance(r, (tuple, list)):
            return "(" + ", ".join(describe(v) for v in r) + ")"
        return f"{np.asarray(r).dtype}{list(np.shape(r))}"

    def no_library():
        raise LibraryReached("every check passed: the call reached the library")
    saved, _lib.load = _lib.load, no_library
    try:
        got = []
        for case, thunk in entries:
            try:
                got.append({"case": case, "type": "returned", "message": describe(thunk())})
            except Exception as e:   # whatever it is: its type and text are the record
                got.append({"case": case, "type": type(e).__name__, "message": str(e)})
        return got
    finally:
        _lib.load = saved


def routes_inputs():
    """{emu: stdin}: per form a call taken, another kind, layout and count, a clip at and above the bound, a refused clip mid-batch."""
    from zafx import _lib
    mf, mfr, stft = _lib.MASKFILTER, _lib.MASKFILTER_REST, _lib.STFT
    ft, tf = _lib.LAYOUT_FT, _lib.LAYOUT_TF
    b27, b28 = 1 << 27, 1 << 28
    stems = [f"{tf} 2 1000", f"{tf} 8 {b28 - 1}", f"{ft} 2 1000", f"{tf} 0 1000", f"{tf} 9 1000", f"{tf} -1 1000", f"{tf} 2 {b28}", f"{tf} 2 {b28 + 1}",
             f"{ft} 0 {b28}", f"{tf} 9 {b28}", f"{tf} 1 0"]
    stems_ragged = [f"{mf} {tf} 2 3 5 1000 0", f"{mfr} {tf} 8 2 {b28 - 1} 7", f"{mf} {tf} 1 0", f"{stft} {tf} 2 1 1000", f"{stft} {ft} 0 1 {b28}",
                    f"{mf} {ft} 2 1 1000", f"{mfr} {ft} 9 1 {b28}", f"{mf} {tf} 0 1 1000", f"{mf} {tf} 9 1 1000", f"{mf} {tf} 9 1 {b28}",
                    f"{mf} {tf} 2 1 {b28}", f"{mf} {tf} 2 1 {b28 + 1}", f"{mf} {tf} 2 3 5 {b28} 0", f"{mfr} {tf} 3 4 {b28 - 1} 1 {b28 + 5} {b28}"]
    cplx = [f"e {mf} {tf} 1000", f"e {mfr} {tf} {b27 - 1}", f"e {stft} {tf} 1000", f"e {stft} {ft} {b27}", f"e {mf} {ft} 1000", f"e {mfr} {ft} {b27}",
            f"e {mf} {tf} {b27}", f"e {mf} {tf} {b27 + 1}", f"e {mf} {tf} 0",
            f"r {mf} {tf} 3 5 1000 0", f"r {mfr} {tf} 2 {b27 - 1} 7", f"r {mf} {tf} 0", f"r {stft} {tf} 1 1000", f"r {stft} {ft} 1 {b27}",
            f"r {mf} {ft} 1 1000", f"r {mfr} {ft} 1 {b27}", f"r {mf} {tf} 1 {b27}", f"r {mf} {tf} 1 {b27 + 1}", f"r {mf} {tf} 3 5 {b27} 0",
            f"r {mfr} {tf} 4 {b27 - 1} 1 {b27 + 5} {b27}"]
    stereo = []
    for mc, bound in ((1, b28), (2, b27)):
        stereo += [f"e {mf} {tf} {mc} 1000", f"e {mfr} {tf} {mc} {bound - 1}", f"e {stft} {tf} {mc} 1000", f"e {mf} {ft} {mc} 1000", f"e {mf} {tf} {mc} {bound}",
                   f"e {mf} {tf} {mc} {bound + 1}", f"e {mfr} {ft} {mc} {bound}",
                   f"r {mf} {tf} {mc} 3 5 1000 0", f"r {mfr} {tf} {mc} 2 {bound - 1} 7", f"r {mf} {tf} {mc} 0", f"r {stft} {tf} {mc} 1 1000",
                   f"r {mf} {ft} {mc} 1 1000", f"r {mf} {tf} {mc} 1 {bound}", f"r {mf} {tf} {mc} 1 {bound + 1}", f"r {mf} {tf} {mc} 3 5 {bound} 0",
                   f"r {mfr} {tf} {mc} 4 {bound - 1} 1 {bound + 5} {bound}", f"r {mfr} {ft} {mc} 1 {bound}"]
    stereo += [f"e {mf} {tf} 0 1000", f"e {mf} {tf} 3 1000", f"e {stft} {ft} 3 {b28}", f"e {mf} {ft} 0 {b28}", f"e {mf} {tf} 3 {b28}", f"e {mf} {tf} 1 {b27}",
               f"r {mf} {tf} 0 1 1000", f"r {mf} {tf} 3 1 1000", f"r {stft} {ft} 3 1 {b28}", f"r {mf} {ft} 0 1 {b28}", f"r {mf} {tf} 3 1 {b28}", f"r {mf} {tf} 1 1 {b27}",
               "c 256 8 4 12 5 0 1 128 391 7685"]
    texts = dict(zip(ROUTES_EMUS, (stems, stems_ragged, cplx, stereo)))
    return {k: "\n".join(v) + "\n" for k, v in texts.items()}


def build_emu(name, directory):
    exe = os.path.join(str(directory), name)
    subprocess.run(["g++", "-std=c++17", "-DZAFX_HOST_EMU", "-O1", "-I", CSRC, os.path.join(EMU, name + ".cpp"), "-o", exe], check=True)
    return exe


def run_emu(exe, text):
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and not res.stderr, (res.returncode, res.stderr[-2000:])
    return res.stdout


def main():
    import zafx
    python = {fn: record_python(entries) for fn, entries in python_catalogue(zafx).items()}
    assert set(python) == set(PYTHON_FUNCTIONS)
    routes = {}
    with tempfile.TemporaryDirectory() as d:
        for name, text in routes_inputs().items():
            routes[name] = {"stdin": text, "stdout": run_emu(build_emu(name, d), text)}
    with open(GOLDEN, "w") as f:
        json.dump({"python": python, "routes": routes}, f, indent=1, sort_keys=True)
        f.write("\n")
    n = sum(len(v) for v in python.values())
    print(f"{GOLDEN}: {n} calls of {len(python)} functions, {len(routes)} programs, {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
