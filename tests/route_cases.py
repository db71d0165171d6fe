"""The calls of tests/test_gpu_routes.py, tests/test_routes_host.py and tests/golden/make_route_golden.py: one per outcome of the float32
launchers' route decisions (zaf-python_amd/csrc/zafx_routes.hpp), each two clips of a few frames' worth of samples.

A case is plain data (`case(...)`): the plan's geometry, the frame count, and the byte offsets of the two arrays from their 256-byte
bases.  Two things are made of it:

  * call_line(c)   the call as the host program tests/host_emu/routes_emu reads it -- arithmetic only, no GPU;
  * record(name)   the plan from the package's own factory, one execute -> (last_kernel, SHA-256 of the whole output array), or
                   ("refused", the message) where the library refuses the call.

The frame count T is 32 ("on grid": rows of whole 128-byte lines of complex64 or float32) or 33 ("off grid"); the length is the largest
whose clip has T frames (T = ceil(n / hop) + 1 for the even windows here, what long_clips.frames_of gives: tests/test_routes_host.py holds
every case to it), less `short` samples.  Inputs are seeded; this file imports the package only, never the oracle."""
import ctypes
import hashlib
import zlib

import numpy as np

FS = 44100
ON, OFF = 32, 33
SPECTRA = {False: 0, True: 1, "magnitude": 2, "power": 3}
KINDS = {"stft": 1, "istft": 2, "mdct": 3, "imdct": 4, "mel": 5, "mfcc": 6, "cqt": 7, "chroma": 8, "center": 11}
SLACK = 4096   # bytes behind either array that belong to the test (the 16-byte gathers may read a row's pad columns)


def case(family, w, hop=None, spectrum=False, layout="FT", row_align=0, frames=ON, short=0, in_delta=0, out_delta=0, filters=0, ncoef=0, pcm=False):
    hop = w // 2 if hop is None or family in ("mdct", "imdct") else hop
    return dict(family=family, W=w, hop=hop, spectrum=spectrum, layout=layout, row_align=row_align, frames=frames, short=short,
                in_delta=in_delta, out_delta=out_delta, filters=filters, ncoef=ncoef, pcm=pcm)


def _cases():
    c = {}
    # ---- forward STFT, reference layout
    for spec, tag in ((False, "two"), (True, "one"), ("magnitude", "mag"), ("power", "pow")):
        c[f"stft_2048_{tag}_on"] = case("stft", 2048, 1024, spec)
        c[f"stft_2048_{tag}_off"] = case("stft", 2048, 1024, spec, frames=OFF)
        c[f"stft_2048_{tag}_on_lines"] = case("stft", 2048, 1024, spec, row_align=16)
        c[f"stft_2048_{tag}_off_lines"] = case("stft", 2048, 1024, spec, row_align=16, frames=OFF)
        c[f"stft_2048_{tag}_x4"] = case("stft", 2048, 1024, spec, in_delta=4)
        c[f"stft_2048_{tag}_out8"] = case("stft", 2048, 1024, spec, out_delta=8)
        c[f"stft_2048_{tag}_odd"] = case("stft", 2048, 1024, spec, short=1)
    for spec, tag in ((False, "two"), (True, "one")):
        c[f"stft_1024_{tag}_on"] = case("stft", 1024, 512, spec)
    c["stft_256_on"] = case("stft", 256, 128)
    c["stft_256_off"] = case("stft", 256, 128, frames=OFF)
    c["stft_64"] = case("stft", 64, 32)
    for spec, tag in ((False, "two"), (True, "one"), ("magnitude", "mag")):
        for hop in (2048, 1024):
            c[f"stft_4096_{tag}_h{hop}_on"] = case("stft", 4096, hop, spec)
            c[f"stft_4096_{tag}_h{hop}_off"] = case("stft", 4096, hop, spec, frames=OFF)
    for spec, tag in ((False, "two"), ("magnitude", "mag")):
        c[f"stft_8192_{tag}_on"] = case("stft", 8192, 4096, spec)
        c[f"stft_8192_{tag}_off"] = case("stft", 8192, 4096, spec, frames=OFF)
    # ---- forward STFT, frame-major layout
    c["stft_2048_tf"] = case("stft", 2048, 1024, layout="TF")
    c["stft_4096_tf"] = case("stft", 4096, 2048, layout="TF")
    # ---- ISTFT
    for spec, tag in ((False, "two"), (True, "one")):
        c[f"istft_2048_{tag}"] = case("istft", 2048, 1024, spec, frames=OFF)
        c[f"istft_2048_{tag}_lines"] = case("istft", 2048, 1024, spec, row_align=16, frames=OFF)
    c["istft_2048_tf"] = case("istft", 2048, 1024, layout="TF")
    c["istft_4096_h2048"] = case("istft", 4096, 2048)
    c["istft_4096_h2048_y4"] = case("istft", 4096, 2048, out_delta=4)
    c["istft_4096_h1024"] = case("istft", 4096, 1024)
    c["istft_4096_h3002"] = case("istft", 4096, 3002)   # (no multiple of 4: not the band form)
    c["istft_8192_h4096"] = case("istft", 8192, 4096)
    c["istft_8192_h4096_y4"] = case("istft", 8192, 4096, out_delta=4)
    c["istft_8192_h2048"] = case("istft", 8192, 2048)
    # ---- MDCT
    c["mdct_256"] = case("mdct", 256)
    c["mdct_2048_on"] = case("mdct", 2048)
    c["mdct_2048_off"] = case("mdct", 2048, frames=OFF)
    c["mdct_2048_n2"] = case("mdct", 2048, short=2)
    c["mdct_2048_x4"] = case("mdct", 2048, in_delta=4)
    c["mdct_2048_tf"] = case("mdct", 2048, layout="TF")
    c["mdct_4096_on"] = case("mdct", 4096)
    c["mdct_4096_off"] = case("mdct", 4096, frames=OFF)
    c["mdct_4096_n2"] = case("mdct", 4096, short=2)
    c["mdct_8192"] = case("mdct", 8192)
    # ---- IMDCT
    c["imdct_2048"] = case("imdct", 2048)
    c["imdct_8192_pitch4"] = case("imdct", 8192)
    c["imdct_8192_pitch33"] = case("imdct", 8192, frames=OFF)
    c["imdct_8192_c4"] = case("imdct", 8192, in_delta=4)
    # ---- mel / MFCC
    c["mel_2048_even"] = case("mel", 2048, 1024, filters=40)
    c["mel_2048_odd"] = case("mel", 2048, 1024, filters=40, short=1)
    c["mfcc_2048_even"] = case("mfcc", 2048, 1024, filters=40, ncoef=13)
    c["mfcc_2048_odd"] = case("mfcc", 2048, 1024, filters=40, ncoef=13, short=1)
    c["mel_4096_128"] = case("mel", 4096, 2048, filters=128)
    c["mel_4096_300"] = case("mel", 4096, 2048, filters=300)
    c["mfcc_4096_128"] = case("mfcc", 4096, 2048, filters=128, ncoef=13)
    # ---- int16 PCM at W = 2048 (mono): a length that takes the direct route, and one that does not
    c["pcm_stft_even"] = case("stft", 2048, 1024, True, pcm=True)
    c["pcm_stft_odd"] = case("stft", 2048, 1024, True, pcm=True, short=1)
    c["pcm_mag_even"] = case("stft", 2048, 1024, "magnitude", pcm=True)
    c["pcm_mag_odd"] = case("stft", 2048, 1024, "magnitude", pcm=True, short=1)
    c["pcm_mel_even"] = case("mel", 2048, 1024, filters=40, pcm=True)
    c["pcm_mel_odd"] = case("mel", 2048, 1024, filters=40, pcm=True, short=1)
    c["pcm_mdct_n4"] = case("mdct", 2048, pcm=True)
    c["pcm_mdct_n2"] = case("mdct", 2048, pcm=True, short=2)
    return c


CASES = _cases()
N_CLIPS = 2


# ------------------------------------------------------------------------------------------------------------ arithmetic (no GPU)
def is_inverse(c):
    return c["family"] in ("istft", "imdct")


def samples(c):
    """The clip length of a forward case: the largest with c["frames"] frames, less c["short"]."""
    return (c["frames"] - 1) * c["hop"] - c["short"]


def pitch(c, t):
    a = c["row_align"]
    return -(-t // a) * a if c["layout"] == "FT" and a > 1 else t


def out_len(c):
    """Samples an inverse case gives (include/zafx.h)."""
    t, w, h = c["frames"], c["W"], c["hop"]
    return max(h * (t - 1) - 1, 0) if c["family"] == "imdct" else max(t * h - (w - h), 0)


def log2nf(c):
    return c["W"].bit_length() - (3 if c["family"] in ("mdct", "imdct") else 2)


def default_log2e(n):
    return 4 if n >= 10 else n - 6 if n >= 7 else 1


def call_line(c, n_clips=N_CLIPS, n=None, frames=None, in_addr=None, out_addr=None):
    """The case as one line of routes_emu's input.  Every table the plan of such a geometry builds is present, the claim word too."""
    t = c["frames"] if frames is None else frames
    n = (t if is_inverse(c) else samples(c)) if n is None else n
    f = dict(kind=KINDS[c["family"]], f64=0, bluestein=0, log2nf=log2nf(c), log2e=default_log2e(log2nf(c)), layout=0 if c["layout"] == "FT" else 1,
             spectrum=SPECTRA[c["spectrum"]], W=c["W"], H=c["hop"], row_align=c["row_align"], n_filters=c["filters"], tables=1, window16=1, claim=1,
             mel2=1, n_clips=n_clips, n=n, T=t, out_len=out_len(dict(c, frames=t)) if is_inverse(c) else 0,
             x=256 + c["in_delta"] if in_addr is None else in_addr, out=256 + c["out_delta"] if out_addr is None else out_addr,
             channels=1 if c["pcm"] else 0, sample_bytes=2 if c["pcm"] else 0)
    return " ".join(f"{k}={v}" for k, v in f.items())


# ------------------------------------------------------------------------------------------------------------ the running half (GPU)
def noise(tag, shape, dtype=np.float32):
    r = np.random.default_rng([43, tag])
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return (r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(dtype)
    if dtype.kind == "i":
        return np.clip(np.round(4000.0 * r.standard_normal(shape)), -32768, 32767).astype(dtype)
    return r.standard_normal(shape).astype(dtype)


def make_plan(c):
    import zafx
    w, h = c["W"], c["hop"]
    if c["family"] == "stft":
        return zafx.stft_plan(zafx.hamming(w), h, layout=c["layout"], onesided=c["spectrum"], row_align=c["row_align"])
    if c["family"] == "istft":
        return zafx.istft_plan(zafx.hamming(w), h, layout=c["layout"], onesided=c["spectrum"], row_align=c["row_align"])
    if c["family"] in ("mdct", "imdct"):
        return zafx.mdct_plan(zafx.sine(w), layout=c["layout"], inverse=c["family"] == "imdct", row_align=c["row_align"])
    return zafx.mel_plan(zafx.hamming(w), h, zafx.melfilterbank(FS, w, c["filters"]), c["ncoef"] or None, layout=c["layout"], row_align=c["row_align"])


def _view(zafx, raw, delta, nbytes):
    return zafx.DeviceBuffer((nbytes,), np.uint8, _ptr_from_pool=ctypes.c_void_p(raw.ptr.value + delta))


def run(c, plan, tag, keep=None):
    """One execute of N_CLIPS clips at the case's addresses -> the output array's bytes (row padding included).  keep: a dict that receives
    the host input ("x", as the plan's rows hold it, pad columns included) and its length or frame count ("n_in")."""
    import zafx
    n_in = c["frames"] if is_inverse(c) else samples(c)
    in_bytes, out_bytes = plan.clip_bytes(n_in)
    if c["pcm"]:
        x = noise(tag, (N_CLIPS, n_in), np.int16)
    else:
        x = noise(tag, (N_CLIPS * in_bytes // plan.in_dtype.itemsize,), plan.in_dtype)
    if keep is not None:
        keep.update(x=x, n_in=n_in)
    host = np.zeros(c["in_delta"] + x.nbytes + SLACK, np.uint8)
    host[c["in_delta"]:c["in_delta"] + x.nbytes] = np.frombuffer(x.tobytes(), np.uint8)
    raw_in = zafx.DeviceBuffer.from_host(host)
    raw_out = zafx.DeviceBuffer((c["out_delta"] + N_CLIPS * out_bytes + SLACK,), np.uint8).fill_zero()
    d_in = _view(zafx, raw_in, c["in_delta"], x.nbytes)
    d_out = _view(zafx, raw_out, c["out_delta"], N_CLIPS * out_bytes)
    d_in.dtype, d_in.shape = x.dtype, x.shape   # (execute_pcm reads both)
    try:
        if c["pcm"]:
            plan.execute_pcm(d_in, d_out, N_CLIPS, n_in, 1)
        else:
            plan.execute(d_in, d_out, N_CLIPS, n_in)
        plan.sync()
        return raw_out.download().tobytes()
    finally:
        d_in.ptr = d_out.ptr = ctypes.c_void_p()   # (views: never freed)
        raw_in.free()
        raw_out.free()


def record(name, keep=None):
    """-> [last_kernel, SHA-256 of the output bytes], or ["refused", the library's message].  keep: a dict that receives the case's plan geometry
    ("out_shape", "out_dtype", "pitch"), run's "x" and "n_in", and the output bytes ("out")."""
    import zafx
    c = CASES[name]
    zafx.clear_plan_cache()
    try:
        try:
            plan = make_plan(c)
            out = run(c, plan, zlib.crc32(name.encode()), keep)
            if keep is not None:
                n_in = keep["n_in"]
                keep.update(out=out, out_shape=plan.out_shape(N_CLIPS, n_in), out_dtype=plan.out_dtype, pitch=plan.row_pitch(n_in))
        except (RuntimeError, ValueError) as e:
            return ["refused", str(e)]
        return [plan.last_kernel, hashlib.sha256(out).hexdigest()]
    finally:
        zafx.clear_plan_cache()
