"""The cases of tests/test_gpu_accuracy.py and tests/test_accuracy_host.py: each catalogue case (tests/const_probe.py, tests/route_cases.py,
tests/linear_cases.py) and the ones added here as three pieces of host arithmetic -- the reference, the yardstick (tests/plain.py at the kernel's precision) and
the way a result is split for tests/accuracy.py.  Nothing here touches the GPU.

Reference: the pinned float64 oracle for a float32 case; tests/plain.py at long double for a float64 one."""
import numpy as np

import const_probe as cp
import linear_cases as lc
import maskfilter_cases as mc
import plain
import route_cases as rc
from oracle import zaf_oracle as orc

PROBE_ROUTES = [r for r in cp.ROUTES if not r.startswith("center_")]   # (the center mask: its yardstick divides near 0 / 0)


def is_pow2(n):
    return n > 0 and not n & (n - 1)


def bluestein(kernel, window_length=0):
    """The routes that run three transforms of >= 2 W points and two chirp products: k_*_bs32, k_*_bs_f64, the k_dct Bluestein forms, and a
    window that is no power of two under any other name (the spectrum kernel in front of k_melfb is k_stft_bs32 then)."""
    return "_bs" in kernel or (window_length > 0 and not is_pow2(window_length))


# A case above the family's factor: {case: (factor, cause)}.  Never above accuracy.MAX_FACTOR, every cause also in DESIGN 1.
OWN_FACTORS = {
    # k_linear sums a row's products as ONE k-ordered fmaf chain (v_mfma_f32_16x16x4_f32: bit for bit fma(a_k, b_k, acc), no wider internal
    # sum), the documented arithmetic of the float32 matrix core.  np.matmul on the case's two vectors runs BLAS's vector form, 8 interleaved
    # partial sums: a chain of n terms carries sqrt(8) = 2.83 times the rounding of 8 chains of n / 8.  Emulated on the host, the single chain
    # gives the kernel's four numbers to all digits (ratios 3.49 / 2.27 / 1.01 / 2.49), 8 chains give 1.23 / 0.99 / 0.83 / 1.01, and np.matmul
    # on 400 vectors (BLAS's matrix form: one chain) is the single chain bit for bit.  K_RMS * sqrt(8) = 5.7, rounded up.
    # k_cqt below 32768 points (fft_frame_chain) and its 65536 double form take every twiddle from a two-level root table and a product tree
    # of depth 4 (zafx_fft.hpp: "a few ulp; the CQT tolerance is 1e-4"): w^r = w^(r / 2) w^(r - r / 2) carries r times the rounding of
    # w = hi * lo, r up to 15 (rms 8.8), where a pass table holds ONE rounded root -- a twiddle error about 15 times a table's in two of the
    # three passes at 4096 points, by which a pass's rounding (the twiddle's a sixth of it) grows 6-fold and the transform's 5-fold; K_RMS
    # times that is above MAX_FACTOR, so the cap.  tests/host_emu/fft_emu.cpp in its chain mode measures the core alone at 4.28 (rms) / 6.84
    # (max) of the yardstick at 4096 points against 1.01 / 0.92 with pass tables (tests/test_accuracy_host.py); behind the contraction the
    # cases measure 1.56 (cqt_8192, inside the family factor), 2.42 (chroma_8192) and 2.84 rms / 3.12 row (cqt_65536: b1^2, the tree, then
    # one more product with b1).  The 32768 form chains its first pass only and measures 1.04.
    "const/chroma_8192": (8.0, "chained twiddles of fft_frame_chain: w^r by a product tree carries r times the rounding of w"),
    "const/cqt_65536": (8.0, "chained twiddles of the double form's first pass: (b1^2)^r b1 by a product tree"),
    "const/linear": (6.0, "one k-ordered fmaf chain per output (float32 MFMA) against BLAS's 8 partial sums at this shape"),
}


# ------------------------------------------------------------------------------------------------ tests/const_probe.py
def probe_plain(case, dtype, consts=None):
    """The case's operation by tests/plain.py -> the clips' results as case.bind(plan)["split"] gives the kernel's."""
    c, kw, x = consts or case.consts, case.kw, case.data
    if case.kind == "STFT":
        return list(plain.stft(x, c["window"], kw["step_length"], dtype, kw["onesided"]))
    if case.kind == "ISTFT":
        return list(plain.istft(x, c["window"], kw["step_length"], dtype, kw["onesided"]))
    if case.kind == "MDCT":
        return list(plain.mdct(x, c["window"], dtype))
    if case.kind == "IMDCT":
        return list(plain.imdct(x, c["window"], dtype))
    if case.kind == "MEL":
        return list(plain.melspectrogram(x, c["window"], kw["step_length"], c["fb"], dtype))
    if case.kind == "MFCC":
        return list(plain.mfcc(x, c["window"], kw["step_length"], c["fb"], c["dct"], dtype, also_mel=kw["with_mel"]))
    if case.kind == "CQT":
        return list(plain.cqtspectrogram(x, kw["step_length"], c["cqt"], dtype))
    if case.kind == "CHROMA":
        return list(plain.cqtchromagram(x, kw["step_length"], kw["octave_resolution"], c["cqt"], dtype))
    if case.kind == "LINEAR":
        return list(plain.linear(x, c["matrix"], dtype))
    raise KeyError(case.kind)


def probe_f64(case):
    return bool(case.kw.get("f64"))


def probe_hop(case):
    """Block length of a 1-D result (None: the result is rows x frames)."""
    return case.kw["step_length"] if case.kind == "ISTFT" else case.kw["window_length"] // 2 if case.kind == "IMDCT" else None


def probe_window(case):
    """The window length of a windowed case (what tells a Bluestein route under another kernel's name), 0 for CQT and LINEAR."""
    return case.kw["window_length"] if case.kind in ("STFT", "ISTFT", "MDCT", "IMDCT", "MEL", "MFCC") else 0


def as_measured(case_kind, clips):
    """The clips' results as tests/accuracy.measure takes them: a LINEAR / DCT result (one vector per clip) becomes one (rows, clips) array."""
    if case_kind in ("LINEAR", "DCT"):
        return [np.stack([np.asarray(v) for v in clips], axis=1)]
    return [np.asarray(v) for v in clips]


def probe_reference(case):
    return probe_plain(case, np.longdouble) if probe_f64(case) else case.refs(None)


def probe_yardstick(case):
    return probe_plain(case, np.float64 if probe_f64(case) else np.float32)


# ------------------------------------------------------------------------------------------------ tests/route_cases.py
def route_consts(c):
    """The constants route_cases.make_plan uploads, as the float32 plan holds them."""
    import zafx
    from zafx import constants
    w = c["W"]
    out = {"window": cp.f32(zafx.sine(w) if c["family"] in ("mdct", "imdct") else zafx.hamming(w))}
    if c["filters"]:
        out["fb"] = cp.f32(zafx.melfilterbank(rc.FS, w, c["filters"]).toarray())
    if c["ncoef"]:
        out["dct"] = cp.f32(constants.dct2_rows(c["filters"], c["ncoef"]))
    return out


def route_input(c, x, n_in, pitch=None):
    """run's input array as (clips, samples) float32 -- PCM as x / 32768, exact in float32 -- or the compact (clips, rows, frames) blocks of an
    inverse case (a row's pad columns, which run fills with noise, dropped)."""
    if c["pcm"]:
        return (x.astype(np.float32) / np.float32(32768.0)).reshape(rc.N_CLIPS, n_in)
    if not rc.is_inverse(c):
        return x.reshape(rc.N_CLIPS, n_in)
    rows = c["W"] // 2 if c["family"] == "imdct" else c["W"] // 2 + 1 if c["spectrum"] else c["W"]
    if c["layout"] == "FT":
        return np.ascontiguousarray(x.reshape(rc.N_CLIPS, rows, rc.pitch(c, n_in) if pitch is None else pitch)[:, :, :n_in])
    return np.ascontiguousarray(x.reshape(rc.N_CLIPS, n_in, rows).transpose(0, 2, 1))


def route_output(c, keep):
    """The clips' results out of the output bytes of route_cases.run."""
    nbytes = int(np.prod(keep["out_shape"])) * np.dtype(keep["out_dtype"]).itemsize
    out = np.frombuffer(keep["out"], np.uint8)[c["out_delta"]:c["out_delta"] + nbytes].view(keep["out_dtype"]).reshape(keep["out_shape"])
    if rc.is_inverse(c):
        return [out[b] for b in range(rc.N_CLIPS)]
    if c["layout"] == "FT":
        return [out[b, :, :c["frames"]] for b in range(rc.N_CLIPS)]
    return [out[b].T for b in range(rc.N_CLIPS)]


def route_plain(c, x, dtype, consts):
    f, w, h = c["family"], consts["window"], c["hop"]
    if f == "stft":
        return list(plain.stft(x, w, h, dtype, c["spectrum"]))
    if f == "istft":
        return list(plain.istft(x, w, h, dtype, bool(c["spectrum"])))
    if f == "mdct":
        return list(plain.mdct(x, w, dtype))
    if f == "imdct":
        return list(plain.imdct(x, w, dtype))
    if f == "mel":
        return list(plain.melspectrogram(x, w, h, consts["fb"], dtype))
    if f == "mfcc":
        return list(plain.mfcc(x, w, h, consts["fb"], consts["dct"], dtype))
    raise KeyError(f)


def route_reference(c, x, consts):
    """The pinned float64 oracle on the float32 input."""
    f, w, h = c["family"], consts["window"], c["hop"]
    x = np.asarray(x, np.complex128 if np.iscomplexobj(x) else np.float64)
    if f == "stft":
        full = orc.stft_batch(x, w, h)
        if c["spectrum"] is False:
            return list(full)
        half = full[:, :c["W"] // 2 + 1]
        return list(half if c["spectrum"] is True else np.abs(half) if c["spectrum"] == "magnitude" else np.abs(half) ** 2)
    if f == "istft":
        if c["spectrum"]:
            x = np.concatenate([x, np.conj(x[:, -2:0:-1])], axis=1)
        return [orc.istft(s, w, h) for s in x]
    if f == "mdct":
        return list(orc.mdct_batch(x, w))
    if f == "imdct":
        return [orc.imdct(k, w) for k in x]
    return cp.mel_ref(x, h, f == "mfcc")(consts)


def route_hop(c):
    return c["hop"] if rc.is_inverse(c) else None


# ------------------------------------------------------------------------------------------------ added here
N_ROWS = 8
DCT_LENGTHS = (64, 1024, 100, 132, 134)


def dct_kernel(n, t, sine):
    """The rule of zafx.dct_plan: k_dct where N / 2 (type 1: N - 1 / N + 1) is a power of two from 32 up; off that grid types 2-4 of a length
    4 j keep k_dct's maps around an N/2-point Bluestein convolution (k_dct_bsh), everything else is the chirp-z sum (k_dct_bs32)."""
    m = (n + 1 if sine else n - 1) if t == 1 else (n // 2 if n % 2 == 0 else 0)
    if 32 <= m <= 8192 and is_pow2(m):
        return "k_dct"
    return "k_dct_bsh" if t >= 2 and n % 4 == 0 else "k_dct_bs32"


def dct_cases():
    """name -> (n, type, sine, kernel): dct and dst, types 1-4.  64 and 1024: k_dct for types 2-4 (type 1 runs the chirp-z form there);
    100 and 132, both 4 j: k_dct_bsh for types 2-4, k_dct_bs32 for type 1; 134: k_dct_bs32 for every type."""
    return {f"{'dst' if sine else 'dct'}{t}_{n}": (n, t, sine, dct_kernel(n, t, sine))
            for n in DCT_LENGTHS for sine in (False, True) for t in (1, 2, 3, 4)}


DCT_CASES = dct_cases()


def dct_input(n):
    return cp.clips_of(900 + n, n, count=N_ROWS)


def dct_reference(x, t, sine):
    return [(orc.dst if sine else orc.dct)(v.astype(np.float64), t) for v in x]


def dct_plain(x, t, sine, dtype):
    return list((plain.dst if sine else plain.dct)(x, t, dtype))


# ------------------------------------------------------------------------------------------------ tests/linear_cases.py
# The table's cases and the dense dct-II at N = 8224, judged against plain.linear_chain: ONE k-ordered float32 chain per output, which is what
# both kernels of zafx_linear.hip compute (OWN_FACTORS above) -- at rows of thousands of columns np.matmul lies 4 ... 9 times BELOW any
# single chain (blocked partial sums), past MAX_FACTOR, and is no yardstick for them.  Family factors, no entry in OWN_FACTORS; const/linear
# keeps np.matmul and its own factor.
DCT2_DENSE = "dct2_%d" % lc.DCT_N
LINEAR_NAMES = [lc.name_of(c) for c in lc.CASES] + [DCT2_DENSE]


def linear_case(name):
    """-> (every clip of the launch, the float32 matrix, the judged clips' indices, their float64 reference, the kernel of the launch).
    DCT2_DENSE: the launch is zafx.dct_batch(clips, 2); the matrix is the one core._transform_batch uploads, the reference the oracle's dct."""
    if name == DCT2_DENSE:
        from zafx import constants
        x = lc.dct_clips()
        pick = np.arange(lc.DCT_DISTINCT)
        ref = np.stack([orc.dct(v.astype(np.float64), 2) for v in x[pick]])
        return x, constants.dct_matrix(lc.DCT_N, 2).astype(np.float32), pick, ref, lc.kernel(lc.DCT_N, lc.DCT_N, lc.DCT_CLIPS)
    rows, cols, count = lc.CASES[LINEAR_NAMES.index(name)]
    x, m, pick = lc.clips(rows, cols, count), lc.matrix(rows, cols), lc.judged(count)
    return x, m, pick, lc.reference(x[pick], m), lc.kernel(rows, cols, count)


# ------------------------------------------------------------------------------------------------ tests/maskfilter_cases.py
# The eight fused float32 STFT-mask-ISTFT kernels: 7 forms (the stereo kind's two among them) x W = 256 ... 2048 x T = 62 / 63 x with and
# without the rest, each through its equal-length launch ("maskfilter/<case>") and, with clips of 1, H, 3 H + 7 and 0 samples between the same
# clips, through its ragged one ("maskfilter/<case>/ragged").  Reference: the float64 oracle's composition; yardstick: plain.maskfilter* at
# float32 -- unpacked, one frame per transform, where the kernels ride two frames (the stereo kernels: the two channels of a frame) in one
# transform and split them.  Every stem of every clip, every channel of a stereo clip, and the rest, is a 1-D result of its own; the block
# length of e_row / e_col is the hop.  Family factors, no entry in OWN_FACTORS.
MASKFILTER_NAMES = list(mc.ACCURACY_CASES)


def maskfilter_case(name):
    """-> (form, W, rest, the batch, its ragged twin, the twin's index of each clip of the batch)."""
    form, wl, _, rest = mc.ACCURACY_CASES[name]
    b, e = mc.accuracy_batch(name)
    twin, where = mc.ragged_twin(b, e)
    return form, wl, rest, b, twin, where


# Cases built like those of tests/const_probe.py.  float64 Bluestein at W = 1000: the library's only device-side trigonometry (sincospi in
# zafx_f64.hip).  mel_1024: k_mel's melspectrogram -- the catalogue reaches k_mel through an MFCC alone, and an MFCC hides a spectrum's
# error behind the rounding of its logarithms (with every root of unity rounded to 18 bits the MFCC cases stay inside their factors).
ADDED_PROBES = {
    "stft_bs_f64": lambda: cp.stft_case(1000, 500, "k_stft_bs_f64", f64=True),
    "mdct_bs_f64": lambda: cp.mdct_case(1000, "k_mdct_bs_f64", f64=True),
    "mel_1024": lambda: cp.mel_case(1024, 256, 64, None, "k_mel", fs=22050),
}
