"""Cases of tests/test_gpu_constants.py: one kernel route each on a private plan whose constants are replaced between executes.

A case holds the plan's geometry, its constants A (a dict: window / fb / dct / matrix / cqt), the host input, the float64 reference as a
function of the constants, and the kernel a fresh plan must report.  A variant is the list of uploads that turn A into B, in order.  Nothing
here touches the GPU until a plan is made: every reference (and the condition that B's differs from A's by 0.1 or more) is host arithmetic.

Shapes: 2 clips of seeded float32-rounded unit noise (conftest.synth_clip); one whole tile of the route plus 3 frames (19 STFT frames, 35
MDCT frames, 11 float64 STFT frames) at a clip length that is no multiple of the hop; center: one tile of hops plus 300 samples; CQT: 5 frames
and half a step.  Every constant is float32-exact."""
import os

import numpy as np
import scipy.sparse

import windows as win
from conftest import relerr, synth_clip
from oracle import zaf_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CLIPS = 2
FS = 44100
TOL_FFT, TOL_FB, TOL_F64, TOL_F64_MFCC = 1e-5, 1e-4, 1e-12, 1e-10   # the project's bounds (tests/test_gpu_parity.py, include/zafx.h)
MIN_CHANGE = 0.1   # relerr(ref_B, ref_A) of every variant, every clip: no case passes by ignoring the upload


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def c64(a):
    return np.asarray(a, np.complex128).astype(np.complex64).astype(np.complex128)


def lib():
    from zafx import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ the constants
def window_a(w, mdct=False):
    return f32(orc.kbd_window(w) if mdct else orc.hamming_periodic(w))


def window_zero_gain(w, hop):
    """Window A with w[0] = -w[hop]: sum(w[0:W:H]) is exactly 0 at hop W / 2."""
    z = window_a(w).copy()
    z[0] = -z[hop]
    assert win.cola_gain(z, hop) == 0.0
    return z


def fb_mel(fs, w, n):
    return f32(orc.melfilterbank(fs, w, n).toarray())


def fb_empty_block(fs, w, n):
    """Filterbank A with rows 16 .. 31 zero: a 16-row block without non-zeros."""
    fb = fb_mel(fs, w, n)
    fb[16:32] = 0.0
    return fb


def fb_dense(w, n):
    """Seeded uniform(0.5, 1.5): every 16-row block is full width."""
    return f32(np.random.default_rng([5, w, n]).uniform(0.5, 1.5, (n, w // 2)))


def dct_a(n, ncoef):
    from zafx import constants
    return f32(constants.dct2_rows(n, ncoef))


def dct_b(n, ncoef):
    return f32(0.5 * dct_a(n, ncoef)[::-1])


def cqt_recipe(which):
    """-> fs, frames per second, bins per octave, kernel A, kernel B3 (same shape, another nnz)."""
    if which == "tiny":
        g = np.load(os.path.join(ROOT, "tests", "golden", "tiny.npz"))
        a = scipy.sparse.csr_matrix(g["ck_dense"])
        rows, cols = a.shape
        dense = np.zeros((rows, cols), np.complex128)   # B3: the rows in reverse order, each without its largest entry
        for r in range(rows):
            row = a.getrow(rows - 1 - r).toarray()[0]
            row[np.argmax(np.abs(row))] = 0.0
            dense[r] = row
        return 4000, 50, 12, a, scipy.sparse.csr_matrix(dense)
    if which == "8192":
        return 22050, 25, 12, orc.cqtkernel(22050, 12, 55, 7000), orc.cqtkernel(22050, 12, 60, 7680)
    if which == "65536":
        return FS, 10, 24, orc.cqtkernel(FS, 24, 27.5, 880.0), None
    return FS, 25, 24, orc.cqtkernel(FS, 24, 55, 3520), orc.cqtkernel(FS, 24, 50, 3200)   # fft_length 32768


def cqt_round(ck, f64):
    """The CSR kernel with sorted indices and, for a float32 plan, complex64-exact values."""
    ck = scipy.sparse.csr_matrix(ck, dtype=np.complex128)
    ck.sort_indices()
    if not f64:
        ck.data = c64(ck.data)
    return ck


def cqt_values_scaled(ck, f64):
    """B1: every value times a seeded factor in [0.5, 1.5] -- one of the two ends, entry by entry: uniform factors average out over a row's
    entries (and over a chroma's bins) to a change of the result just under MIN_CHANGE."""
    b = ck.copy()
    b.data = b.data * np.random.default_rng([6, ck.nnz]).choice([0.5, 1.5], ck.nnz)
    return cqt_round(b, f64)


def cqt_values_complex(ck):
    """B2: every value times (1 + 0.5j): no longer numerically real."""
    b = ck.copy()
    b.data = b.data * (1 + 0.5j)
    return cqt_round(b, False)


# ------------------------------------------------------------------------------------------------ the machinery
class Case:
    """kind: name of the plan kind in zafx._lib; kw: Plan's keyword arguments; consts: constants A in upload order; ref(consts) -> the clips'
    float64 results; bind(plan) -> x, out_shape, launch, split, keep (as tests/cu_probe.py); variants: name -> [(key, value), ...]; data: the
    host input without a plan's row padding -- the clips, or the compact (B, rows, frames) blocks of an inverse case (tests/accuracy_cases.py)."""

    def __init__(self, kind, kw, consts, ref, bind, tol, kernel, variants, err=relerr, data=None):
        self.kind, self.kw, self.consts, self.ref, self.bind, self.tol, self.kernel, self.variants, self.err = kind, kw, consts, ref, bind, tol, kernel, variants, err
        self.data = data
        self.oracle_rows = {}   # variant -> the leading rows of a result that are held to the oracle (mel_case); absent: all of them
        self._refs = {}

    def after(self, steps):
        out = dict(self.consts)
        for key, value in steps:
            out["cqt" if key == "cqt_values" else key] = value
        return out

    def restore(self, steps):
        return [(key, self.consts["cqt" if key == "cqt_values" else key]) for key, _ in steps]

    def refs(self, name):
        """References under constants A (name None) or under a variant, computed once."""
        if name not in self._refs:
            self._refs[name] = self.ref(self.consts if name is None else self.after(self.variants[name]))
        return self._refs[name]

    def make(self, consts=None):
        """A private plan (never the cached factories) with the constants uploaded in their order."""
        import zafx
        plan = zafx.Plan(getattr(lib(), self.kind), **self.kw)
        try:
            upload(plan, (consts or self.consts).items())
        except Exception:
            plan.destroy()
            raise
        return plan


def upload(plan, steps):
    for key, value in steps:
        if key == "window":
            plan.set_window(value)
        elif key == "fb":
            plan.set_mel_filterbank(value)
        elif key == "dct":
            plan.set_dct(value)
        elif key == "matrix":
            plan.set_matrix(value)
        elif key == "cqt":
            plan.set_cqt_kernel(value)
        elif key == "cqt_values":   # the values alone: indptr and indices stay
            plan._set(lib().CONST_CQT_VALUES, value.data, np.complex128 if plan.f64 else np.complex64)
        else:
            raise KeyError(key)


def clips_of(seed, n, dtype=np.float32, count=N_CLIPS):
    return np.stack([synth_clip(seed, c, n) for c in range(count)]).astype(dtype)


def rows_with_nan_pads(blocks, pitch, dtype):
    blocks = np.asarray(blocks)
    x = np.full(blocks.shape[:2] + (pitch,), np.nan, dtype)
    x[:, :, :blocks.shape[2]] = blocks
    return x


def forward_bind(x, n, frames, layout="FT"):
    def bind(plan):
        shape = plan.out_shape(len(x), n)
        rows, t = plan.out_dims(n)
        assert t == frames, (t, frames)
        split = (lambda out: [out[c, :, :t] for c in range(len(x))]) if layout == "FT" else (lambda out: [out[c].T for c in range(len(x))])
        keep = None
        if layout == "FT" and shape[-1] != t:
            keep = np.zeros(shape, bool)
            keep[:, :, :t] = True
        return dict(x=x, out_shape=shape, launch=lambda p, d_in, d_out: p.execute(d_in, d_out, len(x), n), split=split, keep=keep)
    return bind


def inverse_bind(blocks, frames, dtype):
    def bind(plan):
        x = rows_with_nan_pads(blocks, plan.row_pitch(frames), dtype)
        return dict(x=x, out_shape=plan.out_shape(len(blocks), frames), launch=lambda p, d_in, d_out: p.execute(d_in, d_out, len(blocks), frames),
                    split=lambda out: [out[c] for c in range(len(blocks))], keep=None)
    return bind


def nan_filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.float64 if np.dtype(dtype).itemsize % 8 == 0 and np.dtype(dtype) != np.complex64 else np.float32).fill(np.nan)
    return a


def scalars_of(out):
    return out.view(np.float64 if out.dtype.itemsize % 8 == 0 and out.dtype != np.complex64 else np.float32).reshape(-1)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def stft_n(w, hop, frames):
    """A clip length that gives `frames` frames and is no multiple of the hop (even: the kernels' 8-byte loads)."""
    n = (frames - 2) * hop + (300 % hop or 2)
    assert orc.stft_num_frames(n, w, hop) == frames and n % hop, (n, w, hop, frames)
    return n


# ------------------------------------------------------------------------------------------------ window kinds
def window_variants(w):
    return {"window": [("window", win.skew(w))]}


def stft_case(w, hop, kernel, row_align=0, layout="FT", onesided=False, f64=False, frames=None):
    frames = frames or (11 if f64 else 19)
    n = stft_n(w, hop, frames)
    x = clips_of(w + hop, n, np.float64 if f64 else np.float32)

    def ref(c):
        full = orc.stft_batch(x.astype(np.float64), c["window"], hop)
        if onesided is False:
            return list(full)
        half = full[:, :w // 2 + 1]
        return list(half if onesided is True else np.abs(half) if onesided == "magnitude" else np.abs(half) ** 2)
    kw = dict(window_length=w, step_length=hop, layout=layout, onesided=onesided, f64=f64, row_align=row_align)
    return Case("STFT", kw, {"window": window_a(w)}, ref, forward_bind(x, n, frames, layout), TOL_F64 if f64 else TOL_FFT, kernel, window_variants(w),
                data=x)


def istft_case(w, hop, kernel, row_align=0, onesided=False, f64=False, frames=None, zero_gain=False):
    frames = frames or (11 if f64 else 19)
    n = stft_n(w, hop, frames)
    a = window_a(w)
    assert abs(win.cola_gain(win.skew(w), hop)) >= win.MIN_COLA and abs(win.cola_gain(a, hop)) >= win.MIN_COLA
    dtype = np.complex128 if f64 else np.complex64
    spec = orc.stft_batch(clips_of(3 * w + hop, n).astype(np.float64), a, hop).astype(dtype)   # (the input stays; only the plan's window changes)
    if onesided:
        spec = np.ascontiguousarray(spec[:, :w // 2 + 1])

    def ref(c):
        full = spec.astype(np.complex128)
        if onesided:
            full = np.concatenate([full, np.conj(full[:, -2:0:-1])], axis=1)
        return [orc.istft(s, c["window"], hop) for s in full]
    variants = window_variants(w)
    if zero_gain:
        variants["zero_gain"] = [("window", window_zero_gain(w, hop))]
    kw = dict(window_length=w, step_length=hop, onesided=onesided, f64=f64, row_align=row_align)
    return Case("ISTFT", kw, {"window": a}, ref, inverse_bind(spec, frames, dtype), TOL_F64 if f64 else TOL_FFT, kernel, variants, data=spec)


def mdct_case(w, kernel, row_align=0, f64=False, frames=None):
    frames = frames or (19 if f64 else 35)
    m = w // 2
    n = (frames - 2) * m + 4   # (a multiple of four samples: the 16-byte loads of the tiled forms; no multiple of the hop)
    assert orc.mdct_num_frames(n, w) == frames and n % m
    x = clips_of(w + 1, n, np.float64 if f64 else np.float32)
    ref = lambda c: list(orc.mdct_batch(x.astype(np.float64), c["window"]))
    return Case("MDCT", dict(window_length=w, row_align=row_align, f64=f64), {"window": window_a(w, True)}, ref, forward_bind(x, n, frames),
                TOL_F64 if f64 else TOL_FFT, kernel, window_variants(w), data=x)


def imdct_case(w, kernel, row_align=0, f64=False, frames=None):
    frames = frames or (19 if f64 else 35)
    m = w // 2
    a = window_a(w, True)
    dtype = np.float64 if f64 else np.float32
    coefs = orc.mdct_batch(clips_of(w + 2, (frames - 1) * m - 3).astype(np.float64), a).astype(dtype)
    assert coefs.shape[2] == frames
    ref = lambda c: [orc.imdct(k.astype(np.float64), c["window"]) for k in coefs]
    return Case("IMDCT", dict(window_length=w, row_align=row_align, f64=f64), {"window": a}, ref, inverse_bind(coefs, frames, dtype),
                TOL_F64 if f64 else TOL_FFT, kernel, window_variants(w), data=coefs)


# ------------------------------------------------------------------------------------------------ mel / mfcc
def mel_ref(x, hop, mfcc, also_mel=False):
    def ref(c):
        w = len(c["window"])
        spec = orc.stft_batch(x.astype(np.float64), c["window"], hop)[:, 1:w // 2 + 1]
        mel = [c["fb"] @ np.abs(s) for s in spec]
        if not mfcc:
            return mel
        # zaf.py:436-452 with the plan's own rows D in place of scipy's DCT-II rows 1 .. n (the reference fixes D; here it is a constant)
        cep = [c["dct"] @ np.log(c["fb"] @ np.abs(s) ** 2 + np.finfo(float).eps) for s in spec]
        return [np.concatenate([a, b]) for a, b in zip(mel, cep)] if also_mel else cep
    return ref


def mel_case(w, hop, n_mel, n_coef, kernel, fs=FS, f64=False, also_mel=False, row_align=0, extra_fb=(), frames=None):
    """n_coef None: melspectrogram.  Variants: window, fb (the 16 kHz filterbank), dct, both orders of fb and dct, and the filterbanks named in
    extra_fb ("empty_block", "dense")."""
    frames = frames or (11 if f64 else 19)
    n = stft_n(w, hop, frames)
    x = clips_of(w + n_mel, n, np.float64 if f64 else np.float32)
    mfcc = n_coef is not None
    consts = {"window": window_a(w), "fb": fb_mel(fs, w, n_mel)}
    fb_b = fb_mel(16000, w, n_mel)
    assert fb_b.shape == consts["fb"].shape
    # Window B of the MFCC plans is tests/windows.py's `random`, not `skew`: white noise has a flat spectrum under any window, a smooth window
    # only moves the level of every band alike, and that goes into the coefficient the MFCC drops (row 0 of the DCT): the MFCCs under hamming
    # and under skew differ by 0.08 ... 0.12 only.  `random` (no mirror symmetry either) gives every band another realisation of the noise.
    variants = {"window": [("window", win.random(w) if mfcc else win.skew(w))], "fb": [("fb", fb_b)]}
    if mfcc:
        consts["dct"] = dct_a(n_mel, n_coef)
        d_b = dct_b(n_mel, n_coef)
        variants.update({"dct": [("dct", d_b)], "fb_then_dct": [("fb", fb_b), ("dct", d_b)], "dct_then_fb": [("dct", d_b), ("fb", fb_b)]})
    if "empty_block" in extra_fb:
        variants["fb_empty_block"] = [("fb", fb_empty_block(fs, w, n_mel))]
    if "dense" in extra_fb:
        variants["fb_dense"] = [("fb", fb_dense(w, n_mel))]
    kw = dict(window_length=w, step_length=hop, n_filters=n_mel, n_coefs=n_coef or 0, f64=f64, with_mel=also_mel, row_align=row_align)
    tol = (TOL_F64_MFCC if mfcc else TOL_F64) if f64 else TOL_FB
    # the one-pass plan's rows are the melspectrogram's, then the MFCCs': each part against its own level (the MFCCs are a tenth of the other's)
    err = (lambda val, r: max(relerr(val[:n_mel], r[:n_mel]), relerr(val[n_mel:], r[n_mel:]))) if also_mel else relerr
    case = Case("MFCC" if mfcc else "MEL", kw, consts, mel_ref(x, hop, mfcc, also_mel), forward_bind(x, n, frames), tol, kernel, variants, err=err, data=x)
    if mfcc and not f64 and "dense" in extra_fb:
        # Under the dense filterbank every band holds the whole spectrum: the log-mel values are all about 14 and differ by a hundredth, the
        # DCT's rows 1 .. n cancel the common level, and the MFCCs come out at 0.05 -- float32's rounding of the logs alone is 1e-4 of that, and
        # a fresh plan measures 2.75e-4 against the oracle.  TOL_FB was not set for such a constant, so the float32 MFCC rows under it are held to
        # the fresh plan's bits, kernel and NaN pattern only; the melspectrogram rows of the one-pass plan, and the float64 plans, to the oracle.
        case.oracle_rows["fb_dense"] = n_mel if also_mel else 0
    return case


# ------------------------------------------------------------------------------------------------ center / sides
def stereo(seed, n):
    """tests/test_gpu_center.py's stereo noise: a common part and two uncorrelated ones."""
    g = np.random.default_rng([909, seed])
    c, n1, n2 = g.standard_normal(n), g.standard_normal(n), g.standard_normal(n)
    return np.stack([c + 0.5 * n1, 0.8 * c + 0.5 * n2], axis=1).astype(np.float32)


def center_err(sides):
    """tests/center_oracle.py's bounds: the center normwise, the sides against the input's level."""
    def err(val, r):
        if not sides:
            return relerr(val, r)
        if not r.size:
            return 0.0
        level = float(np.abs(r[0] + r[1]).max())
        return max(relerr(val[0], r[0]), float(np.abs(val[1] - r[1]).max()) / level)
    return err


def center_refs(xs, window, sides):
    from center_oracle import oracle_center
    center = [oracle_center(c, window) for c in xs]
    return [np.stack([c, xc.astype(np.float64) - c]) for c, xc in zip(center, xs)] if sides else center


def center_case(w, sides):
    from center_oracle import TOL_CENTER
    f = 4 if w >= 2048 else 8   # center_tile_frames (zafx_center.hpp)
    h = w // 2
    n = f * h + 300
    x = np.stack([stereo(w + c, n) for c in range(N_CLIPS)])
    assert abs(win.cola_gain(win.skew(w), h)) >= win.MIN_COLA

    def bind(plan):
        import zafx
        assert zafx.center_tile_frames(w) == f
        return dict(x=x, out_shape=plan.out_shape(N_CLIPS, n), launch=lambda p, d_in, d_out: p.execute(d_in, d_out, N_CLIPS, n),
                    split=lambda out: [out[c] for c in range(N_CLIPS)], keep=None)
    variants = {"window": [("window", win.skew(w))], "zero_gain": [("window", window_zero_gain(w, h))]}
    return Case("CENTER_SIDES" if sides else "CENTER", dict(window_length=w, step_length=h), {"window": window_a(w)},
                lambda c: center_refs(x, c["window"], sides), bind, TOL_CENTER, "k_center", variants, err=center_err(sides))


# ------------------------------------------------------------------------------------------------ CQT / chroma, LINEAR
def cqt_case(which, chroma, kernel, f64=False):
    fs, tr, res, ck, ck3 = cqt_recipe(which)
    ck = cqt_round(ck, f64)
    step = round(fs / tr)
    n = 5 * step + step // 2
    x = clips_of(len(which) + 70, n, np.float64 if f64 else np.float32)
    x64 = x.astype(np.float64)
    ref = lambda c: [orc.cqtchromagram(s, fs, tr, res, c["cqt"]) if chroma else orc.cqtspectrogram(s, fs, tr, c["cqt"]) for s in x64]
    variants = {"values": [("cqt_values", cqt_values_scaled(ck, f64))]}
    if not f64 and ck3 is not None:
        variants["values_complex"] = [("cqt_values", cqt_values_complex(ck))]
    if ck3 is not None:
        ck3 = cqt_round(ck3, f64)
        assert ck3.shape == ck.shape and ck3.nnz != ck.nnz, (ck3.shape, ck.shape, ck3.nnz, ck.nnz)
        variants["kernel"] = [("cqt", ck3)]
    kw = dict(step_length=step, fft_length=ck.shape[1], n_bins=ck.shape[0], octave_resolution=res if chroma else 0, f64=f64)
    return Case("CHROMA" if chroma else "CQT", kw, {"cqt": ck}, ref, forward_bind(x, n, 5), TOL_F64 if f64 else TOL_FB, kernel, variants, data=x)


def linear_case():
    rows, cols = 64, 100
    g = np.random.default_rng([8, rows, cols])
    a, b = f32(g.standard_normal((rows, cols))), f32(g.standard_normal((rows, cols)))
    x = clips_of(77, cols)

    def bind(plan):
        return dict(x=x, out_shape=(N_CLIPS, rows), launch=lambda p, d_in, d_out: p.execute(d_in, d_out, N_CLIPS, cols),
                    split=lambda out: [out[c] for c in range(N_CLIPS)], keep=None)
    return Case("LINEAR", dict(window_length=cols, n_filters=rows), {"matrix": a}, lambda c: [c["matrix"] @ r.astype(np.float64) for r in x], bind,
                TOL_FFT, "k_linear", {"matrix": [("matrix", b)]}, data=x)


# ------------------------------------------------------------------------------------------------ the routes
# name -> the case; the kernel is what a fresh plan must report (last_kernel) under constants A.
ROUTES = {
    "stft_ft16": lambda: stft_case(2048, 1024, "k_stft_ft16", row_align=16),
    "stft_ft16c": lambda: stft_case(2048, 1024, "k_stft_ft16c"),
    "stft_magnitude": lambda: stft_case(2048, 1024, "k_mel2", onesided="magnitude"),
    "stft_tf": lambda: stft_case(2048, 1024, "k_stft_tf", layout="TF"),
    "stft_ft16b": lambda: stft_case(4096, 2048, "k_stft_ft16b", row_align=16),
    "stft_ft16q": lambda: stft_case(8192, 4096, "k_stft_ft16q", row_align=16),
    "stft_bs32": lambda: stft_case(1000, 500, "k_stft_bs32"),
    "stft_128": lambda: stft_case(128, 64, "k_stft"),
    "istft_ft16": lambda: istft_case(2048, 1024, "k_istft_ft16", zero_gain=True),
    "istft_ft16_onesided": lambda: istft_case(2048, 1024, "k_istft_ft16", onesided=True),
    "istft_ft16d": lambda: istft_case(4096, 2048, "k_istft_ft16d"),
    "istft_ft8q": lambda: istft_case(8192, 4096, "k_istft_ft8q"),
    "istft_bs32": lambda: istft_case(1000, 500, "k_ifft_frames_bs32"),
    "istft_gather": lambda: istft_case(2048, 100, "k_ifft_frames_bs32", frames=35),   # (19 frames at hop 100 are shorter than the trim W - H)
    "mdct_ft32": lambda: mdct_case(2048, "k_mdct_ft32", row_align=32),
    "mdct_ft32_compact": lambda: mdct_case(2048, "k_mdct_ft32"),
    "mdct_4096": lambda: mdct_case(4096, "k_mdct_ft32b", row_align=32),
    "mdct_ft32q": lambda: mdct_case(8192, "k_mdct_ft32q", row_align=32),
    "mdct_bs32": lambda: mdct_case(1000, "k_mdct_bs32"),
    "mdct_128": lambda: mdct_case(128, "k_mdct"),
    "imdct": lambda: imdct_case(2048, "k_imdct", row_align=32),
    "imdct_compact": lambda: imdct_case(2048, "k_imdct"),
    "imdct_4096": lambda: imdct_case(4096, "k_imdct", row_align=32),
    "imdct_q": lambda: imdct_case(8192, "k_imdct_q", row_align=32),
    "imdct_bs32": lambda: imdct_case(1000, "k_imdct_frames_bs32"),
    "imdct_128": lambda: imdct_case(128, "k_imdct"),
    "stft_f64": lambda: stft_case(2048, 1024, "k_stft_ft8_f64", row_align=8, f64=True),
    "stft_f64_512": lambda: stft_case(512, 256, "k_stft_f64", f64=True),
    "istft_f64": lambda: istft_case(2048, 1024, "k_istft_ft8_f64", row_align=8, f64=True),
    "istft_f64_512": lambda: istft_case(512, 256, "k_ifft_frames_f64", f64=True),
    "mdct_f64": lambda: mdct_case(2048, "k_mdct_ft16_f64", row_align=16, f64=True),
    "mdct_f64_512": lambda: mdct_case(512, "k_mdct_f64", f64=True),
    "imdct_f64": lambda: imdct_case(2048, "k_imdct_ft16_f64", row_align=16, f64=True),
    "imdct_f64_512": lambda: imdct_case(512, "k_imdct_frames_f64", f64=True),
    "mel_f64": lambda: mel_case(2048, 1024, 128, None, "k_mel_ft8_f64", f64=True, extra_fb=("dense",)),
    "mfcc_f64": lambda: mel_case(2048, 1024, 128, 20, "k_mel_ft8_f64", f64=True, extra_fb=("dense",)),
    "cqt_f64": lambda: cqt_case("full", False, "k_cqt_ft_f64", f64=True),
    "cqt_f64_8192": lambda: cqt_case("8192", False, "k_cqt_f64", f64=True),
    "mel2_mel": lambda: mel_case(2048, 1024, 128, None, "k_mel2", extra_fb=("empty_block", "dense")),
    "mel2_mfcc": lambda: mel_case(2048, 1024, 128, 20, "k_mel2", extra_fb=("empty_block", "dense")),
    "mel2_both": lambda: mel_case(2048, 1024, 128, 20, "k_mel2", also_mel=True, extra_fb=("empty_block", "dense")),
    "mfcc_64": lambda: mel_case(2048, 1024, 64, 13, "k_mel2"),
    "mfcc_1024": lambda: mel_case(1024, 256, 64, 13, "k_mel", fs=22050),   # (k_mel: the item walk, the resident descriptors, the register-fed DCT)
    "mfcc_ft16b": lambda: mel_case(4096, 2048, 128, 20, "k_mel_ft16b"),
    "mel_melfb": lambda: mel_case(8192, 4096, 300, None, "k_melfb"),
    "mfcc_melfb": lambda: mel_case(8192, 4096, 300, 20, "k_melfb"),
    "mfcc_bluestein": lambda: mel_case(1764, 441, 64, 13, "k_melfb"),
    "cqt_tiny": lambda: cqt_case("tiny", False, "k_cqt"),
    "cqt_8192": lambda: cqt_case("8192", False, "k_cqt"),
    "chroma_8192": lambda: cqt_case("8192", True, "k_cqt"),
    "cqt_split": lambda: cqt_case("full", False, "k_cqt"),
    "chroma_split": lambda: cqt_case("full", True, "k_cqt"),
    "cqt_65536": lambda: cqt_case("65536", False, "k_cqt"),
    "center_2048": lambda: center_case(2048, False),
    "center_sides_2048": lambda: center_case(2048, True),
    "center_sides_256": lambda: center_case(256, True),
    "linear": linear_case,
}

# the variants of a route that are refusals, not replacements (test_zero_gain_refused)
REFUSALS = ("zero_gain",)
# one case per family also runs with the upload enqueued behind step 1's execute, before its result is downloaded
ASYNC = {"stft_ft16": "window", "istft_ft16": "window", "mdct_ft32": "window", "imdct": "window", "stft_f64": "window", "mel2_mfcc": "fb_then_dct",
         "cqt_8192": "values", "cqt_f64": "values", "center_sides_2048": "window", "linear": "matrix"}


WINDOW = ("window",)
MEL = ("window", "fb")
MFCC = MEL + ("dct", "fb_then_dct", "dct_then_fb")
# route -> its replacements by name (what the test is parametrised over: building a case costs host transforms, so collection builds none;
# case() checks the table against the case)
VARIANTS = {r: WINDOW for r in ROUTES if r.split("_")[0] in ("stft", "istft", "mdct", "imdct", "center")}
VARIANTS.update({
    "mel_f64": MEL + ("fb_dense",), "mfcc_f64": MFCC + ("fb_dense",),
    "mel2_mel": MEL + ("fb_empty_block", "fb_dense"), "mel2_mfcc": MFCC + ("fb_empty_block", "fb_dense"), "mel2_both": MFCC + ("fb_empty_block", "fb_dense"),
    "mfcc_64": MFCC, "mfcc_1024": MFCC, "mfcc_ft16b": MFCC, "mel_melfb": MEL, "mfcc_melfb": MFCC, "mfcc_bluestein": MFCC,
    "cqt_f64": ("values", "kernel"), "cqt_f64_8192": ("values", "kernel"), "cqt_65536": ("values",), "linear": ("matrix",),
})
VARIANTS.update({r: ("values", "values_complex", "kernel") for r in ("cqt_tiny", "cqt_8192", "chroma_8192", "cqt_split", "chroma_split")})
assert set(VARIANTS) == set(ROUTES)
_CASES = {}


def case(route):
    """The route's case, built once per process: its references are shared by the tests of all its variants."""
    if route not in _CASES:
        c = ROUTES[route]()
        assert tuple(v for v in c.variants if v not in REFUSALS) == VARIANTS[route], (route, tuple(c.variants))
        _CASES[route] = c
    return _CASES[route]


def pairs():
    return [(route, v) for route, names in VARIANTS.items() for v in names]
