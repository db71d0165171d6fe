"""Child process of tests/test_gpu_compute_units.py: one kernel route on plans made under ZAFX_COMPUTE_UNITS = unset, 32, 3 and 1, in that order.

    python tests/cu_probe.py ROUTE            one JSON line per cap (and one in front of every launch), flushed
    python tests/cu_probe.py ROUTE --dry      the route's inputs, references and geometry alone (no GPU)
    python tests/cu_probe.py --list

Every cap gets a plan of its own (the plan cache is emptied first: the switch is read when a plan is created) and two launches into
NaN-filled buffers.  Reported per cap: the plan's compute units and the device's, the kernel that ran, the worst normwise error of a clip
against the float64 oracle, whether every shape is the oracle's, whether both launches gave the same bytes, and whether those are the bytes of
the uncapped plan's launch -- the whole buffer: pad columns and the gaps between ragged clips included.

Shapes (ISSUE: the smallest at which the caps bite): 7 clips of ten whole tiles of the route plus a partial one, 77 tiles -- no multiple of 32,
64, 3, 6, 1 x 11 or 2 x 11 workgroups; ragged batches: 9 clips of {0 or 1, 1, 2, 3, 5, 8, 11, 13, 21} tiles, the last one partial, packed with
gaps of 1, 3 and 5 elements; CQT: 9 clips of 20 or 21 frames (eight groups with uneven lists); DCT: 77 tiles of rows and one row.  Input:
seeded float32-rounded unit noise.  Window: tests/windows.py's skew."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "zaf-python_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
os.environ.setdefault("ZAFX_MELW_CHUNK_MB", "3")   # (read once per process: the k_melfb route in three chunks of 3, 3 and 1 clips)

import windows as win  # noqa: E402
from oracle import zaf_oracle as orc  # noqa: E402

CAPS = (None, 32, 3, 1)
N_CLIPS = 7
TOL_FFT, TOL_FB, TOL_F64 = 1e-5, 1e-4, 1e-12
RAGGED_TILES = (0, 1, 2, 3, 5, 8, 11, 13, 21)   # (clip 0: the fewest tiles the route's entry point takes, 0 or 1)
GAPS = (1, 3, 5)
FS = 44100


def synth_clip(seed, c, n):
    """conftest.synth_clip: white Gaussian noise, sigma 1, float32-rounded."""
    return np.random.default_rng([seed, c]).standard_normal(n).astype(np.float32)


def relerr(out, ref):
    """conftest.relerr: max|out - ref| / max|ref|."""
    out, ref = np.asarray(out), np.asarray(ref)
    if out.shape != ref.shape:
        return float("inf")
    if not ref.size:
        return 0.0
    denom = float(np.max(np.abs(ref))) or 1.0
    return float(np.max(np.abs(out - ref)) / denom)


def zafx():
    import zafx as z
    return z


class Case:
    """One route, ready to run.  make(): the plan (called with the cap in the environment); bind(plan) fills in what needs the plan's geometry:
    x (the host input), out_shape / out_dtype, launch(plan, d_in, d_out), split(out) -> the clips' results in the order of refs, and
    keep (bool array over the output: the elements a clip's result occupies; None: all of it)."""

    def __init__(self, make, bind, refs, tol, kernel, info, err=relerr, env=None):
        self.make, self.bind, self.refs, self.tol, self.kernel, self.info, self.err, self.env = make, bind, refs, tol, kernel, info, err, env or {}


def clips_of(seed, n, count=N_CLIPS, dtype=np.float32):
    return np.stack([synth_clip(seed, c, n) for c in range(count)]).astype(dtype)


def rows_with_nan_pads(blocks, pitch, dtype):
    """(clips, rows, T) -> (clips, rows, pitch), NaN in the pad columns (an inverse plan's input)."""
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
    """blocks: (clips, rows, T) in the plan's input dtype."""
    def bind(plan):
        x = rows_with_nan_pads(blocks, plan.row_pitch(frames), dtype)
        shape = plan.out_shape(len(blocks), frames)
        return dict(x=x, out_shape=shape, launch=lambda p, d_in, d_out: p.execute(d_in, d_out, len(blocks), frames),
                    split=lambda out: [out[c] for c in range(len(blocks))], keep=None)
    return bind


# ------------------------------------------------------------------------------------------------ equal lengths, float32 and float64
def stft_n(w, hop, frames):
    """A clip length that gives `frames` frames and is no multiple of the hop."""
    n = (frames - 2) * hop + (300 % hop or 1)
    assert orc.stft_num_frames(n, w, hop) == frames and n % hop, (n, w, hop, frames)
    return n


def stft_case(w, hop, row_align, kernel, layout="FT", tile=16, f64=False, env=None, carry=None):
    frames = 10 * tile + tile // 2 + 2
    n = stft_n(w, hop, frames)
    window = win.skew(w)
    x = clips_of(w + hop, n, dtype=np.float64 if f64 else np.float32)
    refs = list(orc.stft_batch(x.astype(np.float64), window, hop))
    make = lambda: zafx().stft_plan(window, hop, layout=layout, row_align=row_align, f64=f64)
    info = dict(tiles=N_CLIPS * -(-frames // tile), tiles_per_clip=-(-frames // tile), frames=frames, n=n)
    if carry:   # (the units carry_segments cuts: one per clip, or one per clip and band)
        info["carry"] = [carry * N_CLIPS, -(-frames // tile)]
    return Case(make, forward_bind(x, n, frames, layout), refs, TOL_F64 if f64 else TOL_FFT, kernel, info, env=env)


def istft_case(w, hop, row_align, kernel, tile=16, f64=False, units_per_clip=1):
    frames = 10 * tile + tile // 2 + 2
    n = stft_n(w, hop, frames)
    window = win.skew(w)
    assert abs(win.cola_gain(window, hop)) >= win.MIN_COLA
    dtype = np.complex128 if f64 else np.complex64
    spec = orc.stft_batch(clips_of(3 * w + hop, n).astype(np.float64), window, hop).astype(dtype)
    refs = [orc.istft(s.astype(np.complex128), window, hop) for s in spec]
    make = lambda: zafx().istft_plan(window, hop, row_align=row_align, f64=f64)
    tiles = -(-frames // tile)
    info = dict(tiles=N_CLIPS * tiles, tiles_per_clip=tiles, frames=frames, carry=[units_per_clip * N_CLIPS, tiles])
    return Case(make, inverse_bind(spec, frames, dtype), refs, TOL_F64 if f64 else TOL_FFT, kernel, info)


def mdct_case(w, row_align, kernel, tile=32, f64=False, carry=None):
    frames = 10 * tile + 2
    m = w // 2
    n = (frames - 2) * m + 4   # (a multiple of four samples: the 16-byte loads of the tiled forms)
    assert orc.mdct_num_frames(n, w) == frames
    window = win.skew(w)
    x = clips_of(w + 1, n, dtype=np.float64 if f64 else np.float32)
    refs = list(orc.mdct_batch(x.astype(np.float64), window))
    make = lambda: zafx().mdct_plan(window, row_align=row_align, f64=f64)
    tiles = -(-frames // tile)
    info = dict(tiles=N_CLIPS * tiles, tiles_per_clip=tiles, frames=frames, n=n)
    if carry:
        info["carry"] = [carry * N_CLIPS, tiles]
    return Case(make, forward_bind(x, n, frames), refs, TOL_F64 if f64 else TOL_FFT, kernel, info)


def imdct_case(w, row_align, kernel, tile=32, f64=False):
    frames = 10 * tile + 10
    m = w // 2
    window = win.skew(w)
    dtype = np.float64 if f64 else np.float32
    coefs = orc.mdct_batch(clips_of(w + 2, (frames - 1) * m).astype(np.float64), window).astype(dtype)
    assert coefs.shape[2] == frames
    refs = [orc.imdct(c.astype(np.float64), window) for c in coefs]
    make = lambda: zafx().mdct_plan(window, inverse=True, row_align=row_align, f64=f64)
    tiles = -(-frames // tile)
    info = dict(tiles=N_CLIPS * tiles, tiles_per_clip=tiles, frames=frames, carry=[N_CLIPS, tiles])
    return Case(make, inverse_bind(coefs, frames, dtype), refs, TOL_F64 if f64 else TOL_FFT, kernel, info)


def mel_case(w, hop, fs, n_mel, n_coef, what, kernel, f64=False):
    frames = 170
    n = stft_n(w, hop, frames)
    window = win.skew(w)
    x = clips_of(w + n_mel, n, dtype=np.float64 if f64 else np.float32)
    fb = orc.melfilterbank(fs, w, n_mel)
    x64 = x.astype(np.float64)
    mel = [orc.melspectrogram(c, window, hop, fb) for c in x64] if what != "mfcc" else None
    cep = [orc.mfcc(c, window, hop, fb, n_coef) for c in x64] if what != "mel" else None
    refs = mel if what == "mel" else cep if what == "mfcc" else [np.concatenate([a, b]) for a, b in zip(mel, cep)]

    def make():
        z = zafx()
        return z.mel_plan(window, hop, z.melfilterbank(fs, w, n_mel), None if what == "mel" else n_coef, f64=f64, also_mel=what == "both")
    info = dict(tiles=N_CLIPS * 11, tiles_per_clip=11, frames=frames, n=n)
    return Case(make, forward_bind(x, n, frames), refs, TOL_F64 if f64 else TOL_FB, kernel, info)


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
        if np.asarray(val).shape != r.shape:
            return float("inf")
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
    f = 4 if w >= 2048 else 8   # center_tile_frames (zafx_center.hpp)
    h = w // 2
    n = 10 * f * h + 300        # 41 blocks of one hop: ten tiles of four frames and a partial one
    window = win.skew(w)
    x = np.stack([stereo(w + c, n) for c in range(N_CLIPS)])

    def bind(plan):
        assert zafx().center_tile_frames(w) == f
        return dict(x=x, out_shape=plan.out_shape(N_CLIPS, n), launch=lambda p, d_in, d_out: p.execute(d_in, d_out, N_CLIPS, n),
                    split=lambda out: [out[c] for c in range(N_CLIPS)], keep=None)
    make = lambda: zafx().center_plan(window, sides=sides)
    return Case(make, bind, center_refs(x, window, sides), TOL_FFT, "k_center", dict(tiles=N_CLIPS * 11, tiles_per_clip=11, n=n), err=center_err(sides))


def cqt_kernel(which):
    import scipy.sparse
    if which == "tiny":
        g = np.load(os.path.join(ROOT, "tests", "golden", "tiny.npz"))
        return 4000, 50, 12, scipy.sparse.csr_matrix(g["ck_dense"])
    if which == "8192":
        return 22050, 25, 12, orc.cqtkernel(22050, 12, 55, 7000)
    return 44100, 25, 24, orc.cqtkernel(44100, 24, 55, 3520)   # fft_length 32768: the split transform (cqt_split, zafx_internal.hpp)


def cqt_case(which, chroma, kernel, f64=False):
    fs, tr, res, ck = cqt_kernel(which)
    step = round(fs / tr)
    n = 20 * step + step // 2 + 1
    count = 9   # eight groups: one of two clips, seven of one
    x = clips_of(len(which) + 70, n, count, np.float64 if f64 else np.float32)
    x64 = x.astype(np.float64)
    refs = [orc.cqtchromagram(c, fs, tr, res, ck) if chroma else orc.cqtspectrogram(c, fs, tr, ck) for c in x64]
    frames = refs[0].shape[1]
    make = lambda: zafx().cqt_plan(fs, tr, ck, res if chroma else None, f64=f64)
    info = dict(frames=frames, clips=count, fft_length=int(ck.shape[1]), n=n)
    return Case(make, forward_bind(x, n, frames), refs, TOL_F64 if f64 else TOL_FB, kernel, info)


def dct_case(n, kind, rows_per_tile, kernel):
    rows = 77 * rows_per_tile + 1
    x = np.stack([synth_clip(n + kind, r, n) for r in range(rows)])
    refs = [np.stack([orc.dct(r.astype(np.float64), kind) for r in x])]

    def bind(plan):
        return dict(x=x, out_shape=(rows, n), launch=lambda p, d_in, d_out: p.execute(d_in, d_out, rows, n), split=lambda out: [out], keep=None)
    return Case(lambda: zafx().dct_plan(n, kind, False), bind, refs, TOL_FFT, kernel, dict(tiles=78, rows=rows))


# ------------------------------------------------------------------------------------------------ ragged batches
def with_gaps(parts, dtype, unit=1):
    """The parts back to back with GAPS[i % 3] * unit elements of NaN behind part i: -> (flat, offsets in elements)."""
    offsets, pieces, at = [], [], 0
    for i, a in enumerate(parts):
        offsets.append(at)
        g = np.full(GAPS[i % len(GAPS)] * unit, np.nan, dtype)
        pieces += [np.ascontiguousarray(a, dtype).reshape(-1), g]
        at += a.size + g.size
    return np.concatenate(pieces), np.array(offsets, np.int64)


def ragged_frames(tile, least):
    """Frame counts of RAGGED_TILES tiles each, the last tile partial; `least`: the frames of clip 0."""
    return [least if k == 0 else tile * (k - 1) + tile // 2 + 1 for k in RAGGED_TILES]


def forward_ragged_case(kind, kernel, f64=False):
    """zafx_execute_ragged: STFT, mel and MDCT plans at W = 2048 whose rows are whole lines."""
    w, hop = 2048, 1024
    window = win.skew(w)
    dtype = np.float64 if f64 else np.float32
    tile = {"stft": 8 if f64 else 16, "mel": 16, "mdct": 16 if f64 else 32}[kind]
    if kind == "mdct":
        lengths = [0] + [(t - 2) * hop + 5 for t in ragged_frames(tile, 0)[1:]]
        assert [orc.mdct_num_frames(n, w) for n in lengths[1:]] == ragged_frames(tile, 0)[1:]
        tiles = [-(-orc.mdct_num_frames(n, w) // tile) for n in lengths]
    else:
        lengths = [0] + [stft_n(w, hop, t) for t in ragged_frames(tile, 0)[1:]]
        tiles = [-(-orc.stft_num_frames(n, w, hop) // tile) for n in lengths]
    assert tiles[1:] == list(RAGGED_TILES[1:]) and tiles[0] <= 1, tiles
    xs = [synth_clip(70 + len(kind), i, n).astype(dtype) for i, n in enumerate(lengths)]
    flat, in_offsets = with_gaps(xs, dtype)
    if f64:   # (the float64 forms read 16-byte pieces of a clip from its own base: any offset)
        assert (in_offsets % 2).any()
    lens = np.array(lengths, np.int64)
    fb = orc.melfilterbank(FS, w, 128)
    if kind == "stft":
        refs = [orc.stft(x.astype(np.float64), window, hop) for x in xs]
        make = lambda: zafx().stft_plan(window, hop, row_align=8 if f64 else 16, f64=f64)
    elif kind == "mel":
        refs = [orc.melspectrogram(x.astype(np.float64), window, hop, fb) for x in xs]
        make = lambda: zafx().mel_plan(window, hop, zafx().melfilterbank(FS, w, 128), row_align=16 if f64 else 32, f64=f64)
    else:
        refs = [orc.mdct(x.astype(np.float64), window) for x in xs]
        make = lambda: zafx().mdct_plan(window, row_align=16 if f64 else 32, f64=f64)

    def bind(plan):
        offs, frames, pitch = plan.ragged_layout(lens)
        rows = refs[1].shape[0]
        keep = np.zeros(int(offs[-1]), bool)
        for i in range(len(lens)):
            keep[int(offs[i]):int(offs[i]) + rows * int(pitch[i])].reshape(rows, int(pitch[i]))[:, :int(frames[i])] = True
        split = lambda out: [out[int(offs[i]):int(offs[i]) + rows * int(pitch[i])].reshape(rows, int(pitch[i]))[:, :int(frames[i])] for i in range(len(lens))]
        return dict(x=flat, out_shape=(int(offs[-1]),), launch=lambda p, d_in, d_out: p.execute_ragged(d_in, in_offsets, lens, d_out), split=split, keep=keep)
    tol = TOL_F64 if f64 else TOL_FB if kind == "mel" else TOL_FFT
    return Case(make, bind, refs, tol, kernel, dict(tiles=int(sum(tiles)), clip_tiles=tiles, lengths=lengths))


def out_places(sizes, unit=1):
    """Output offsets (in units) with GAPS between the clips and 5 units in front: -> (offsets, total)."""
    offs, at = [], 5
    for i, n in enumerate(sizes):
        offs.append(at)
        at += n + GAPS[i % len(GAPS)]
    return np.array(offs, np.int64), at


def inverse_ragged_case(kind, kernel):
    """zafx_execute_imdct_ragged / zafx_execute_istft_ragged at W = 2048: blocks at the plan's pitch with NaN pad columns and gaps of 1, 3 and 5
    elements behind them; the clips' samples at places with gaps between them."""
    w, hop = 2048, 1024
    window = win.skew(w)
    tile = 32 if kind == "imdct" else 16
    frames = ragged_frames(tile, 1)   # (one frame: no output, no tile, for either transform at hop W / 2)
    if kind == "imdct":
        blocks = [orc.mdct(synth_clip(79, i, (t - 1) * hop).astype(np.float64), window).astype(np.float32) for i, t in enumerate(frames)]
        refs = [orc.imdct(b.astype(np.float64), window) if t > 1 else np.zeros(0) for b, t in zip(blocks, frames)]
        make = lambda: zafx().mdct_plan(window, inverse=True, row_align=32)
        dtype = np.float32
    else:
        blocks = [orc.stft(synth_clip(80, i, stft_n(w, hop, t) if t > 1 else 0).astype(np.float64), window, hop).astype(np.complex64) for i, t in enumerate(frames)]
        refs = [orc.istft(b.astype(np.complex128), window, hop) for b in blocks]
        make = lambda: zafx().istft_plan(window, hop, row_align=16)
        dtype = np.complex64
    assert [b.shape[1] for b in blocks] == frames, [b.shape for b in blocks]
    sizes = [len(r) for r in refs]
    assert sizes[0] == 0
    out_off, total = out_places(sizes)
    frames_a = np.array(frames, np.int64)

    def bind(plan):
        packed = [rows_with_nan_pads(b[None], plan.row_pitch(t), dtype)[0] for b, t in zip(blocks, frames)]
        flat, in_off = with_gaps(packed, dtype)
        keep = np.zeros(total, bool)
        for o, n in zip(out_off.tolist(), sizes):
            keep[o:o + n] = True
        name = "execute_imdct_ragged" if kind == "imdct" else "execute_istft_ragged"
        return dict(x=flat, out_shape=(total,), launch=lambda p, d_in, d_out: getattr(p, name)(d_in, in_off, frames_a, d_out, out_off),
                    split=lambda out: [out[o:o + n] for o, n in zip(out_off.tolist(), sizes)], keep=keep)
    tiles = [0 if n == 0 else -(-t // tile) for t, n in zip(frames, sizes)]
    assert tiles == list(RAGGED_TILES)
    return Case(make, bind, refs, TOL_FFT, kernel, dict(tiles=int(sum(tiles)), clip_tiles=tiles, frames=frames))


def center_ragged_case():
    """zafx_execute_center_ragged at W = 256 (tiles of 8 frames).  Three times RAGGED_TILES: k_center's units aim at 12 per slot and have a floor
    of 29 blocks, so a cap of 1 lifts the segment length above the floor only from 29 x 12 x 4 blocks on."""
    w, f = 256, 8
    h = w // 2
    window = win.skew(w)
    lengths = [0 if k == 0 else (3 * k * f - f // 2) * h - 37 for k in RAGGED_TILES]
    xs = [stereo(3 * w + c, n) for c, n in enumerate(lengths)]
    flat, in_floats = with_gaps(xs, np.float32, unit=2)
    refs = center_refs(xs, window, True)
    out_off, total = out_places([2 * n for n in lengths])   # (sample frames; center and sides: 2 n)
    lens = np.array(lengths, np.int64)

    def bind(plan):
        assert zafx().center_tile_frames(w) == f
        keep = np.zeros((total, 2), bool)
        for o, n in zip(out_off.tolist(), lengths):
            keep[o:o + 2 * n] = True
        return dict(x=flat, out_shape=(total, 2), launch=lambda p, d_in, d_out: p.execute_center_ragged(d_in, in_floats // 2, lens, d_out, out_off),
                    split=lambda out: [out[o:o + 2 * n].reshape(2, n, 2) for o, n in zip(out_off.tolist(), lengths)], keep=keep)
    blocks = [-(-n // h) for n in lengths]
    return Case(lambda: zafx().center_plan(window, sides=True), bind, refs, TOL_FFT, "k_center_ragged",
                dict(blocks=int(sum(blocks)), lengths=lengths, window=w, tile_frames=f), err=center_err(True))


# ------------------------------------------------------------------------------------------------ the routes
# name -> the case.  Geometry -> kernel as tests/test_gpu_windows.py and the docstring of tests/test_gpu_arena.py give it: rows padded to whole
# lines (row_align) select the plain forms, compact rows of T = 170 / 322 frames (no multiple of 16) the carry forms.
ROUTES = {
    "stft_ft16_claimed": lambda: stft_case(2048, 1024, 16, "k_stft_ft16"),
    "stft_ft16_static": lambda: stft_case(2048, 1024, 16, "k_stft_ft16", env={"ZAFX_STFT_DYNAMIC": "0"}),
    "stft_ft16c": lambda: stft_case(2048, 1024, 0, "k_stft_ft16c", carry=1),
    "stft_ft16b": lambda: stft_case(4096, 2048, 16, "k_stft_ft16b"),
    "stft_ft16bc": lambda: stft_case(4096, 2048, 0, "k_stft_ft16bc", carry=2),
    "stft_ft16q": lambda: stft_case(8192, 4096, 16, "k_stft_ft16q"),
    "stft_tf": lambda: stft_case(2048, 1024, 0, "k_stft_tf", layout="TF"),
    "mel_ft16b": lambda: mel_case(4096, 2048, FS, 128, 20, "mfcc", "k_mel_ft16b"),
    "mel2_mel": lambda: mel_case(2048, 1024, FS, 128, 20, "mel", "k_mel2"),
    "mel2_mfcc": lambda: mel_case(2048, 1024, FS, 128, 20, "mfcc", "k_mel2"),
    "mel2_both": lambda: mel_case(2048, 1024, FS, 128, 20, "both", "k_mel2"),
    "mel": lambda: mel_case(1024, 256, 22050, 64, 13, "mfcc", "k_mel"),
    "melfb": lambda: mel_case(2048, 1024, FS, 300, 20, "mel", "k_melfb"),
    "istft_ft16": lambda: istft_case(2048, 1024, 0, "k_istft_ft16"),
    "istft_ft16b": lambda: istft_case(4096, 1024, 0, "k_istft_ft16b", units_per_clip=2),
    "istft_ft16d": lambda: istft_case(4096, 2048, 0, "k_istft_ft16d"),
    "istft_ft8q": lambda: istft_case(8192, 4096, 0, "k_istft_ft8q", tile=8),
    "mdct_ft32_plain": lambda: mdct_case(2048, 32, "k_mdct_ft32"),
    "mdct_ft32_carry": lambda: mdct_case(2048, 0, "k_mdct_ft32", carry=1),
    "mdct_ft32b": lambda: mdct_case(4096, 32, "k_mdct_ft32b"),
    "mdct_ft32bc": lambda: mdct_case(4096, 0, "k_mdct_ft32bc", carry=2),
    "mdct_ft32q": lambda: mdct_case(8192, 32, "k_mdct_ft32q"),
    "imdct": lambda: imdct_case(2048, 0, "k_imdct"),
    "imdct_q": lambda: imdct_case(8192, 32, "k_imdct_q", tile=16),
    "center": lambda: center_case(2048, False),
    "center_sides": lambda: center_case(2048, True),
    "cqt_tiny": lambda: cqt_case("tiny", False, "k_cqt"),
    "cqt_8192": lambda: cqt_case("8192", False, "k_cqt"),
    "chroma_8192": lambda: cqt_case("8192", True, "k_cqt"),
    "cqt_split": lambda: cqt_case("full", False, "k_cqt"),
    "dct": lambda: dct_case(64, 2, 16, "k_dct"),
    "dct_bsh": lambda: dct_case(100, 2, 4, "k_dct_bsh"),
    "dct_bs32": lambda: dct_case(441, 2, 1, "k_dct_bs32"),
    "stft_ragged": lambda: forward_ragged_case("stft", "k_stft_ft16_ragged"),
    "mel2_ragged": lambda: forward_ragged_case("mel", "k_mel2_ragged"),
    "mdct_ragged": lambda: forward_ragged_case("mdct", "k_mdct_ft32_ragged"),
    "imdct_ragged": lambda: inverse_ragged_case("imdct", "k_imdct_ragged"),
    "istft_ragged": lambda: inverse_ragged_case("istft", "k_istft_ragged"),
    "center_ragged": center_ragged_case,
    "stft_f64": lambda: stft_case(2048, 1024, 8, "k_stft_ft8_f64", tile=8, f64=True),
    "mdct_f64": lambda: mdct_case(2048, 16, "k_mdct_ft16_f64", tile=16, f64=True),
    "mel_f64": lambda: mel_case(2048, 1024, FS, 128, 20, "mel", "k_mel_ft8_f64", f64=True),
    "istft_f64": lambda: istft_case(2048, 1024, 8, "k_istft_ft8_f64", tile=8, f64=True),
    "imdct_f64": lambda: imdct_case(2048, 16, "k_imdct_ft16_f64", tile=16, f64=True),
    "cqt_f64": lambda: cqt_case("full", False, "k_cqt_ft_f64", f64=True),
    "stft_f64_ragged": lambda: forward_ragged_case("stft", "k_stft_ft8_f64_ragged", f64=True),
    "mdct_f64_ragged": lambda: forward_ragged_case("mdct", "k_mdct_ft16_f64_ragged", f64=True),
    "mel_f64_ragged": lambda: forward_ragged_case("mel", "k_mel_ft8_f64_ragged", f64=True),
}


# ------------------------------------------------------------------------------------------------ the run
class capped:
    """ZAFX_COMPUTE_UNITS (and the route's own switches) in the environment while a plan is made."""

    def __init__(self, cap, extra):
        self.env = dict(extra, ZAFX_COMPUTE_UNITS=None if cap is None else str(cap))

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def say(**fields):
    print(json.dumps(fields), flush=True)


def nan_filled(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.float64 if np.dtype(dtype).itemsize % 8 == 0 and np.dtype(dtype) != np.complex64 else np.float32).fill(np.nan)
    return a


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def main(route, dry):
    t0 = time.time()
    case = ROUTES[route]()
    say(route=route, stage="ready", info=case.info, kernel_expected=case.kernel, secs=round(time.time() - t0, 2))
    if dry:
        return
    z = zafx()
    first, bound, d_in = None, None, None
    for cap in CAPS:
        with capped(cap, case.env):
            z.clear_plan_cache()
            plan = case.make()
        if bound is None:
            bound = case.bind(plan)
            d_in = z.DeviceBuffer.from_host(bound["x"])
        dtype = plan.out_dtype
        runs = []
        for launch in range(2):   # two launches in a row of one plan: whatever a launch leaves behind in the plan is what the next one finds
            d_out = z.DeviceBuffer(bound["out_shape"], dtype)
            d_out.upload(nan_filled(bound["out_shape"], dtype))
            say(route=route, stage="launch", cap=cap, launch=launch)
            bound["launch"](plan, d_in, d_out)
            plan.sync()
            runs.append(d_out.download())
            d_out.free()
        out = runs[0]
        if first is None:
            first = out
        got = bound["split"](out)
        errs = [case.err(np.asarray(g, np.complex128 if np.iscomplexobj(g) else np.float64), r) for g, r in zip(got, case.refs)]
        scalars = out.view(np.float64 if out.dtype.itemsize % 8 == 0 and out.dtype != np.complex64 else np.float32).reshape(-1)
        keep = bound["keep"]
        outside_untouched = True
        if keep is not None:
            per = scalars.size // keep.size
            outside_untouched = bool(np.isnan(scalars.reshape(-1, per)[~keep.reshape(-1)]).all())
            written = bool(np.isfinite(scalars.reshape(-1, per)[keep.reshape(-1)]).all())
        else:
            written = bool(np.isfinite(scalars).all())
        same = bool(np.array_equal(as_bytes(out), as_bytes(first)))
        line = dict(route=route, stage="done", cap=cap, compute_units=plan.compute_units, device_compute_units=plan.device_compute_units,
                    kernel=plan.last_kernel, worst=max(errs) if errs else 0.0, tol=case.tol, clips=len(got), refs=len(case.refs),
                    shapes_ok=all(np.asarray(g).shape == r.shape for g, r in zip(got, case.refs)), written=written, outside_untouched=outside_untouched,
                    repeat_same=bool(np.array_equal(as_bytes(runs[1]), as_bytes(out))), same_as_uncapped=same, secs=round(time.time() - t0, 2))
        if not same:   # what differs, for the record
            a, b = scalars, first.view(scalars.dtype).reshape(-1)
            both = np.isfinite(a) & np.isfinite(b)
            line.update(words_differing=int((as_bytes(out) != as_bytes(first)).reshape(-1, scalars.dtype.itemsize).any(axis=1).sum()), words=int(a.size),
                        nan_mismatch=int((np.isfinite(a) != np.isfinite(b)).sum()),
                        normwise_to_uncapped=float(np.max(np.abs(a[both] - b[both])) / (np.max(np.abs(b[both])) or 1.0)) if both.any() else None)
        say(**line)
    say(route=route, stage="end", secs=round(time.time() - t0, 2))


if __name__ == "__main__":
    if sys.argv[1] == "--list":
        print("\n".join(ROUTES))
    else:
        main(sys.argv[1], "--dry" in sys.argv[2:])
