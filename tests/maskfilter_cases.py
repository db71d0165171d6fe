"""The mask-filter cases of the cross-route contracts (tests/test_gpu_accuracy.py, tests/test_gpu_windows.py, tests/test_gpu_signals.py and
their host twins): per case the clips, the masks, the window, the float64 reference (tests/maskfilter_oracle.py,
tests/maskfilter_complex_oracle.py; the rest is x minus the sum of the stems) and the float32 yardstick (tests/plain.py's maskfilter*: unpacked,
one frame per transform).  Host arithmetic only: the launches are in tests/maskfilter_run.py.

Forms -- the eight fused float32 kernels through every mask layout they read:

    ft, ft32, tf   a real mask in "FT" compact, "FT" with row_align 32, "TF"      k_maskfilter / k_maskfilter_ragged
    stems          S = 3 real masks, "TF"                                        k_maskfilter_stems / k_maskfilter_stems_ragged
    complex        a complex mask, "TF"                                          k_maskfilter_complex / k_maskfilter_complex_ragged
    stereo1        interleaved stereo clips, one real mask for both channels     k_maskfilter_stereo / k_maskfilter_stereo_ragged
    stereo2        ... a real mask per channel, (T, 2, W/2 + 1)                  the same two

A stereo clip is (N, 2) float32; its results, references and yardsticks are (rows, N) like everyone's, the channels de-interleaved: y_L, y_R
and behind them rest_L, rest_R -- two rows of rest (rest_rows) where the mono forms have one.  The stereo kernels pack the two CHANNELS of one
frame into one transform where the mono kernels pack two frames; the yardstick (plain.maskfilter_stereo) packs nothing.

A batch is 3 clips of unit noise of `blocks` H + 5 samples; its ragged twin holds the same clips with clips of 1, H, 3 H + 7 and 0 samples
between them.  blocks = 60 gives T = 62 frames, 61 gives T = 63: the last frame pairs with zeros.  Either runs several tiles, so the carry is
handed on, and a batch this small is cut into segments, whose edges fall inside a hop-long block of tests/accuracy.py's e_col.

Also here: a NumPy float32 model of the kernels' PACKED arithmetic (two frames in one W-point transform, the split, the re-pack, one inverse),
with one defect at a time for tests/test_accuracy_host.py, its sibling for the stereo packing (stereo_model), the per-hop bound of the signal
contract (hop_share; hop_share_stereo with the floor's level over both channels) and the PCM kernels' int16 bound made per hop."""
import functools

import numpy as np

import const_probe as cp
import plain
import signals as sig
import windows as win
from conftest import excess, row_bound
from maskfilter_complex_oracle import make_complex_mask, oracle_maskfilter_complex
from maskfilter_oracle import TOL_FFT, make_mask, mask_error, mask_frames, oracle_maskfilter   # noqa: F401
from maskfilter_stereo_oracle import make_stereo_masks, oracle_maskfilter_stereo

WINDOWS = (256, 512, 1024, 2048)
BLOCKS = (60, 61)   # clips of 60 H + 5 (T = 62) and of 61 H + 5 (T = 63)
N_STEMS = 3
REAL_MASKS = ("uniform", "sparse", "unit", "signed_wide")
EPS32 = float(np.finfo(np.float32).eps)
C_FLOOR = 2.0   # tests/test_gpu_signals.py's constant for frames of up to 2048 points

# form -> (family, mask layout, row_align)
FORMS = {"ft": ("real", "FT", 0), "ft32": ("real", "FT", 32), "tf": ("real", "TF", 0), "stems": ("stems", "TF", 0), "complex": ("complex", "TF", 0),
         "stereo1": ("stereo", "TF", 0), "stereo2": ("stereo", "TF", 0)}
# family -> (the equal-length launch's last_kernel, the ragged launch's)
KERNELS = {"real": ("k_maskfilter", "k_maskfilter_ragged"), "stems": ("k_maskfilter_stems", "k_maskfilter_stems_ragged"),
           "complex": ("k_maskfilter_complex", "k_maskfilter_complex_ragged"), "stereo": ("k_maskfilter_stereo", "k_maskfilter_stereo_ragged")}
# the PCM entry points' kernels, by n_channels: (equal-length, ragged)
PCM_KERNELS = {1: ("k_maskfilter_pcm", "k_maskfilter_pcm_ragged"), 2: ("k_maskfilter_stereo_pcm", "k_maskfilter_stereo_pcm_ragged")}
PCM_FORMS = ("tf", "stereo1", "stereo2")   # what zafx_execute_masked_pcm takes: mono "TF", and the two stereo forms
STEREO_DATA = {"stereo1": 1, "stereo2": 2}   # the data of a stereo form -> its mask_channels


def family_of(form):
    return FORMS[form][0]


def data_of(form):
    """What batch(), extras(), masks_for(), reference() and yardstick() are keyed by: the family -- the forms of the real kind share their
    clips and masks --, and for the stereo family the form, whose masks differ in shape."""
    return form if family_of(form) == "stereo" else family_of(form)


def rest_rows(form_or_data):
    """The rows the rest takes at the end of a clip's (rows, N): 2 for a stereo form (rest_L, rest_R), else 1."""
    return 2 if form_or_data in STEREO_DATA else 1


def window_of(name, wl):
    """"hamming": periodic Hamming; else a recipe of tests/windows.py.  Rounded through float32: what the plan is handed."""
    return cp.window_a(wl) if name == "hamming" else win.window(name, wl)


def clip(seed, n):
    return np.random.default_rng([303, seed, n]).standard_normal(n).astype(np.float32)


def stereo_clip(seed, n):
    """(N, 2) unit noise, a seed stream of the stereo forms' own."""
    return np.random.default_rng([404, seed, n]).standard_normal((n, 2)).astype(np.float32)


def clip_of(data, seed, n):
    return stereo_clip(seed, n) if data in STEREO_DATA else clip(seed, n)


def _covers(m):
    """Every two neighbouring frames of the mask (W/2 + 1, T) hold a non-zero between them."""
    live = m.any(axis=0)
    return bool((live[:-1] | live[1:]).all())


def covering_sparse_stereo(wl, n, channels, seed):
    """covering_sparse's rule per channel: make_stereo_masks("sparse") of the first seed in seed, seed + 100, ... for which EACH channel's
    mask leaves no hop-long block without a reference."""
    while True:
        m = make_stereo_masks("sparse", wl, n, channels, seed=seed)
        if all(_covers(v) for v in (m[None] if channels == 1 else m)):
            return m
        seed += 100


def covering_sparse(wl, n, seed):
    """The "sparse" mask of the first seed in seed, seed + 100, ... that leaves no hop-long block without a reference: every two neighbouring
    frames hold a one between them.  At W = 256 a frame's 129 values are all zero once in 14 frames, and where two such frames meet the
    reference -- and the unpacked yardstick -- is exactly 0 while a packed frame carries its partner's rounding (zafx_maskfilter.hpp): e_col
    of tests/accuracy.py would divide by zero there.  What a kernel may leave in such a block is the floor term of hop_share below, which
    tests/test_gpu_signals.py holds under the plain "sparse" mask."""
    while True:
        m = make_mask("sparse", wl, n, seed=seed)
        if _covers(m):
            return m
        seed += 100


def masks_for(family, wl, n, seed, kind):
    """One clip's masks: (W/2 + 1, T) float32, (N_STEMS, W/2 + 1, T) float32 "unit" per stem -- they do not sum to one, so the rest is no near
    cancellation -- or (W/2 + 1, T) complex64 "disc"."""
    if family in STEREO_DATA:   # (W/2 + 1, T) for both channels or (2, W/2 + 1, T): two different masks of the kind
        ch = STEREO_DATA[family]
        return covering_sparse_stereo(wl, n, ch, seed) if kind == "sparse" else make_stereo_masks(kind, wl, n, ch, seed=seed)
    if family == "real":
        return covering_sparse(wl, n, seed) if kind == "sparse" else make_mask(kind, wl, n, seed=seed)
    if family == "stems":
        return np.stack([make_mask("unit", wl, n, seed=10 * seed + s) for s in range(N_STEMS)])
    return make_complex_mask("disc", wl, n, seed=seed)


def reference(family, x, w, m):
    """(rows, N) float64: the stems (one for the one-mask families), then the rest x - sum of them; stereo: y_L, y_R, rest_L, rest_R."""
    if family in STEREO_DATA:
        y = oracle_maskfilter_stereo(x, w, m)
        return np.ascontiguousarray(np.concatenate((y.T, (np.asarray(x, np.float64) - y).T)))
    if family == "real":
        ys = [oracle_maskfilter(x, w, m)]
    elif family == "stems":
        ys = [oracle_maskfilter(x, w, ms) for ms in m]
    else:
        ys = [oracle_maskfilter_complex(x, w, m)]
    return np.stack(ys + [np.asarray(x, np.float64) - sum(ys)])


def yardstick(family, x, w, m):
    """(rows, N) float32 by tests/plain.py: the stems, then the float32 subtraction chain ((x - y_0) - y_1) - ...; stereo: each channel
    alone through the unpacked chain."""
    if family in STEREO_DATA:
        return plain.maskfilter_stereo(x, w, m, np.float32, rest=True)
    if family == "real":
        return plain.maskfilter_stems(x, w, m[None], np.float32, rest=True)
    if family == "stems":
        return plain.maskfilter_stems(x, w, m, np.float32, rest=True)
    y = plain.maskfilter_complex(x, w, m, np.float32)
    return np.stack([y, np.asarray(x, np.float32) - y])


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def batch(family, wl, n, window="hamming", masks="catalogue", rotate=0, count=3):
    """-> dict: w, clips, masks, refs, yard (tuples, one entry per clip; refs / yard: (rows, N) with the rest last).  masks "catalogue": clip k of a
    real-kind batch takes REAL_MASKS[(k + rotate) % 4]; "unit": every real mask is "unit".  Computed once and left unchanged."""
    w = window_of(window, wl)
    clips = [clip_of(family, k, n) for k in range(count)]
    kinds = [REAL_MASKS[(k + rotate) % len(REAL_MASKS)] if masks == "catalogue" else "unit" for k in range(count)]
    ms = [masks_for(family, wl, n, k, kinds[k]) for k in range(count)]
    return {"w": w, "clips": _frozen(clips), "masks": _frozen(ms), "kinds": tuple(kinds),
            "refs": _frozen([reference(family, x, w, m) for x, m in zip(clips, ms)]),
            "yard": _frozen([yardstick(family, x, w, m) for x, m in zip(clips, ms)])}


def extra_lengths(wl):
    h = wl // 2
    return (1, h, 3 * h + 7, 0)


@functools.lru_cache(maxsize=None)
def extras(family, wl, window="hamming"):
    """The clips a ragged twin adds, lengths 1, H, 3 H + 7 and 0, with "unit" / "disc" masks and their references and yardsticks."""
    w = window_of(window, wl)
    clips = [clip_of(family, 10 + i, n) for i, n in enumerate(extra_lengths(wl))]
    ms = [masks_for(family, wl, len(x), 10 + i, "unit") for i, x in enumerate(clips)]
    return {"clips": _frozen(clips), "masks": _frozen(ms),
            "refs": _frozen([reference(family, x, w, m) for x, m in zip(clips, ms)]),
            "yard": _frozen([yardstick(family, x, w, m) for x, m in zip(clips, ms)])}


TWIN_ORDER = (("batch", 0), ("extra", 0), ("extra", 1), ("batch", 1), ("extra", 2), ("extra", 3), ("batch", 2))


def ragged_twin(b, e):
    """The batch's clips with the extra ones between them -> (dict like batch()'s, the twin's index of each clip of the batch)."""
    pick = lambda key: tuple((b if src == "batch" else e)[key][i] for src, i in TWIN_ORDER)   # noqa: E731
    twin = {"w": b["w"], "clips": pick("clips"), "masks": pick("masks"), "refs": pick("refs"), "yard": pick("yard")}
    return twin, [i for i, (src, _) in enumerate(TWIN_ORDER) if src == "batch"]


# ------------------------------------------------------------------------------------------------ the accuracy catalogue
def accuracy_cases():
    """name -> (form, W, blocks, rest): 7 forms x 4 windows x 2 clip lengths x with and without the rest."""
    return {f"{form}_{wl}_{blocks}{'_rest' if rest else ''}": (form, wl, blocks, rest)
            for form in FORMS for wl in WINDOWS for blocks in BLOCKS for rest in (False, True)}


ACCURACY_CASES = accuracy_cases()


def accuracy_batch(name):
    """-> (batch, extras) of a catalogue case.  The real and the stereo kinds' four masks rotate with the window and the clip length, so that
    every form meets every mask."""
    form, wl, blocks, rest = ACCURACY_CASES[name]
    data = data_of(form)
    rotate = WINDOWS.index(wl) + BLOCKS.index(blocks) if family_of(form) in ("real", "stereo") else 0
    return batch(data, wl, blocks * (wl // 2) + 5, rotate=rotate), extras(data, wl)


def all_rows(results):
    """Per-clip (rows, N) arrays -> the list of 1-D results tests/accuracy.measure takes.  Clips of length 0 have nothing to measure."""
    return [v for r in results if np.asarray(r).shape[1] for v in np.asarray(r)]


def rows_of(refs, rest, tail=1):
    """The same of references or yardsticks, whose last `tail` rows are the rest (rest_rows): every stem of every clip, and with `rest` its
    rest."""
    return all_rows([r if rest else r[:-tail] for r in refs])


def row_level(ref, x, j, tail=1):
    """The level mask_error holds row j of a clip's (rows, N) result to, as a stand-in for its `x`: the clip itself for a mono form; for a
    stereo form (tail = 2) the rows come in channel pairs and the level is taken over BOTH channels, of the clip and of the pair's
    reference -- the bound of tests/test_gpu_maskfilter_stereo.py (stereo_error)."""
    if tail == 1:
        return x
    pair = np.asarray(ref)[j - j % 2:j - j % 2 + 2]
    return np.array([np.abs(pair).max() if pair.size else 0.0, np.abs(np.asarray(x)).max() if np.size(x) else 0.0])


# ------------------------------------------------------------------------------------------------ signals that are not white noise
SIGNAL_NAMES = sig.NAMES + ("loud_quiet",)   # the mono recipes and channel 0 of the stereo "loud_quiet": unit noise, then noise at -90 dB
SIGNAL_WINDOWS = (2048, 256)
SIGNAL_MASKS = ("uniform", "sparse")
SIGNAL_FORMS = ("tf", "ft", "stems", "complex")


def signal_clip(name, n):
    return np.ascontiguousarray(sig.stereo_signal(name, n)[:, 0]) if name == "loud_quiet" else sig.signal(name, n)


@functools.lru_cache(maxsize=None)
def signal_case(name, wl):
    """family -> {"clips", "masks", "refs", "yard", "equal"}: the ragged batch of the signal at 20 H + 9 samples and its first 7 H + 3, and the
    indices of the clips of full length, which are the equal-length batch.  Real kind: the clip under "uniform", its head under "uniform", the
    clip under "sparse"; stems: S = 2, "uniform" and "sparse"; complex: "disc"."""
    h = wl // 2
    w = window_of("hamming", wl)
    x = signal_clip(name, 20 * h + 9)
    head = np.ascontiguousarray(x[:7 * h + 3])
    real = lambda v, kind: make_mask(kind, wl, len(v), seed=0)   # noqa: E731
    both = lambda v: np.stack([real(v, kind) for kind in SIGNAL_MASKS])   # noqa: E731
    disc = lambda v: make_complex_mask("disc", wl, len(v), seed=0)   # noqa: E731
    plans = {"real": ([x, head, x], [real(x, "uniform"), real(head, "uniform"), real(x, "sparse")], [0, 2]),
             "stems": ([x, head], [both(x), both(head)], [0]),
             "complex": ([x, head], [disc(x), disc(head)], [0])}
    out = {"w": w}
    for family, (clips, masks, equal) in plans.items():
        out[family] = {"clips": _frozen(clips), "masks": _frozen(masks), "equal": tuple(equal),
                       "refs": _frozen([reference(family, c, w, m) for c, m in zip(clips, masks)]),
                       "yard": _frozen([yardstick(family, c, w, m) for c, m in zip(clips, masks)])}
    return out


# ------------------------------------------------------------------------------------------------ the per-hop bound
def hops(y, h):
    """A 1-D result as rows of one hop each (zero-filled at the end)."""
    n = -(-len(y) // h) * h
    return np.pad(np.asarray(y, np.float64), (0, n - len(y))).reshape(-1, h)


def hop_share(y, ref, x, h, level=None):
    """max over samples of |y - ref| / (10 TOL_FFT max_hop|ref| + C_FLOOR eps32 max(max|ref|, max|x|)): at most 1 where the per-hop bound
    holds; 0 for an exact result (silence).  level: the floor's level where it is not this row's own (hop_share_stereo)."""
    if level is None:
        level = max(float(np.abs(ref).max()), float(np.abs(x).max())) if len(ref) else 0.0
    return excess(hops(y, h), hops(ref, h), row_bound(hops(ref, h), TOL_FFT, C_FLOOR * EPS32 * level))


def hop_share_stereo(y, ref, x, h):
    """hop_share of a channel pair, y and ref (2, N), of the stereo clip x (N, 2) -> (the share of L, of R).  max_hop|ref| is each channel's
    own; the floor's level is max(max|ref|, max|x|) over BOTH channels: the two channels of a frame share a transform, and "rounding error of
    the louder channel ... reaches the other channel of the same frame" (zafx_maskfilter_stereo.hpp) -- never the next frame's, so a quiet HOP
    beside a loud one is still held to its own level."""
    y, ref, x = np.asarray(y), np.asarray(ref), np.asarray(x)
    assert y.shape == ref.shape and len(ref) == 2 and x.shape == (ref.shape[1], 2), (y.shape, ref.shape, x.shape)
    level = max(float(np.abs(ref).max()), float(np.abs(x).max())) if ref.size else 0.0
    return tuple(hop_share(y[c], ref[c], None, h, level=level) for c in (0, 1))


def int16_bound(ref, xn, h):
    """What an int16 output of the PCM kernels may differ by from 32768 ref, in LSB, per sample: 0.5 + 32768 (the per-hop bound) -- half an LSB
    of the quantiser on top of hop_share's bound (mono: ref (1, N)) or hop_share_stereo's (ref (2, N): y_L, y_R), whose level is taken over
    the rows of `ref` and the normalised clip xn = x / 32768.  tests/test_gpu_maskfilter_pcm.py::test_int16_out_against_the_float64_oracle's
    bound made per hop."""
    ref, xn = np.asarray(ref, np.float64), np.asarray(xn)
    assert ref.ndim == 2 and ref.shape[1] == len(xn), (ref.shape, xn.shape)
    if not ref.size:
        return np.full(ref.shape, 0.5)
    level = max(float(np.abs(ref).max()), float(np.abs(xn).max()))
    per_hop = [row_bound(hops(r, h), TOL_FFT, C_FLOOR * EPS32 * level).repeat(h, axis=1).reshape(-1)[:len(r)] for r in ref]
    return 0.5 + 32768.0 * np.stack(per_hop)


def to_int16(x, scale):
    """rint(scale x) clipped to int16: the PCM twin of a float clip."""
    return np.clip(np.rint(float(scale) * np.asarray(x, np.float64)), -32768, 32767).astype(np.int16)


def normalised(q):
    """The float32 clip the PCM kernels see: s / 32768, exact."""
    return np.asarray(q).astype(np.float32) / np.float32(32768)


# ------------------------------------------------------------------------------------------------ stereo signals that are not white noise
STEREO_SIGNAL_FORMS = {"stereo1": ("uniform",), "stereo2": ("uniform", "sparse")}   # form -> the mask kind(s): one for both channels; L's, R's


@functools.lru_cache(maxsize=None)
def stereo_signal_case(name, wl):
    """form -> {"clips", "masks", "refs", "yard", "equal"}: the ragged batch of the stereo signal at 20 H + 9 sample frames and its first
    7 H + 3, and the index of the clip of full length, which is the equal-length batch.  stereo1: "uniform" for both channels; stereo2:
    "uniform" on L, "sparse" on R (plain make_mask: a hop without a reference is the floor term's business)."""
    h = wl // 2
    w = window_of("hamming", wl)
    x = sig.stereo_signal(name, 20 * h + 9)
    clips = [x, np.ascontiguousarray(x[:7 * h + 3])]
    out = {"w": w}
    for form, kinds in STEREO_SIGNAL_FORMS.items():
        one = lambda v: [make_mask(kind, wl, len(v), seed=s) for s, kind in enumerate(kinds)]   # noqa: E731
        masks = [one(v)[0] if len(kinds) == 1 else np.stack(one(v)) for v in clips]
        out[form] = {"clips": _frozen(clips), "masks": _frozen(masks), "equal": (0,),
                     "refs": _frozen([reference(form, c, w, m) for c, m in zip(clips, masks)]),
                     "yard": _frozen([yardstick(form, c, w, m) for c, m in zip(clips, masks)])}
    return out


# ------------------------------------------------------------------------------------------------ the packed arithmetic, as a model
DEFECTS = ("window_mirror", "bin_h", "round16")


def round_mantissa(a, keep):
    """complex64 / float32 values rounded to `keep` mantissa bits (to nearest, ties up)."""
    drop = 23 - keep
    u = np.ascontiguousarray(a).view(np.uint32)
    return ((u + np.uint32(1 << (drop - 1))) & np.uint32(~((1 << drop) - 1) & 0xFFFFFFFF)).view(a.dtype)


def packed_model(x, w, m, defect=None):
    """y (N,) float32 by the kernels' arithmetic in NumPy float32: frames 2j and 2j + 1 as Z = FFT(a + i b), A = (Z[k] + conj Z[W-k]) / 2,
    B = (Z[k] - conj Z[W-k]) / 2i, C = m_a A + i m_b B, one inverse transform whose real and imaginary parts are the two masked frames,
    overlap-add, the division by the COLA gain (zafx_maskfilter.hpp).  Not the kernels' bits: their rounding, order by order.

    defect, one at a time: "window_mirror" the window read at (W - n) % W; "bin_h" bin H's mask taken from bin H - 1; "round16" Z rounded to
    16 mantissa bits before the split."""
    assert defect is None or defect in DEFECTS, defect
    x, w32, m = np.asarray(x, np.float32), np.asarray(w).astype(np.float32), np.asarray(m, np.float32)
    wl, n = len(w32), len(x)
    h, t = wl // 2, mask_frames(len(x), len(w32))
    assert m.shape == (h + 1, t), (m.shape, h + 1, t)
    gain = w32[0] + w32[h]
    if defect == "window_mirror":
        w32 = w32[(wl - np.arange(wl)) % wl]
    tp = t + (t & 1)   # (an odd frame count: the last frame pairs with zeros, under a mask of zeros)
    xp = np.zeros((tp + 1) * h, np.float32)
    xp[h:h + n] = x
    frames = xp[(np.arange(tp) * h)[:, None] + np.arange(wl)[None, :]] * w32
    z = plain.fft((frames[0::2] + 1j * frames[1::2]).astype(np.complex64), axis=-1)   # (tp / 2, W)
    if defect == "round16":
        z = round_mantissa(z, 16)
    full = np.zeros((wl, tp), np.float32)
    full[:h + 1, :t] = m
    if defect == "bin_h":
        full[h] = full[h - 1]
    full[h + 1:] = full[h - 1:0:-1]
    zn = np.conj(z[:, (wl - np.arange(wl)) % wl])
    a2, b2 = z + zn, np.complex64(-1j) * (z - zn)
    c = a2 * (np.float32(0.5) * full[:, 0::2].T) + np.complex64(1j) * (b2 * (np.float32(0.5) * full[:, 1::2].T))
    assert c.dtype == np.complex64
    back = plain.ifft(c, axis=-1)
    y = np.zeros((tp + 1) * h, np.float32)
    for j in range(tp // 2):
        y[2 * j * h:2 * j * h + wl] += back[j].real
        y[(2 * j + 1) * h:(2 * j + 1) * h + wl] += back[j].imag
    out = y[h:h + n] / gain
    assert out.dtype == np.float32
    return out


# ------------------------------------------------------------------------------------------------ the stereo packing, as a model
STEREO_DEFECTS = ("window_mirror", "channel_swap", "bin_h", "round16")


def stereo_model(x, w, m, defect=None):
    """y (N, 2) float32 by the stereo kernels' arithmetic in NumPy float32: per frame Z = FFT((L + i R) w), the two CHANNELS in one W-point
    transform.  One mask m (W/2 + 1, T) for both: C = m Z, never split.  Masks (2, W/2 + 1, T): A = (Z[k] + conj Z[W-k]) / 2,
    B = (Z[k] - conj Z[W-k]) / 2i, C = m_0 A + i m_1 B.  One inverse transform whose real part is L's masked frame and whose imaginary part
    is R's, overlap-add, the division by the COLA gain (zafx_maskfilter_stereo.hpp).  Not the kernels' bits: their rounding, order by order.

    defect, one at a time: "window_mirror" the window read at (W - n) % W; "channel_swap" with two masks, m_0 and m_1 exchanged (one mask:
    nothing to exchange); "bin_h" bin H's mask taken from bin H - 1; "round16" Z rounded to 16 mantissa bits before the masks."""
    assert defect is None or defect in STEREO_DEFECTS, defect
    x, w32, m = np.asarray(x, np.float32), np.asarray(w).astype(np.float32), np.asarray(m, np.float32)
    wl, n = len(w32), len(x)
    h, t = wl // 2, mask_frames(len(x), len(w32))
    assert x.shape == (n, 2) and m.shape[-2:] == (h + 1, t) and m.ndim in (2, 3), (x.shape, m.shape, h + 1, t)
    gain = w32[0] + w32[h]
    if defect == "window_mirror":
        w32 = w32[(wl - np.arange(wl)) % wl]
    if defect == "channel_swap" and m.ndim == 3:
        m = m[::-1]
    xp = np.zeros(((t + 1) * h, 2), np.float32)
    xp[h:h + n] = x
    frames = xp[(np.arange(t) * h)[:, None] + np.arange(wl)[None, :]] * w32[None, :, None]   # (T, W, 2)
    z = plain.fft((frames[..., 0] + 1j * frames[..., 1]).astype(np.complex64), axis=-1)   # (T, W)
    if defect == "round16":
        z = round_mantissa(z, 16)

    def mirrored(one):
        full = np.zeros((wl, t), np.float32)
        full[:h + 1] = one
        if defect == "bin_h":
            full[h] = full[h - 1]
        full[h + 1:] = full[h - 1:0:-1]
        return full.T
    if m.ndim == 2:
        c = z * mirrored(m)
    else:
        zn = np.conj(z[:, (wl - np.arange(wl)) % wl])
        a2, b2 = z + zn, np.complex64(-1j) * (z - zn)
        c = a2 * (np.float32(0.5) * mirrored(m[0])) + np.complex64(1j) * (b2 * (np.float32(0.5) * mirrored(m[1])))
    assert c.dtype == np.complex64
    back = plain.ifft(c, axis=-1)
    y = np.zeros(((t + 1) * h, 2), np.float32)
    for j in range(t):
        y[j * h:j * h + wl, 0] += back[j].real
        y[j * h:j * h + wl, 1] += back[j].imag
    out = y[h:h + n] / gain
    assert out.dtype == np.float32
    return out


def stereo_model_rows(x, w, m, defect=None):
    """stereo_model as a clip's (4, N) float32 rows: y_L, y_R, rest_L, rest_R."""
    y = stereo_model(x, w, m, defect)
    return np.ascontiguousarray(np.concatenate((y.T, (np.asarray(x, np.float32) - y).T)))
