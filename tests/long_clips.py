"""One clip, as long as the launchers' per-clip bounds: the harness of tests/test_gpu_long_clips.py (checked on the CPU by
tests/test_long_clips_host.py).

The launchers take their fast kernels only below fixed lengths of a single clip -- the kernels address a clip through one buffer descriptor
with 32-bit byte offsets, or count samples in 32 bits (BOUNDS below, read off zaf-python_amd/csrc/zafx_routes.hpp, which
tests/test_routes_host.py holds to every record on the CPU).  A clip that long has an output of 1 - 4 GiB,
and no oracle transforms it.  So the clip is PERIODIC:

    x[n] = p[n mod P],   P = Q hop,   Q = 7   (coprime to the 8-, 16- and 32-frame tiles: equal frames land on every position of a tile)

Every frame whose window lies wholly inside the clip then equals the frame Q frames before it, and the float64 oracle of the whole clip is
three short oracle results: the head frames (windows that start in front of the clip), ONE period of interior frames, served by index
t mod Q, and the tail frames (windows that reach past the end): periodic_reference.  It serves any range of frames or rows lazily -- the
reference of a 4 GiB output is a matrix of some twenty columns and an index.  The inverse transforms (ISTFT, IMDCT) take a spectrum whose frames
are periodic in the same way, and give samples that are: the same three pieces, per hop of samples.

The checking half is plain NumPy (FrameChecker, HopChecker): EVERY output element is compared, and every frame (hop of samples) is held to
a bound of its own,

    max_k |out[k, t] - ref[k, t]|  <=  tol max_k |ref[k, t]|  +  floor,      floor = C eps32 max|ref|
    || out[:, t] - ref[:, t] ||_2  <=  tol || ref[:, t] ||_2  +  floor sqrt(rows)

(tol: the project's 1e-5 for the transforms, 1e-4 for filterbanks and CQT; floor: the float32 floor of tests/test_gpu_signals.py, C_FLOOR = 2,
8 for the CQT's 32768-point frames).  A normwise bound over the clip would let one wrong frame among 131072 pass.  The bound does not depend
on the clip's length.  The output is prefilled with arena.FILL32 / FILL64: an element that still carries the fill was never written, and the row
padding of a row_align plan must still carry it.  A failure is a LongClipFailure that names the frame (row, element) -- what
tests/test_long_clips_host.py checks on doctored arrays.

The running half (device_clip, device_ragged, device_filled, walk_frames, walk_hops, assert_untouched) takes the zafx module as an argument, so this file
imports nothing from the GPU side.  The clip is built on the device: a block of a few MB of whole periods is uploaded once and doubled
with device-to-device copies; the host never holds the clip."""
import ctypes
import math

import numpy as np

import arena
from oracle import zaf_oracle as orc

Q = 7
TOL_FFT = 1e-5
TOL_FB = 1e-4
EPS32 = float(np.finfo(np.float32).eps)
C_FLOOR = 2.0
C_FLOOR_CQT = 8.0
FS = 44100
TONE = 0.05

FRAMED = ("stft", "stft_one_sided", "magnitude", "power", "mel", "mfcc", "mel_mfcc", "mdct", "cqt", "chroma")
INVERSE = ("istft", "istft_one_sided", "imdct")
KINDS = FRAMED + INVERSE + ("center",)
TOL = {k: TOL_FFT for k in ("stft", "stft_one_sided", "magnitude", "power", "mdct", "istft", "istft_one_sided", "imdct", "center")}
TOL.update({k: TOL_FB for k in ("mel", "mfcc", "mel_mfcc", "cqt", "chroma")})


class LongClipFailure(AssertionError):
    """What the checker found: `what` in ("fill", "padding", "finite", "bound", "coverage"), at frame (hop) `frame`, row / element `row`."""

    def __init__(self, what, frame, row, text):
        super().__init__(f"({what}) frame {frame}, row {row}: {text}")
        self.what, self.frame, self.row = what, frame, row


# ------------------------------------------------------------------------------------------------------------ the periodic clip
def period_block(hop, q=Q, seed=0, dtype=np.float32, channels=1):
    """One period p of q hop samples: seeded Gaussian noise of sigma 1 (conftest.synth_clip's scale) plus a tone of amplitude TONE with a whole
    number of cycles per period that is no whole number per hop.  The tone is kept at the level of the noise in the spectrum -- its bin of a
    Hamming frame of 2048 samples is about 28, a noise bin about 30 --, so that no single bin sets the level every frame is held to.  int16: the same at a sigma of 4000.  channels = 2: (P, 2), the right channel
    0.6 of the left plus noise of its own (a pan the center mask has to work on)."""
    n = q * hop
    rng = np.random.default_rng([seed, hop, q, channels])
    tone = TONE * np.sin(2.0 * np.pi * (5 * q + 3) * np.arange(n) / n)
    x = rng.standard_normal(n) + tone
    if channels == 2:
        x = np.stack([x, 0.6 * x + 0.5 * rng.standard_normal(n)], axis=1)
    if np.dtype(dtype).kind == "i":
        return np.clip(np.round(4000.0 * x), -32768, 32767).astype(dtype)
    return x.astype(dtype)


def periodic_clip(p, count, start=0):
    """Samples start ... start + count - 1 of the periodic clip, on the host (short pieces only)."""
    return np.asarray(p)[(int(start) + np.arange(int(count))) % len(p)]


# ------------------------------------------------------------------------------------------------------------ the oracle in three pieces
def _half(w):
    return len(w) // 2 + 1


def _oracle_frames(kind, x, prm):
    """The plain float64 oracle of `kind` on the host clip x: (rows, T)."""
    x = np.asarray(x, np.float64)
    if kind in ("stft", "stft_one_sided", "magnitude", "power"):
        s = orc.stft(x, prm["w"], prm["hop"])
        if kind == "stft":
            return s
        s = s[:_half(prm["w"])]
        return s if kind == "stft_one_sided" else np.abs(s) if kind == "magnitude" else np.abs(s) ** 2
    if kind == "mel":
        return orc.melspectrogram(x, prm["w"], prm["hop"], prm["fb"])
    if kind == "mfcc":
        return orc.mfcc(x, prm["w"], prm["hop"], prm["fb"], prm["ncoef"])
    if kind == "mel_mfcc":   # (the one-pass plan's rows: the mel bands, then the coefficients)
        return np.concatenate([orc.melspectrogram(x, prm["w"], prm["hop"], prm["fb"]), orc.mfcc(x, prm["w"], prm["hop"], prm["fb"], prm["ncoef"])])
    if kind == "mdct":
        return orc.mdct(x, prm["w"])
    if kind == "cqt":
        return orc.cqtspectrogram(x, prm["fs"], prm["tr"], prm["ck"])
    if kind == "chroma":
        return orc.cqtchromagram(x, prm["fs"], prm["tr"], prm["octave"], prm["ck"])
    raise ValueError(kind)


def geometry(kind, prm):
    """(step, left, length, frames_of): frame t of `kind` is the `length` samples from t step - left; frames_of(n) frames in a clip of n."""
    if kind in ("mdct", "imdct"):
        wl = len(prm["w"])
        return wl // 2, wl // 2, wl, lambda n: orc.mdct_num_frames(n, wl)
    if kind in ("cqt", "chroma"):
        step, fft_len = round(prm["fs"] / prm["tr"]), prm["ck"].shape[1]
        return step, int(math.ceil((fft_len - step) / 2)), fft_len, lambda n: n // step
    wl, hop = len(prm["w"]), prm["hop"]
    return hop, wl // 2, wl, lambda n: orc.stft_num_frames(n, wl, hop)


def frames_of(kind, n, **prm):
    return geometry(kind, prm)[3](int(n))


class PeriodicRef:
    """The oracle's result of the long clip, never materialised: `small` holds the distinct columns (head | one period | tail), idx[t] the
    column of frame (hop) t.  ref(t0, t1[, r0, r1]) -> the float64 (complex128) values of those frames and rows; `first`, `last`: the range
    of frames served by index t mod q (empty when the clip is too short to have one: then `small` is the plain oracle's result)."""

    def __init__(self, small, idx, first, last, q, n_out=None):
        self.small, self.idx, self.first, self.last, self.q = small, idx, int(first), int(last), int(q)
        self.rows, self.frames = small.shape[0], len(idx)
        self.n_out = n_out
        self.peak = float(np.abs(small).max()) if small.size else 0.0

    def __call__(self, t0, t1, r0=0, r1=None):
        return self.small[r0:r1][:, self.idx[t0:t1]]

    def hops(self, m0, m1):
        """Inverse kinds: hops m0 ... m1 - 1 as rows of one hop of samples each (the last hop of the clip zero-filled)."""
        return self.small[:, self.idx[m0:m1]].T


def _pieces(head, tail, first, last, q, total, tail_from):
    """small = head[:, :first + q] | tail[:, tail_from:], and the index: t < first -> t; first <= t < last -> first + (t - first) mod q; else the tail."""
    small = np.concatenate([head[:, :first + q], tail[:, tail_from:]], axis=1)
    t = np.arange(total)
    idx = np.where(t < first, t, np.where(t < last, first + (t - first) % q, first + q + (t - last)))
    assert small.shape[1] == first + q + (total - last), (small.shape, first, q, total, last)
    return small, idx.astype(np.int64)


def framed_reference(kind, p, n, **prm):
    """periodic_reference of the kinds that cut the clip into frames."""
    step, left, length, count = geometry(kind, prm)
    n, period = int(n), len(p)
    if period % step:
        raise ValueError("the period must be a whole number of steps")
    q = period // step
    total = count(n)
    first = -(-left // step)                                    # frames 0 ... first - 1 start in front of the clip
    last = (n - length + left) // step + 1 if n - length + left >= 0 else 0   # frames last ... reach past its end
    last = min(max(last, first), total)
    if last - first < q:                                        # no whole period of interior frames: the plain oracle
        ref = _oracle_frames(kind, periodic_clip(p, n), prm)
        return PeriodicRef(ref, np.arange(total, dtype=np.int64), 0, 0, q)
    n_head = (first + q - 1) * step - left + length             # through the end of frame first + q - 1 (inside the clip: that frame is interior)
    while count(n_head) < first + q:
        n_head += step
    head = _oracle_frames(kind, periodic_clip(p, min(n_head, n)), prm)
    n0 = (last * step - left) // period * period                # a whole number of periods in front of the first tail frame
    tail = _oracle_frames(kind, periodic_clip(p, n - n0), prm)
    assert tail.shape[1] == total - n0 // step, (tail.shape, total, n0, step)
    small, idx = _pieces(head, tail, first, last, q, total, last - n0 // step)
    return PeriodicRef(small, idx, first, last, q)


def _inverse(kind, spec, prm):
    """The oracle's inverse of a short block of frames, as hops: (hop, count) -- the last hop zero-filled -- and the number of samples."""
    if kind == "imdct":
        y, hop = orc.imdct(spec, prm["w"]), len(prm["w"]) // 2
    else:
        if kind == "istft_one_sided":
            spec = np.concatenate([spec, np.conj(spec[-2:0:-1])], axis=0)
        y, hop = orc.istft(spec, prm["w"], prm["hop"]), prm["hop"]
    m = -(-len(y) // hop)
    return np.pad(y, (0, m * hop - len(y))).reshape(m, hop).T, len(y)


def inverse_reference(kind, spectrum, **prm):
    """periodic_reference of ISTFT / IMDCT: `spectrum` is the PeriodicRef of the input frames (stft, stft_one_sided or mdct of the periodic
    clip).  Hop m of the output is the overlap-add of frames m ... m + r - 1 (r = W / H; 2 for the IMDCT), so it is periodic wherever those are."""
    wl = len(prm["w"])
    hop = wl // 2 if kind == "imdct" else prm["hop"]
    if wl % hop:
        raise ValueError("the hop must divide the window")
    r, q, total = wl // hop, spectrum.q, spectrum.frames
    n_out = max(hop * (total - 1) - 1, 0) if kind == "imdct" else max(total * hop - (wl - hop), 0)
    n_hops = -(-n_out // hop)
    first, last = spectrum.first, spectrum.last - r + 1          # hops first ... last - 1 take interior frames only
    if last - first < q:
        y, n = _inverse(kind, spectrum(0, total), prm)
        assert n == n_out
        return PeriodicRef(y, np.arange(n_hops, dtype=np.int64), 0, 0, q, n_out)
    head, _ = _inverse(kind, spectrum(0, first + q + r), prm)
    t0 = first + (last - first) // q * q                         # a whole number of periods behind `first`, not behind `last`
    tail, n_tail = _inverse(kind, spectrum(t0, total), prm)
    assert n_tail == n_out - t0 * hop, (n_tail, n_out, t0, hop)
    small, idx = _pieces(head, tail, first, last, q, n_hops, last - t0)
    return PeriodicRef(small, idx, first, last, q, n_out)


def center_reference(p, n, **prm):
    """periodic_reference of the center extraction (center_oracle.oracle_center; sides=True: of the sides, input - center): p is (P, 2), the
    result n sample frames of (L, R).  A hop
    of the output -- h = W / 2 sample frames, both channels: 2 h values -- takes the two frames that cover it; hops 2 ... n / h - 4 are periodic."""
    from center_oracle import oracle_center
    w = prm["w"]
    h, n, period = len(w) // 2, int(n), len(p)
    if period % h:
        raise ValueError("the period must be a whole number of hops")
    q, n_hops = period // h, -(-n // h)

    sides = bool(prm.get("sides"))

    def hops_of(start, count):
        x = periodic_clip(p, count, start).astype(np.float64)
        y = oracle_center(x, w)
        if sides:   # (zaf.py:198: what the center leaves of the input)
            y = x - y
        m = -(-count // h)
        return np.pad(y, ((0, m * h - count), (0, 0))).reshape(m, 2 * h).T

    first, last = 2, n // h - 3
    if last - first < 2 * q:
        return PeriodicRef(hops_of(0, n), np.arange(n_hops, dtype=np.int64), 0, 0, q, n)
    head = hops_of(0, (first + q + 3) * h)
    t0 = first + ((last - first) // q - 1) * q                   # one period early: the short clip's own first hops are not used
    tail = hops_of(t0 * h, n - t0 * h)
    small, idx = _pieces(head, tail, first, last, q, n_hops, last - t0)
    return PeriodicRef(small, idx, first, last, q, n)


def periodic_reference(kind, p, n, **prm):
    """The float64 oracle of `kind` on the periodic clip of n samples with period block p, as a PeriodicRef.  Parameters: w (window), hop;
    fb, ncoef (mel kinds); fs, tr, ck, octave (CQT kinds).  The inverse kinds take the oracle's own forward transform of the clip as input."""
    if kind in FRAMED:
        return framed_reference(kind, p, n, **prm)
    if kind in ("istft", "istft_one_sided"):
        return inverse_reference(kind, framed_reference("stft" if kind == "istft" else "stft_one_sided", p, n, **prm), **prm)
    if kind == "imdct":
        return inverse_reference(kind, framed_reference("mdct", p, n, **prm), **prm)
    if kind == "center":
        return center_reference(p, n, **prm)
    raise ValueError(kind)


def plain_oracle(kind, x, **prm):
    """The same result from the plain oracle on the whole host clip (small sizes: what tests/test_long_clips_host.py compares with):
    (rows, T), or (values per hop, hops) for the inverse kinds and the center."""
    if kind in FRAMED:
        return _oracle_frames(kind, x, prm)
    if kind in ("istft", "istft_one_sided"):
        return _inverse(kind, _oracle_frames("stft" if kind == "istft" else "stft_one_sided", x, prm), prm)[0]
    if kind == "imdct":
        return _inverse(kind, _oracle_frames("mdct", x, prm), prm)[0]
    from center_oracle import oracle_center
    h = len(prm["w"]) // 2
    y = oracle_center(np.asarray(x, np.float64), prm["w"])
    m = -(-len(y) // h)
    return np.pad(y, ((0, m * h - len(y)), (0, 0))).reshape(m, 2 * h).T


# ------------------------------------------------------------------------------------------------------------ the checker
def floor_of(kind, ref):
    return (C_FLOOR_CQT if kind in ("cqt", "chroma") else C_FLOOR) * EPS32 * ref.peak


def _carries_fill(a):
    """Elementwise: does the element (complex: either part) still carry the output fill?"""
    a = np.ascontiguousarray(a)
    wdtype, value = arena.fill_word(a.dtype)
    words = a.dtype.itemsize // wdtype.itemsize
    return (a.view(wdtype).reshape(a.shape + (words,)) == value).any(axis=-1)


class FrameChecker:
    """A (rows, pitch) output against ref, walked in chunks of rows: add(r0, got) takes rows r0 ... of the device array as they lie (pitch
    columns, the first ref.frames of them the clip's); finish() holds every frame to its bound.  Fill left inside, padding written and values
    that are not finite fail at once, at their (row, frame)."""

    def __init__(self, ref, tol, floor):
        self.ref, self.tol, self.floor = ref, float(tol), float(floor)
        self.err = np.zeros(ref.frames)
        self.err2 = np.zeros(ref.frames)   # the frame's squared error norm
        self.level2 = np.sqrt((np.abs(ref.small) ** 2).sum(axis=0))[ref.idx] if ref.small.size else np.zeros(ref.frames)
        self.level = np.abs(ref.small).max(axis=0)[ref.idx] if ref.small.size else np.zeros(ref.frames)   # (every row is compared: finish)
        self.seen = np.zeros(ref.rows, bool)

    def add(self, r0, got):
        got = np.asarray(got)
        t, r1 = self.ref.frames, r0 + got.shape[0]
        if got.ndim != 2 or got.shape[1] < t or r1 > self.ref.rows or self.seen[r0:r1].any():
            raise LongClipFailure("coverage", None, r0, f"rows {r0}:{r1} of shape {got.shape} do not fit {self.ref.rows} x {t}, or came twice")
        self.seen[r0:r1] = True
        wdtype, value = arena.fill_word(got.dtype)
        if got.shape[1] > t or (np.ascontiguousarray(got).view(wdtype) == value).any():   # (one pass where nothing carries the fill and there is no padding)
            carries = _carries_fill(got)
            if carries[:, :t].any():
                r, f = np.argwhere(carries[:, :t])[0]
                raise LongClipFailure("fill", int(f), r0 + int(r), f"{int(carries[:, :t].sum())} elements of rows {r0}:{r1} never written")
            if not carries[:, t:].all():
                r, f = np.argwhere(~carries[:, t:])[0]
                raise LongClipFailure("padding", t + int(f), r0 + int(r), f"{int((~carries[:, t:]).sum())} row-padding elements of rows {r0}:{r1} written")
        val = got[:, :t]
        want = self.ref(0, t, r0, r1)
        dist = np.abs(val - want)
        err = dist.max(axis=0)
        if not np.isfinite(err).all():   # (a NaN or an infinity anywhere in a frame shows in its maximum)
            bad = ~np.isfinite(val)
            r, f = np.argwhere(bad)[0]
            raise LongClipFailure("finite", int(f), r0 + int(r), f"{int(bad.sum())} values of rows {r0}:{r1} not finite")
        np.maximum(self.err, err, out=self.err)
        dist *= dist
        self.err2 += dist.sum(axis=0)

    def finish(self):
        if not self.seen.all():
            raise LongClipFailure("coverage", None, int(np.flatnonzero(~self.seen)[0]), f"{int((~self.seen).sum())} rows never compared")
        # both per frame: the largest error against the largest value, and the error's 2-norm against the frame's (a floor per element)
        worst = _hold(self.err, self.level, self.tol, self.floor, 0)
        return max(worst, _hold(np.sqrt(self.err2), self.level2, self.tol, self.floor * np.sqrt(self.ref.rows), 0))


def _hold(err, level, tol, floor, t0):
    """Every frame within tol level + floor; -> the worst frame's share of its bound."""
    bound = tol * level + floor
    over = err > bound
    if over.any():
        f = int(np.flatnonzero(over)[0])
        raise LongClipFailure("bound", t0 + f, None, f"{int(over.sum())} frames over their bound, the first off by {err[f]:.3e} at a level of "
                              f"{level[f]:.3e}: {err[f] / level[f] if level[f] else np.inf:.3e} relative, bound {bound[f]:.3e}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.max(np.where(bound > 0, err / bound, 0.0))) if len(err) else 0.0


class HopChecker:
    """A 1-D output (samples; the center: interleaved sample frames) against ref, walked in chunks of whole hops: add(m0, got) takes the
    values of hops m0 ... as they lie (the clip's last hop may be short); every hop is held to its bound at once."""

    def __init__(self, ref, tol, floor):
        self.ref, self.tol, self.floor = ref, float(tol), float(floor)
        self.width = ref.small.shape[0]
        self.next, self.worst = 0, 0.0

    def add(self, m0, got):
        got = np.asarray(got).reshape(-1)
        if m0 != self.next:
            raise LongClipFailure("coverage", m0, None, f"hops {self.next}:{m0} skipped or repeated")
        m1 = m0 + -(-len(got) // self.width)
        if m1 > self.ref.frames or (len(got) % self.width and m1 != self.ref.frames):
            raise LongClipFailure("coverage", m0, None, f"{len(got)} values from hop {m0} do not fit {self.ref.frames} hops of {self.width}")
        self.next = m1
        carries = _carries_fill(got)
        if carries.any():
            i = int(np.flatnonzero(carries)[0])
            raise LongClipFailure("fill", m0 + i // self.width, i % self.width, f"{int(carries.sum())} elements of hops {m0}:{m1} never written")
        bad = ~np.isfinite(got)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise LongClipFailure("finite", m0 + i // self.width, i % self.width, f"{int(bad.sum())} values of hops {m0}:{m1} not finite")
        want = self.ref.hops(m0, m1)
        val = np.zeros(want.shape)
        val.reshape(-1)[:len(got)] = got
        if len(got) < val.size:   # (the clip's last hop: the oracle's zero fill stands in for what the output does not have)
            val.reshape(-1)[len(got):] = want.reshape(-1)[len(got):]
        dist = np.abs(val - want)
        self.worst = max(self.worst, _hold(dist.max(axis=1), np.abs(want).max(axis=1), self.tol, self.floor, m0),
                         _hold(np.sqrt((dist * dist).sum(axis=1)), np.sqrt((want * want).sum(axis=1)), self.tol, self.floor * np.sqrt(self.width), m0))

    def finish(self):
        if self.next != self.ref.frames:
            raise LongClipFailure("coverage", self.next, None, f"hops {self.next}:{self.ref.frames} never compared")
        return self.worst


def check_frames(out, ref, tol, floor, chunk_rows=64):
    """A whole (rows, pitch) host array through FrameChecker (the host tests' form)."""
    ck = FrameChecker(ref, tol, floor)
    for r0 in range(0, out.shape[0], chunk_rows):
        ck.add(r0, out[r0:r0 + chunk_rows])
    return ck.finish()


def check_hops(out, ref, tol, floor, chunk_hops=16):
    """A whole 1-D host array through HopChecker."""
    ck = HopChecker(ref, tol, floor)
    out = np.asarray(out).reshape(-1)
    step = chunk_hops * ck.width
    for i in range(0, max(len(out), 1), step):
        ck.add(i // ck.width, out[i:i + step])
    return ck.finish()


# ------------------------------------------------------------------------------------------------------------ the bounds table
# One record per condition of a launcher that depends on the length of ONE clip (float32, layout "FT", one clip, arrays on 256 bytes).
#   cond       the condition restated in Python: cond(n) -> the launcher takes `kernel_below`'s route
#   on_route   the lengths this record speaks about (alignment, rows on or off the line grid): both n_below and n_above satisfy it
#   n_below    the largest length on the route that satisfies cond;  n_above  the smallest one that violates it
#   above      what runs at n_above: a kernel name (the same name where the launcher switches to the kernel's other instantiation), or "refused"
# Where two conditions of one launcher coincide, `note` says so and the hop separates them as far as it can.
def _t(n, w, hop):
    return orc.stft_num_frames(n, w, hop)


def _tm(n, w):
    return orc.mdct_num_frames(n, w)


def _pitch(t, align):
    return -(-t // align) * align if align > 1 else t


def _search(cond, on_route, lo, hi):
    """(n_below, n_above) of a condition that holds at lo and fails at hi and changes once between them: bisection over the lengths on the route."""
    assert cond(lo) and not cond(hi), (lo, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if cond(mid) else (lo, mid)
    below, above = lo, hi
    while not on_route(below):
        below -= 1
    while not on_route(above):
        above += 1
    return below, above


def _bound(name, kind, w, hop, options, cond, text, source, kernel_below, above, lo, hi, on_route=lambda n: True, route="any length", note="", layout="FT"):
    n_below, n_above = _search(cond, on_route, lo, hi)
    return dict(name=name, kind=kind, W=w, hop=hop, layout=layout, options=options, cond=cond, condition=text, source=source, on_route=on_route,
                route=route, n_below=n_below, n_above=n_above, kernel_below=kernel_below, above=above, note=note)


_LO, _HI = 1 << 20, 9 << 28
BOUNDS = [
    # |X| and |X|^2 at W = 2048 run on k_mel2 (spec2_usable) below 2^29 samples, on k_stft_ft16's magnitude / power forms above.  The hop is W,
    # so the output stays at 1 GiB; spec2_usable has no condition on T H, so nothing coincides.
    _bound("stft_magnitude_2048", "magnitude", 2048, 2048, dict(row_align=0), lambda n: n < 1 << 29, "n_samples < 2^29", "zafx_routes.hpp:spec2_usable",
           "k_mel2", "k_stft_ft16", _LO, _HI),
    _bound("stft_power_2048_padded", "power", 2048, 2048, dict(row_align=32), lambda n: n < 1 << 29, "n_samples < 2^29", "zafx_routes.hpp:spec2_usable",
           "k_mel2", "k_stft_ft16", _LO, _HI),
    # Complex rows off the line grid (compact, T % 16 != 0) run on k_stft_ft16c: its buffer-load form below the bound, its pointer form above
    # (one kernel name, two instantiations).  T H >= n + H at every hop, so `n_samples < 2^29` never decides: it is implied by T H < 2^29.
    # The lengths between n_below and n_above give T = 2^18, rows of whole lines, which k_stft_ft16 takes: they are not on this route.
    _bound("stft_one_sided_2048_carry", "stft_one_sided", 2048, 2048, dict(row_align=0), lambda n: n < 1 << 29 and _t(n, 2048, 2048) * 2048 < 1 << 29,
           "n_samples < 2^29 and T H < 2^29 (even n)", "zafx_routes.hpp:frames_addressable", "k_stft_ft16c", "k_stft_ft16c", _LO, _HI,
           on_route=lambda n: n % 2 == 0 and _t(n, 2048, 2048) % 16 != 0, route="n even, T no multiple of 16",
           note="n_samples < 2^29 is implied by T H < 2^29 (T H >= n + H); T = 2^18 lies between the two lengths and runs k_stft_ft16"),
    _bound("stft_two_sided_2048_carry", "stft", 2048, 2048, dict(row_align=0), lambda n: n < 1 << 29 and _t(n, 2048, 2048) * 2048 < 1 << 29,
           "n_samples < 2^29 and T H < 2^29 (even n)", "zafx_routes.hpp:frames_addressable", "k_stft_ft16c", "k_stft_ft16c", _LO, _HI,
           on_route=lambda n: n % 2 == 0 and _t(n, 2048, 2048) % 16 != 0, route="n even, T no multiple of 16",
           note="as the one-sided record; 4 GiB of output"),
    # The forward STFT at W = 4096 and 8192: these conditions carry the 16-frame halo of the tile the kernels read ahead ((T + 16) H); the
    # generic one-workgroup-per-tile k_stft above.  T H >= n + H, so `n_samples < 2^29` never decides.  Hop W keeps the outputs at 0.5 - 2 GiB.
    _bound("stft_one_sided_4096_carry", "stft_one_sided", 4096, 4096, dict(row_align=0), lambda n: n < 1 << 29 and (_t(n, 4096, 4096) + 16) * 4096 < 1 << 29,
           "n_samples < 2^29 and (T + 16) H < 2^29", "zafx_routes.hpp:band_addressable", "k_stft_ft16bc", "k_stft", _LO, _HI,
           on_route=lambda n: _t(n, 4096, 4096) % 16 != 0, route="T no multiple of 16", note="n_samples < 2^29 is implied by (T + 16) H < 2^29"),
    _bound("stft_magnitude_4096", "magnitude", 4096, 4096, dict(row_align=0), lambda n: n < 1 << 29 and (_t(n, 4096, 4096) + 16) * 4096 < 1 << 29,
           "n_samples < 2^29 and (T + 16) H < 2^29", "zafx_routes.hpp:band_addressable", "k_stft_ft16b", "k_stft", _LO, _HI, note="n_samples < 2^29 is implied"),
    _bound("stft_magnitude_8192", "magnitude", 8192, 8192, dict(row_align=0), lambda n: n < 1 << 29 and (_t(n, 8192, 8192) + 16) * 8192 < 1 << 28,
           "n_samples < 2^29 and (T + 16) H < 2^28", "zafx_routes.hpp:quad_addressable", "k_stft_ft16q", "k_stft", _LO, _HI, note="n_samples < 2^29 is implied"),
    # mel at W = 4096: the fused two-band kernel k_mel_ft16b with the same halo; the spectrum kernel + k_melfb above
    _bound("mel_4096", "mel", 4096, 2048, dict(), lambda n: n < 1 << 29 and (_t(n, 4096, 2048) + 16) * 2048 < 1 << 29,
           "n_samples < 2^29 and (T + 16) H < 2^29", "zafx_routes.hpp:mel_band_usable", "k_mel_ft16b", "k_melfb", _LO, _HI, note="n_samples < 2^29 is implied"),
    # ISTFT at W = 2048: the carry kernel k_istft_ft16 addresses the clip's spectrum -- counted as W rows, one-sided too -- through one
    # descriptor with signed 32-bit byte offsets; the generic k_istft above.  The condition is on the row pitch: T here, T rounded up to 16
    # for a row_align plan.  Lengths are those of the clip whose STFT is inverted (hop 1024: T = n / 1024 + 1 for n a multiple of 1024).
    _bound("istft_2048", "istft", 2048, 1024, dict(row_align=0), lambda n: 2048 * _t(n, 2048, 1024) * 8 < 1 << 31, "W pitch 8 < 2^31",
           "zafx_routes.hpp:spectrum_addressable", "k_istft_ft16", "k_istft", _LO, _HI, on_route=lambda n: n % 1024 == 0, route="n a multiple of the hop"),
    _bound("istft_one_sided_2048_padded", "istft_one_sided", 2048, 1024, dict(row_align=16), lambda n: 2048 * _pitch(_t(n, 2048, 1024), 16) * 8 < 1 << 31,
           "W pitch 8 < 2^31 (W rows counted for a one-sided spectrum too)", "zafx_routes.hpp:spectrum_addressable", "k_istft_ft16", "k_istft", _LO, _HI,
           on_route=lambda n: n % 1024 == 0, route="n a multiple of the hop"),
    # W = 4096 at hop W / 2 (the two-class kernel k_istft_ft16d; the band form k_istft_ft16b has the same condition) and W = 8192 at hop W / 2
    # (the four-class kernel k_istft_ft8q): 32-bit byte offsets inside a clip's spectrum, the generic k_istft above
    _bound("istft_4096", "istft", 4096, 2048, dict(row_align=0), lambda n: 4096 * _t(n, 4096, 2048) * 8 < 1 << 31, "4096 pitch 8 < 2^31",
           "zafx_routes.hpp:spectrum_addressable", "k_istft_ft16d", "k_istft", _LO, _HI, on_route=lambda n: n % 2048 == 0, route="n a multiple of the hop"),
    _bound("istft_one_sided_4096", "istft_one_sided", 4096, 2048, dict(row_align=0), lambda n: 4096 * _t(n, 4096, 2048) * 8 < 1 << 31,
           "4096 pitch 8 < 2^31 (W rows counted for a one-sided spectrum too)", "zafx_routes.hpp:spectrum_addressable", "k_istft_ft16d", "k_istft", _LO, _HI,
           on_route=lambda n: n % 2048 == 0, route="n a multiple of the hop"),
    _bound("istft_8192", "istft", 8192, 4096, dict(row_align=0), lambda n: 8192 * _t(n, 8192, 4096) * 8 < 1 << 31, "8192 pitch 8 < 2^31",
           "zafx_routes.hpp:spectrum_addressable", "k_istft_ft8q", "k_istft", _LO, _HI, on_route=lambda n: n % 4096 == 0, route="n a multiple of the hop"),
    _bound("istft_one_sided_8192", "istft_one_sided", 8192, 4096, dict(row_align=0), lambda n: 8192 * _t(n, 8192, 4096) * 8 < 1 << 31,
           "8192 pitch 8 < 2^31 (W rows counted for a one-sided spectrum too)", "zafx_routes.hpp:spectrum_addressable", "k_istft_ft8q", "k_istft", _LO, _HI,
           on_route=lambda n: n % 4096 == 0, route="n a multiple of the hop"),
    # W = 4096 at another hop (a multiple of 4, at least 512): the band form k_istft_ft16b, the same condition
    _bound("istft_4096_band", "istft", 4096, 1024, dict(row_align=0), lambda n: 4096 * _t(n, 4096, 1024) * 8 < 1 << 31, "4096 pitch 8 < 2^31",
           "zafx_routes.hpp:spectrum_addressable", "k_istft_ft16b", "k_istft", _LO, _HI, on_route=lambda n: n % 1024 == 0, route="n a multiple of the hop"),
    # MDCT at W = 2048: k_mdct_ft32's 16-byte buffer loads below 2^28 samples, its 4-byte edge form above (one kernel name)
    _bound("mdct_2048", "mdct", 2048, 1024, dict(row_align=32), lambda n: n < 1 << 28, "n_samples < 2^28 (n a multiple of 4)", "zafx_routes.hpp:mdct_aligned",
           "k_mdct_ft32", "k_mdct_ft32", _LO, _HI, on_route=lambda n: n % 4 == 0, route="n a multiple of 4"),
    # the same on compact rows off the 64-byte grid (T = 262145): the carry instantiation below the bound, the plain 4-byte form above
    _bound("mdct_2048_carry", "mdct", 2048, 1024, dict(row_align=0), lambda n: n < 1 << 28, "n_samples < 2^28 (n a multiple of 4)", "zafx_routes.hpp:mdct_aligned",
           "k_mdct_ft32", "k_mdct_ft32", _LO, _HI, on_route=lambda n: n % 4 == 0 and _tm(n, 2048) % 16 != 0, route="n a multiple of 4, T no multiple of 16"),
    # MDCT at W = 4096: the two-band kernels (16-byte buffer loads) below 2^28 samples -- whole half lines: k_mdct_ft32b, compact rows off them:
    # the carry form k_mdct_ft32bc --, the generic k_mdct above
    _bound("mdct_4096", "mdct", 4096, 2048, dict(row_align=32), lambda n: n < 1 << 28, "n_samples < 2^28 (n a multiple of 4)", "zafx_routes.hpp:mdct_aligned",
           "k_mdct_ft32b", "k_mdct", _LO, _HI, on_route=lambda n: n % 4 == 0, route="n a multiple of 4"),
    _bound("mdct_4096_carry", "mdct", 4096, 2048, dict(row_align=0), lambda n: n < 1 << 28, "n_samples < 2^28 (n a multiple of 4)", "zafx_routes.hpp:mdct_aligned",
           "k_mdct_ft32bc", "k_mdct", _LO, _HI, on_route=lambda n: n % 4 == 0 and _tm(n, 4096) % 16 != 0, route="n a multiple of 4, T no multiple of 16"),
    # MDCT at W = 8192: the four-class kernel k_mdct_ft32q reads 33 frames of halo through the clip's descriptor; the generic k_mdct above.
    # (T + 33) 4096 >= n + 34 * 4096, so `n_samples < 2^28` never decides: it is implied.
    _bound("mdct_8192", "mdct", 8192, 4096, dict(row_align=32), lambda n: n < 1 << 28 and (_tm(n, 8192) + 33) * 4096 < 1 << 28,
           "n_samples < 2^28 and (T + 33) 4096 < 2^28", "zafx_routes.hpp:mdct_route", "k_mdct_ft32q", "k_mdct", _LO, _HI,
           note="n_samples < 2^28 is implied by (T + 33) 4096 < 2^28"),
    # IMDCT at W = 8192: k_imdct_q (four frames per 16-byte piece: a pitch that is a multiple of 4) with 32-bit byte offsets inside a clip's
    # coefficients, the generic k_imdct above
    _bound("imdct_8192", "imdct", 8192, 4096, dict(row_align=0), lambda n: 4096 * _tm(n, 8192) * 4 < 1 << 31, "4096 pitch 4 < 2^31 (pitch a multiple of 4)",
           "zafx_routes.hpp:imdct_route", "k_imdct_q", "k_imdct", _LO, _HI, on_route=lambda n: n % 4096 == 0 and _tm(n, 8192) % 4 == 0,
           route="n a multiple of the hop, T a multiple of 4"),
    # IMDCT at W = 2048: k_imdct's 16-byte gather while a clip's coefficients stay below 2^32 bytes, its 4-byte gather above (one kernel name).
    # The only 2^32 bound of the equal-length launchers: 4 GiB of coefficients and 4 GiB of samples.
    _bound("imdct_2048", "imdct", 2048, 1024, dict(row_align=32, split=True), lambda n: 1024 * _pitch(_tm(n, 2048), 32) * 4 < 1 << 32, "M pitch 4 < 2^32",
           "zafx_mdct.hip:k_imdct", "k_imdct", "k_imdct", _LO, _HI, on_route=lambda n: n % 1024 == 0, route="n a multiple of the hop"),
    # mel / MFCC at W = 2048: the aligned form of the fused kernel below 2^29 samples, the pointer form above (one kernel name)
    _bound("mel_2048", "mel", 2048, 1024, dict(), lambda n: n < 1 << 29, "n_samples < 2^29 (even n)", "zafx_routes.hpp:mel_aligned", "k_mel2", "k_mel2", _LO, _HI,
           on_route=lambda n: n % 2 == 0, route="n even"),
    _bound("mfcc_2048", "mfcc", 2048, 1024, dict(), lambda n: n < 1 << 29, "n_samples < 2^29 (even n)", "zafx_routes.hpp:mel_aligned", "k_mel2", "k_mel2", _LO, _HI,
           on_route=lambda n: n % 2 == 0, route="n even"),
    _bound("mel_mfcc_2048", "mel_mfcc", 2048, 1024, dict(), lambda n: n < 1 << 29, "n_samples < 2^29 (even n)", "zafx_routes.hpp:mel_aligned", "k_mel2", "k_mel2",
           _LO, _HI, on_route=lambda n: n % 2 == 0, route="n even"),
    # int16 PCM on the device (zafx_execute_pcm, mono): the integers are read in the kernels' own loads below the bound; above it the clip is
    # converted into the plan's float32 staging array first and takes the float route.  (The STFT's T H < 2^29 implies n_frames < 2^29.)
    _bound("stft_pcm16_one_sided_2048", "stft_one_sided", 2048, 2048, dict(row_align=16, pcm=True), lambda n: n < 1 << 29 and _t(n, 2048, 2048) * 2048 < 1 << 29,
           "n_frames < 2^29 and T H < 2^29 (even n_frames)", "zafx_routes.hpp:stft_pcm_direct_ok", "k_stft_ft16", "k_stft_ft16", _LO, _HI,
           on_route=lambda n: n % 2 == 0, route="n even", note="n_frames < 2^29 is implied by T H < 2^29"),
    _bound("mel_pcm16_2048", "mel", 2048, 1024, dict(pcm=True), lambda n: n < 1 << 29, "n_frames < 2^29", "zafx_routes.hpp:pcm_direct_ok", "k_mel2", "k_mel2", _LO, _HI),
    _bound("stft_pcm16_magnitude_2048", "magnitude", 2048, 2048, dict(row_align=0, pcm=True), lambda n: n < 1 << 29, "n_frames < 2^29", "zafx_routes.hpp:pcm_direct_ok",
           "k_mel2", "k_stft_ft16", _LO, _HI),
    _bound("mdct_pcm16_2048", "mdct", 2048, 1024, dict(row_align=32, pcm=True), lambda n: n < 1 << 28, "n_frames < 2^28 (a multiple of 4)",
           "zafx_routes.hpp:mdct_pcm_direct_ok", "k_mdct_ft32", "k_mdct_ft32", _LO, _HI, on_route=lambda n: n % 4 == 0, route="n a multiple of 4"),
    # CQT / chromagram: refused from 2^29 samples on
    _bound("cqt", "cqt", 0, 1764, dict(), lambda n: n < 1 << 29, "n_samples < 2^29", "zafx_routes.hpp:cqt_clip_refused", "k_cqt", "refused", _LO, _HI),
    _bound("chroma", "chroma", 0, 1764, dict(), lambda n: n < 1 << 29, "n_samples < 2^29", "zafx_routes.hpp:cqt_clip_refused", "k_cqt", "refused", _LO, _HI),
    # center: refused from 2^28 sample frames on
    _bound("center_2048", "center", 2048, 1024, dict(sides=False), lambda n: n < 1 << 28, "n_samples < 2^28 (sample frames)", "zafx_routes.hpp:center_clip_refused",
           "k_center", "refused", _LO, _HI),
    _bound("center_sides_2048", "center", 2048, 1024, dict(sides=True), lambda n: n < 1 << 28, "n_samples < 2^28 (sample frames)", "zafx_routes.hpp:center_clip_refused",
           "k_center", "refused", _LO, _HI),
]
BOUND_NAMES = [b["name"] for b in BOUNDS]


def bound(name):
    return BOUNDS[BOUND_NAMES.index(name)]


# ------------------------------------------------------------------------------------------------------------ the running half (needs the zafx module)
BLOCK_BYTES = 4 << 20


def _replicate(buf, block, offset=0, nbytes=None):
    """Fill `nbytes` of the DeviceBuffer `buf` from byte `offset` on (default: all of it) with the host bytes `block` repeated: one upload, then
    device-to-device copies that double what is there."""
    block = np.ascontiguousarray(block).view(np.uint8).reshape(-1)
    nbytes = buf.nbytes - offset if nbytes is None else int(nbytes)
    if offset < 0 or nbytes < 0 or offset + nbytes > buf.nbytes:
        raise ValueError("the range lies outside the buffer")
    have = min(len(block), nbytes)
    if not have:
        return buf
    first = type(buf).from_host(block[:have])
    try:
        buf.copy_from(first, nbytes=have, dst_offset=offset)
    finally:
        first.free()
    while have < nbytes:   # (`have` stays a whole number of blocks until the last copy: the phase is kept)
        k = min(have, nbytes - have)
        buf.copy_from(buf, nbytes=k, dst_offset=offset + have, src_offset=offset)
        have += k
    return buf


def device_clip(zafx, p, n):
    """The periodic clip of n samples (sample frames) on the device: a DeviceBuffer of p's dtype, (n,) or (n, channels)."""
    p = np.ascontiguousarray(p)
    reps = max(1, BLOCK_BYTES // p.nbytes)
    buf = zafx.DeviceBuffer((int(n),) + p.shape[1:], p.dtype)
    return _replicate(buf, np.concatenate([p] * reps))


def device_ragged(zafx, clips, align=32):
    """A ragged batch on the device: `clips` are host arrays (short clips) or (p, n) -- the periodic clip of n samples --, laid back to back on
    slots of `align` samples (sample frames) in one zero-filled array: -> (buffer, in_offsets, lengths)."""
    first = clips[0] if isinstance(clips[0], np.ndarray) else clips[0][0]
    lengths = [len(c) if isinstance(c, np.ndarray) else int(c[1]) for c in clips]
    offsets, at = [], 0
    for n in lengths:
        offsets.append(at)
        at += -(-n // align) * align
    buf = zafx.DeviceBuffer((max(at, 1),) + first.shape[1:], first.dtype)
    frame = buf.nbytes // buf.shape[0]
    _replicate(buf, np.zeros(BLOCK_BYTES, np.uint8))
    for c, o, n in zip(clips, offsets, lengths):
        block = c if isinstance(c, np.ndarray) else np.concatenate([c[0]] * max(1, BLOCK_BYTES // c[0].nbytes))
        _replicate(buf, np.ascontiguousarray(block, dtype=first.dtype), o * frame, n * frame)
    return buf, np.array(offsets, np.int64), np.array(lengths, np.int64)


def device_filled(zafx, shape, dtype):
    """An output array of `shape` in which every word is the arena's fill."""
    wdtype, value = arena.fill_word(dtype)
    buf = zafx.DeviceBuffer(shape, dtype)
    return _replicate(buf, np.full(BLOCK_BYTES // wdtype.itemsize, value, dtype=wdtype))


def _view(zafx, buf, shape, offset=0):
    """`shape` elements of buf's dtype from element `offset` on: a view, never freed."""
    nbytes = int(np.prod(shape, dtype=np.int64)) * buf.dtype.itemsize
    if offset < 0 or offset * buf.dtype.itemsize + nbytes > buf.nbytes:
        raise ValueError("the view lies outside the buffer")
    return zafx.DeviceBuffer(shape, buf.dtype, _ptr_from_pool=ctypes.c_void_p(buf.ptr.value + offset * buf.dtype.itemsize))


def download_block(zafx, buf, shape, offset=0):
    """The elements of one block of a device array, on the host (short clips only)."""
    view = _view(zafx, buf, shape, offset)
    try:
        return view.download()
    finally:
        view.ptr = ctypes.c_void_p()


def walk_frames(zafx, d_out, rows, pitch, ref, tol, floor, chunk_bytes=32 << 20, part=None, offset=0):
    """FrameChecker over the device array (rows, pitch), downloaded some rows at a time: -> the worst frame's share of its bound.  part = (a, b):
    `ref` speaks about the rows a ... b - 1 of the array only (rows that share a bound); offset: the array starts at that element of d_out."""
    a, b = part or (0, rows)
    view = _view(zafx, d_out, (rows, pitch), offset)
    ck = FrameChecker(ref, tol, floor)
    step = max(1, chunk_bytes // (pitch * d_out.dtype.itemsize))
    try:
        for r0 in range(a, b, step):
            ck.add(r0 - a, view.download(r0, min(step, b - r0)))
    finally:
        view.ptr = ctypes.c_void_p()
    return ck.finish()


def walk_hops(zafx, d_out, count, ref, tol, floor, chunk_bytes=32 << 20, offset=0):
    """HopChecker over `count` values of the device array from element `offset` on, downloaded some hops at a time."""
    view = _view(zafx, d_out, (int(count),), offset)
    ck = HopChecker(ref, tol, floor)
    step = max(1, chunk_bytes // (ck.width * d_out.dtype.itemsize)) * ck.width
    try:
        for i in range(0, max(int(count), 1), step):
            ck.add(i // ck.width, view.download(i, min(step, int(count) - i)))
    finally:
        view.ptr = ctypes.c_void_p()
    return ck.finish()


def assert_untouched(zafx, d_out, chunk_bytes=64 << 20):
    """Every word of the prefilled array is still the fill (after a refused call)."""
    wdtype, value = arena.fill_word(d_out.dtype)
    words = d_out.nbytes // wdtype.itemsize
    view = zafx.DeviceBuffer((words,), wdtype, _ptr_from_pool=ctypes.c_void_p(d_out.ptr.value))
    step = chunk_bytes // wdtype.itemsize
    try:
        for i in range(0, words, step):
            hit = view.download(i, min(step, words - i)) != value
            if hit.any():
                raise LongClipFailure("untouched", None, i + int(np.flatnonzero(hit)[0]), f"{int(hit.sum())} words of a refused call's output changed")
    finally:
        view.ptr = ctypes.c_void_p()
