"""Ragged float64 batches on the GPU (-m gpu): clips of different lengths in ONE launch of the RAGGED forms of the tiled float64 kernels of
W = 2048 (zafx_execute_ragged; zafx.stft_ragged / mdct_ragged / melspectrogram_ragged / mfcc_ragged with f64=True):

    stft, stft_one   k_stft_ft8_f64_ragged    8-frame tiles   complex128
    mdct             k_mdct_ft16_f64_ragged   16-frame tiles  float64
    mel, mfcc        k_mel_ft8_f64_ragged     16-frame tiles  float64   (two rounds of 8 frames)

Hamming 2048 (KBD 2048 for the MDCT), 128 filters at 44.1 kHz, 20 coefficients.  Bounds, normwise per clip (conftest.relerr): the project's
own for these kernels (tests/test_gpu_arena.py TOL_F64 / TOL_F64_MFCC, tests/test_gpu_signals.py) -- 1e-12 for STFT, MDCT and mel, 1e-10
for the MFCC.  One MFCC input is held as tests/test_gpu_signals.py::test_signal_in_float64_mel_mfcc_cqt holds it for the equal-length
kernel: the full-scale tone exactly on a bin.  Its far bands sit at 1e-26 of the peak and hold nothing but the round-off of the
reference's own transform, so any second float64 program moves those coefficients by some 1e-9 (measured on MI355X: 7.05e-9 normwise at
all three lengths, the equal-length k_mel_ft8_f64's 7.1e-9; the ragged launch is bit-equal to it, test 2); it is held to
conftest.mfcc_floor with float64's epsilon (measured: 0.22 - 0.61 of the floor).  Everything else, the MFCCs of silence included (9.1e-14),
holds the normwise bound.  Every figure is printed before it is asserted."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import arena
import signals as sig
import windows as win
from conftest import excess, mfcc_floor, relerr
from oracle import zaf_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_F64 = 1e-12
TOL_F64_MFCC = 1e-10
C_FLOOR = 2.0   # tests/test_gpu_signals.py
W, HOP, FS, N_FILTERS, N_COEFS = 2048, 1024, 44100, 128, 20
KINDS = ("stft", "stft_one", "mdct", "mel", "mfcc")
NATIVE = {"stft": "k_stft_ft8_f64_ragged", "stft_one": "k_stft_ft8_f64_ragged", "mdct": "k_mdct_ft16_f64_ragged", "mel": "k_mel_ft8_f64_ragged",
          "mfcc": "k_mel_ft8_f64_ragged"}
LENGTHS = [0, 1, 1023, 2048, 2049, 44100, 123457]
EDGE_FRAMES = [7, 8, 9, 15, 16, 17]   # both sides of an 8-frame and of a 16-frame tile's edge


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    return z


class Kind:
    """One kind on one window and hop: the plan on whole-line rows, the ragged call, the oracle, the bound and the kernel's name."""

    def __init__(self, zafx, kind, hop=HOP, window=None):
        self.kind, self.hop, self.native = kind, hop, NATIVE[kind]
        self.tol = TOL_F64_MFCC if kind == "mfcc" else TOL_F64
        self.dtype = np.complex128 if kind.startswith("stft") else np.float64
        fb = zafx.melfilterbank(FS, W, N_FILTERS)
        if kind.startswith("stft"):
            one = kind == "stft_one"
            w = zafx.hamming(W) if window is None else window
            self.plan = zafx.stft_plan(w, hop, onesided=one, f64=True, row_align=8)
            self.run = lambda clips: zafx.stft_ragged(clips, w, hop, onesided=one, f64=True)
            self.ref = lambda c: orc.stft(c, w, hop)[: W // 2 + 1 if one else W]
        elif kind == "mdct":
            w = zafx.kaiser_bessel_derived(W) if window is None else window
            self.plan = zafx.mdct_plan(w, row_align=16, f64=True)
            self.run = lambda clips: zafx.mdct_ragged(clips, w, f64=True)
            self.ref = lambda c: orc.mdct(c, w)
        else:
            w = zafx.hamming(W) if window is None else window
            nc = N_COEFS if kind == "mfcc" else None
            self.plan = zafx.mel_plan(w, hop, fb, nc, row_align=16, f64=True)
            if kind == "mfcc":
                self.run = lambda clips: zafx.mfcc_ragged(clips, w, hop, fb, N_COEFS, f64=True)
                self.ref = lambda c: orc.mfcc(c, w, hop, fb, N_COEFS)
            else:
                self.run = lambda clips: zafx.melspectrogram_ragged(clips, w, hop, fb, f64=True)
                self.ref = lambda c: orc.melspectrogram(c, w, hop, fb)
        self.window, self.fb = w, fb

    def frames(self, n):
        return int(self.plan.out_dims(n)[1])

    def length_for(self, t):
        """The smallest clip of `t` frames (plan.out_dims is monotone in the length)."""
        lo, hi = 0, t * max(self.hop, W)
        assert self.frames(hi) >= t
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if self.frames(mid) >= t else (mid + 1, hi)
        assert self.frames(lo) == t, (t, lo, self.frames(lo))
        return lo

    def held(self, got, ref, clip, what):
        """One clip against the oracle: shape, dtype and the normwise bound."""
        assert got.shape == ref.shape and got.dtype == self.dtype, (what, got.shape, ref.shape, got.dtype)
        err = relerr(got, ref)
        print(f"{self.kind} hop {self.hop} {what} n {len(clip)} T {ref.shape[1]} relerr {err:.3e}")
        assert err <= self.tol, (what, len(clip), err)


def noise_clips(lengths, seed):
    return [np.random.default_rng([seed, i]).standard_normal(int(n)) for i, n in enumerate(lengths)]


def family(name):
    return name[: -len("_ragged")] if name.endswith("_ragged") else name


def launch_direct(zafx, plan, flat, in_off, lens, d_out=None, fill=None, slack=0):
    """Plan.execute_ragged on a packed array: -> (whole output array, offs, frames, pitch, the kernel that ran)."""
    lens = np.asarray(lens, np.int64)
    offs, frames, pitch = plan.ragged_layout(lens)
    total = max(int(offs[-1]), 1) + slack
    d_in = zafx.DeviceBuffer.from_host(np.ascontiguousarray(flat, plan.in_dtype), plan.device)
    own = d_out is None
    if own:
        d_out = (zafx.DeviceBuffer.from_host(np.full(total, fill, plan.out_dtype), plan.device) if fill is not None
                 else zafx.DeviceBuffer((total,), plan.out_dtype, plan.device))
    try:
        plan.execute_ragged(d_in, np.asarray(in_off, np.int64), lens, d_out)
        plan.sync()
        return d_out.download(), offs, frames, pitch, plan.last_kernel
    finally:
        d_in.free()
        if own:
            d_out.free()


def views(plan, res, offs, frames, pitch):
    rows = plan.out_dims(0)[0]
    return [res[o: o + rows * p].reshape(rows, p)[:, :t] for o, t, p in zip(offs.tolist(), frames.tolist(), pitch.tolist())]


# ------------------------------------------------------------------ 1: against the oracle, the native route taken
ORACLE_CASES = [("stft", h) for h in (1024, 512, 100, 37)] + [("stft_one", h) for h in (1024, 512, 100, 37)] + [("mdct", HOP), ("mel", HOP), ("mfcc", HOP)]


@pytest.mark.parametrize("kind,hop", ORACLE_CASES)
def test_against_the_oracle_in_one_launch(zafx, kind, hop):
    k = Kind(zafx, kind, hop)
    edge = [k.length_for(t) for t in EDGE_FRAMES]
    assert [k.frames(n) for n in edge] == EDGE_FRAMES
    lengths = LENGTHS + edge
    clips = noise_clips(lengths, 1)
    got = k.run(clips)
    assert k.plan.last_kernel == k.native, k.plan.last_kernel   # (the parent commit: "per-clip ...")
    assert len(got) == len(clips)
    for i, (g, c) in enumerate(zip(got, clips)):
        assert g.shape[1] == k.frames(len(c))
        k.held(g, k.ref(c), c, f"clip {i}")


# ------------------------------------------------------------------ 2: bit-equal to the padded batch on the same plan
@pytest.mark.parametrize("lengths_are", ["even", "any"])
@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_padded_batch_bit_for_bit(zafx, kind, lengths_are):
    k = Kind(zafx, kind)
    lengths = np.random.default_rng([5, lengths_are == "even"]).integers(0, 40000, 48)
    if lengths_are == "even":
        lengths -= lengths % 2
    clips = noise_clips(lengths.tolist(), 6)
    got = k.run(clips)
    assert k.plan.last_kernel == k.native, k.plan.last_kernel
    nmax = max(len(c) for c in clips)
    x = np.zeros((len(clips), nmax))
    for i, c in enumerate(clips):
        x[i, : len(c)] = c
    pad = k.plan.run_host(x, nmax)
    assert k.plan.last_kernel == family(k.native), k.plan.last_kernel   # the same kernel, equal-length form
    for i, g in enumerate(got):
        assert g.shape[1] == k.frames(int(lengths[i]))
        assert np.array_equal(g, pad[i][:, : g.shape[1]]), (i, int(lengths[i]))


# ------------------------------------------------------------------ 3: bit-equal to the per-clip route (the measurement switch)
CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import numpy as np
import zafx
import test_gpu_f64_ragged as t
clips = t.noise_clips({lengths!r}, 30)
out = {{}}
for kind in t.KINDS:
    k = t.Kind(zafx, kind)
    got = k.run(clips)
    out[kind + "_kernel"] = np.array(k.plan.last_kernel)
    for i, g in enumerate(got):
        out[f"{{kind}}_{{i}}"] = g
np.savez({out!r}, **out)
"""


def test_the_measurement_switch_keeps_a_batch_per_clip(zafx, tmp_path):
    """ZAFX_RAGGED_F64_NATIVE=0, set in a fresh child process: one execute per clip, array_equal to the one launch for every kind."""
    lengths = [0, 1, 2049, 9 * HOP + 3, 16 * HOP, 17 * HOP - 1, 30001]
    clips = noise_clips(lengths, 30)
    native = {}
    for kind in KINDS:
        k = Kind(zafx, kind)
        native[kind] = k.run(clips)
        assert k.plan.last_kernel == k.native, k.plan.last_kernel
    out = str(tmp_path / "per_clip.npz")
    script = CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "zaf-python_amd"), tests=os.path.join(ROOT, "tests"), lengths=lengths, out=out)
    env = dict(os.environ, ZAFX_RAGGED_F64_NATIVE="0")
    res = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-1000:]
    child = np.load(out)
    for kind in KINDS:
        assert str(child[kind + "_kernel"]).startswith("per-clip "), (kind, child[kind + "_kernel"])
        for i, g in enumerate(native[kind]):
            assert np.array_equal(child[f"{kind}_{i}"], g), (kind, i, lengths[i])


# ------------------------------------------------------------------ 4: nothing but the clips is written
@pytest.mark.parametrize("kind", ["stft_one", "mdct", "mfcc"])
def test_writes_nothing_but_the_clips(zafx, kind):
    k = Kind(zafx, kind)
    clips = noise_clips([0, 1, 3 * W + 7, 5000, 77, 20000, k.length_for(8), k.length_for(9), k.length_for(17)], 9)
    x, in_off, lens = zafx.pack_ragged(clips, np.float64)
    res, offs, frames, pitch, kernel = launch_direct(zafx, k.plan, x, in_off, lens, fill=np.nan, slack=64)
    assert kernel == k.native, kernel
    rows = k.plan.out_dims(0)[0]
    real = np.zeros(len(res), bool)
    for o, t, p in zip(offs.tolist(), frames.tolist(), pitch.tolist()):
        real[o: o + rows * p].reshape(rows, p)[:, :t] = True
    assert (~real).sum() >= 64 + rows   # (pad columns and the slack are there to be left alone)
    assert np.all(np.isfinite(res[real]))
    assert np.all(np.isnan(res[~real]))


# ------------------------------------------------------------------ 5: order does not matter
@pytest.mark.parametrize("kind", KINDS)
def test_permutation_gives_identical_clips(zafx, kind):
    k = Kind(zafx, kind)
    clips = noise_clips(np.random.default_rng(10).integers(0, 30000, 48).tolist() + [0, 15 * HOP + 1], 11)
    perm = np.random.default_rng(12).permutation(len(clips))
    a = k.run(clips)
    b = k.run([clips[i] for i in perm])
    assert k.plan.last_kernel == k.native
    for j, i in enumerate(perm.tolist()):
        assert np.array_equal(a[i], b[j]), i


# ------------------------------------------------------------------ 6: clips at odd offsets (the scalar loads against the 16-byte loads)
@pytest.mark.parametrize("kind", KINDS)
def test_odd_offsets_equal_even_offsets(zafx, kind):
    k = Kind(zafx, kind)
    lengths = [0, 1, 2049, 9 * HOP + 3, 16 * HOP, 17 * HOP - 1, 12346, 30001]
    clips = noise_clips(lengths, 40)
    results = {}
    for parity in (0, 1):
        in_off, at = [], 0
        for c in clips:
            at += (at + parity) % 2   # every clip starts at an element offset of this parity
            in_off.append(at)
            at += len(c) + 3          # poison between the clips: a read outside a clip shows
        flat = np.full(at + 2, np.nan)
        for o, c in zip(in_off, clips):
            assert o % 2 == parity
            flat[o: o + len(c)] = c
        res, offs, frames, pitch, kernel = launch_direct(zafx, k.plan, flat, in_off, lengths)
        assert kernel == k.native, (parity, kernel)   # d_in itself is on 16 bytes in both
        results[parity] = views(k.plan, res, offs, frames, pitch)
    for i, (e, o) in enumerate(zip(results[0], results[1])):
        assert np.all(np.isfinite(e)), i
        assert np.array_equal(e, o), (i, lengths[i])


# ------------------------------------------------------------------ 7: the routes that stay on one execute per clip
def _per_clip_cases(zafx):
    ham, kbd = zafx.hamming(W), zafx.kaiser_bessel_derived(W)
    ham1k = zafx.hamming(1024)
    return [
        ("magnitude", zafx.stft_plan(ham, HOP, onesided="magnitude", f64=True, row_align=16), 0,
         lambda c: zafx.stft_batch(c[None], ham, HOP, onesided="magnitude", f64=True, row_align=0)[0]),
        ("TF", zafx.stft_plan(ham, HOP, layout="TF", f64=True), 0, lambda c: zafx.stft_batch(c[None], ham, HOP, layout="TF", f64=True)[0]),
        ("W = 1024", zafx.stft_plan(ham1k, 512, f64=True, row_align=8), 0, lambda c: zafx.stft_batch(c[None], ham1k, 512, f64=True, row_align=0)[0]),
        ("compact rows", zafx.stft_plan(ham, HOP, f64=True, row_align=0), 0, lambda c: zafx.stft_batch(c[None], ham, HOP, f64=True, row_align=0)[0]),
        ("d_out + 8 bytes", zafx.mdct_plan(kbd, row_align=16, f64=True), 8, lambda c: zafx.mdct_batch(c[None], kbd, f64=True, row_align=0)[0]),
    ]


@pytest.mark.parametrize("case", range(5))
def test_other_routes_stay_per_clip(zafx, case):
    name, plan, shift, per_clip = _per_clip_cases(zafx)[case]
    clips = noise_clips([1, 3000, 44100, 100003, 25000], 13)
    x, in_off, lens = zafx.pack_ragged(clips, np.float64)
    offs, frames, pitch = plan.ragged_layout(lens)
    rows = plan.out_dims(0)[0]
    n_out = max(int(offs[-1]), 1)
    base = zafx.DeviceBuffer((n_out + 16,), plan.out_dtype, plan.device)
    d_out = zafx.DeviceBuffer((n_out,), plan.out_dtype, _ptr_from_pool=ctypes.c_void_p(base.ptr.value + shift))   # (a view: nothing to free)
    try:
        res, *_, kernel = launch_direct(zafx, plan, x, in_off, lens, d_out=d_out)
    finally:
        d_out.ptr = ctypes.c_void_p()
        base.free()
    assert kernel.startswith("per-clip "), (name, kernel)
    for i, c in enumerate(clips):
        o, t, p = int(offs[i]), int(frames[i]), int(pitch[i])
        got = res[o: o + rows * p].reshape(rows, p)[:, :t] if plan.layout == zafx.LAYOUT_FT else res[o: o + t * rows].reshape(t, rows)
        assert np.array_equal(got, per_clip(c)), (name, i)


# ------------------------------------------------------------------ 8: the staging copy of the table
@pytest.mark.parametrize("kind", ["stft", "mdct"])
def test_back_to_back_calls_each_see_their_own_table(zafx, kind):
    plan = Kind(zafx, kind).plan
    rng = np.random.default_rng(14)
    batches = []
    for b in range(2):
        clips = noise_clips(rng.integers(0, 6000, 600 - 200 * b).tolist(), 15 + b)
        x, in_off, lens = zafx.pack_ragged(clips, np.float64)
        offs, frames, pitch = plan.ragged_layout(lens)
        batches.append((zafx.DeviceBuffer.from_host(x), in_off, lens, int(offs[-1])))
    outs = [zafx.DeviceBuffer((n,), plan.out_dtype) for *_, n in batches]
    expect = []
    for (d_in, in_off, lens, _), d_out in zip(batches, outs):   # one call at a time
        plan.execute_ragged(d_in, in_off, lens, d_out)
        plan.sync()
        assert plan.last_kernel == NATIVE[kind]
        expect.append(d_out.download())
        d_out.upload(np.zeros(d_out.shape, plan.out_dtype))
    for (d_in, in_off, lens, _), d_out in zip(batches, outs):   # both enqueued, no sync between them
        plan.execute_ragged(d_in, in_off, lens, d_out)
    plan.sync()
    for e, d_out in zip(expect, outs):
        assert np.array_equal(d_out.download(), e)
    for (d_in, *_), d_out in zip(batches, outs):
        d_in.free()
        d_out.free()


# ------------------------------------------------------------------ 9: signals and windows
SIGNAL_LENGTHS = (sig.N_FRAMES, sig.N_FRAMES + 1, 5 * sig.HOP + 3)


@pytest.mark.parametrize("kind", KINDS)
def test_signals_as_one_ragged_batch(zafx, kind):
    """The nine tests/signals.py signals at three lengths, 27 clips in one launch."""
    k = Kind(zafx, kind)
    cases = [(name, n) for name in sig.NAMES for n in SIGNAL_LENGTHS]
    clips = [sig.signal(name, n).astype(np.float64) for name, n in cases]
    got = k.run(clips)
    assert k.plan.last_kernel == k.native, k.plan.last_kernel
    for (name, n), c, g in zip(cases, clips, got):
        ref = k.ref(c)
        if name == "silence" and kind != "mfcc":
            assert g.shape == ref.shape and not np.any(ref) and np.array_equal(g, ref), (name, n)   # the oracle's zeros, exactly
        elif name == "sine_bin" and kind == "mfcc":   # (module docstring: the reference's own far bands are round-off)
            half = orc.stft(c, k.window, k.hop)[: W // 2 + 1]
            fl = mfcc_floor(half, k.fb.toarray(), N_COEFS, C_FLOOR, float(np.finfo(float).eps))
            print(f"mfcc {name} n {n} relerr {relerr(g, ref):.3e} error over floor {excess(g, ref, fl):.3f}")
            assert g.shape == ref.shape and excess(g, ref, fl) <= 1.0, (name, n)
        else:
            k.held(g, ref, c, name)


@pytest.mark.parametrize("kind", KINDS)
def test_windows_that_are_not_mirror_symmetric(zafx, kind):
    names = win.MEL_WINDOWS if kind in ("mel", "mfcc") else win.NAMES
    for name in names:
        k = Kind(zafx, kind, window=win.window(name, W))
        clips = noise_clips([1, 2049, 9 * HOP + 3, 17 * HOP - 1, 12346], 50)
        got = k.run(clips)
        assert k.plan.last_kernel == k.native, (name, k.plan.last_kernel)
        for i, (g, c) in enumerate(zip(got, clips)):
            k.held(g, k.ref(c), c, f"window {name} clip {i}")


# ------------------------------------------------------------------ 10: in an arena (tests/arena.py)
ARENA_PAIRS = [(128, 128), (16, 128), (128, 8), (8, 128), (8, 8)]   # (delta_in, delta_out) in bytes


@pytest.mark.parametrize("kind", KINDS)
def test_in_an_arena(zafx, kind):
    """Three lengths in one call, the blocks in an arena of the FILL64 word, then the middle clip poisoned: nothing outside the clips'
    elements is written and the neighbours do not move.  d_out on the line grid and d_in on 16 bytes: the one launch; either off: one
    execute per clip."""
    k = Kind(zafx, kind)
    lengths = np.array([17 * HOP + 5, 3000, 9 * HOP], np.int64)
    x = noise_clips(lengths.tolist(), 77)
    in_offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    flat = np.concatenate(x)
    ref = [k.ref(c) for c in x]
    offs, frames, pitch = k.plan.ragged_layout(lengths)
    rows = ref[0].shape[0]
    blocks = [arena.Block(int(offs[i]), (rows, int(pitch[i])), int(frames[i]), ref[i]) for i in range(3)]
    assert int(offs[3]) == sum(rows * int(p) for p in pitch) and [r.shape[1] for r in ref] == frames.tolist()
    poisoned = flat.copy()
    poisoned[in_offsets[1]: in_offsets[1] + lengths[1]] = np.nan
    launch = lambda d_in, d_out: (k.plan.execute_ragged(d_in, in_offsets, lengths, d_out), k.plan.sync())
    guard = arena.guard_bytes(int(lengths.max()) * 8, max(rows * int(p) for p in pitch) * k.plan.out_dtype.itemsize)
    failures, seen = [], []
    for di, do in ARENA_PAIRS:
        arena.run_case(zafx, flat, k.plan.out_dtype, blocks, guard, (di, do), launch, k.tol, relerr, poisoned=poisoned)
        ran = k.plan.last_kernel
        seen.append(f"({di}, {do}): {ran}")
        native = do % 128 == 0 and di % 16 == 0
        if not (ran == k.native if native else ran.startswith("per-clip ")):
            failures.append(f"({di}, {do}): ran {ran}")
    print("; ".join(seen))
    assert not failures, "\n".join(failures)
