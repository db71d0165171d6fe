"""The mask filter on 16-bit PCM on the GPU (k_maskfilter_pcm, k_maskfilter_stereo_pcm; zafx_execute_masked_pcm, zafx_execute_masked_pcm_ragged).

The contract (include/zafx.h, DESIGN.md 4.12 "PCM"): a sample s enters as s / 32768, so
  1. a float32 output is BIT-IDENTICAL to zafx_execute_masked / zafx_execute_masked_stereo on x.astype(float32) / 32768, rest included;
  2. an int16 output is the NumPy quantiser np.where(isnan(y), 0, clip(rint(y * 32768), -32768, 32767)) of that float32 output, exactly;
  3. independent of the float kernel: |y_q - 32768 ref| <= 0.5 + 32768 TOL_FFT max(max|ref|, max|x / 32768|) against the float64 oracle -- half
     an LSB of the quantiser plus the family's bound;
  4. under a mask of ones y_q == x to the bit on full-range noise (the family's bound is 0.33 LSB at level 1, below the half LSB of a flip);
  5. the rest is integer arithmetic on what was written: rest_q == clip(x - y_q, -32768, 32767), y_q + rest_q == x where that did not saturate;
  6. NaN -> 0, +inf -> 32767, and a non-finite mask value stays inside its frame's output blocks (mono: its partner frame's too) of its clip;
  7. a clip has the same bits alone, in a batch, in a ragged batch, however cut, and on one compute unit;
  8. nothing is read or written outside [0, N) of a block, at bases 2 bytes off the 4-byte grid (mono) and 4 off the 8- and 128-byte grids (stereo);
  9. every refusal leaves the output untouched and the plan usable.
Forms: (n_channels, mask_channels) = (1, 1) mono, (2, 1) stereo under one mask, (2, 2) stereo under a mask per channel."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from maskfilter_oracle import TOL_FFT, make_mask, mask_frames, oracle_maskfilter
from maskfilter_stereo_oracle import make_stereo_masks, oracle_maskfilter_stereo

pytestmark = pytest.mark.gpu

WINDOWS = (256, 512, 1024, 2048)
FORMS = ((1, 1), (2, 1), (2, 2))
KINDS = ("unit", "sparse", "signed_wide")
SENT16 = -12345                # the pre-fill of an int16 output no refused or skipped call may touch
SENT32 = 0xC640E400            # -12345.0 as float32 bits: the same for a float32 output
POISON16 = 0x7A5B              # int16 words around the clips: a neighbour read as a clip's tail would change the clip's result
FILL = 0x7FC5A5A5              # a quiet NaN around the masks


def numpy_quantise(y):
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isnan(y), 0, np.clip(np.rint(y * np.float32(32768)), -32768, 32767)).astype(np.int16)


def int_rest(x, yq):
    return np.clip(x.astype(np.int32) - yq.astype(np.int32), -32768, 32767).astype(np.int16)


def edge_lengths(wl):
    h = wl // 2
    return [1, h - 1, h, h + 1, wl, 3 * h + 7]


def long_lengths(wl):
    """60 H + 5 at the smallest and the largest window: several tiles, so the carry is handed on, and a batch this small is cut into segments."""
    return [60 * (wl // 2) + 5] if wl in (256, 2048) else []


def matrix_lengths(wl):
    return edge_lengths(wl) + long_lengths(wl)


def noise(seed, n, ch, sigma=None):
    """int16 noise, (n,) or (n, 2): full range, or (sigma) Gaussian at that level."""
    g = np.random.default_rng([707, seed, n, ch])
    shape = (n,) + ((2,) if ch == 2 else ())
    if sigma is None:
        return g.integers(-32768, 32768, shape).astype(np.int16)
    return np.clip(np.rint(g.standard_normal(shape) * sigma), -32768, 32767).astype(np.int16)


def masks_of(kind, wl, n, form, seed=0):
    """One clip's masks in the reference's order: (W/2 + 1, T), or (2, W/2 + 1, T) for a mask per channel."""
    return make_mask(kind, wl, n, seed) if form[1] == 1 else make_stereo_masks(kind, wl, n, 2, seed)


def tf(m, batched=True):
    """Masks as the device reads them: (..., T, W/2 + 1) or (..., T, 2, W/2 + 1) float32, compact."""
    m = np.asarray(m, np.float32)
    lead = (0,) if batched else ()
    k = len(lead)
    per_channel = m.ndim - k == 3
    return np.ascontiguousarray(m.transpose(lead + ((k + 2, k, k + 1) if per_channel else (k + 1, k))))


def normalised(x):
    return x.astype(np.float32) / np.float32(32768)


def plan_of(wl, rest=False, layout="TF"):
    import zafx
    return zafx.maskfilter_plan(zafx.hamming(wl), rest=rest, layout=layout)


def out_shape(plan, b, n, ch):
    return plan.stereo_out_shape(b, n) if ch == 2 else plan.out_shape(b, n)


def run_float(xf, m, wl, form, rest=False):
    """The float entry point of the form on float32 clips: the plan's whole output array."""
    import zafx
    plan = plan_of(wl, rest)
    b, n = xf.shape[:2]
    d_in, d_mask = zafx.DeviceBuffer.from_host(np.ascontiguousarray(xf, np.float32)), zafx.DeviceBuffer.from_host(tf(m))
    d_out = zafx.DeviceBuffer(out_shape(plan, b, n, form[0]), np.float32)
    try:
        if form[0] == 1:
            plan.execute_masked(d_in, d_mask, d_out, b, n)
        else:
            plan.execute_masked_stereo(d_in, d_mask, d_out, b, n, form[1])
        plan.sync()
        assert plan.last_kernel == ("k_maskfilter" if form[0] == 1 else "k_maskfilter_stereo")
        return d_out.download()
    finally:
        for buf in (d_in, d_mask, d_out):
            buf.free()


def run_pcm(x, m, wl, form, rest=False, out=np.int16):
    """zafx_execute_masked_pcm on int16 clips (B, N[, 2]): the plan's whole output array, of dtype `out`."""
    import zafx
    plan = plan_of(wl, rest)
    b, n = x.shape[:2]
    assert x.dtype == np.int16 and x.ndim == 1 + form[0]
    d_in, d_mask = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(tf(m))
    d_out = zafx.DeviceBuffer(out_shape(plan, b, n, form[0]), out)
    try:
        plan.execute_masked_pcm(d_in, d_mask, d_out, b, n, form[0], form[1])
        plan.sync()
        assert plan.last_kernel == ("k_maskfilter_pcm" if form[0] == 1 else "k_maskfilter_stereo_pcm") and plan.kernel_name == "k_maskfilter"
        return d_out.download()
    finally:
        for buf in (d_in, d_mask, d_out):
            buf.free()


def run_pcm_ragged(clips, masks, wl, form, rest=False, out=np.int16):
    """maskfilter_pcm_ragged: a list of per-clip arrays (blocks, N_i[, 2]), blocks = 2 with rest."""
    import zafx
    res = zafx.maskfilter_pcm_ragged(clips, zafx.hamming(wl), masks, rest=rest, out_dtype=out)
    if any(len(c) for c in clips):
        assert plan_of(wl, rest).last_kernel == ("k_maskfilter_pcm_ragged" if form[0] == 1 else "k_maskfilter_stereo_pcm_ragged")
    return [np.stack(r) if rest else r[None] for r in res]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


# The matrix of 1 and 2, computed once: per (W, form, rest, N) three clips -- one per mask kind -- of full-range noise, the float kernel's
# output on the normalised clips, and the PCM kernels' float32 and int16 outputs.
_MATRIX = {}


def matrix(wl, form, rest, n):
    key = (wl, form, rest, n)
    if key not in _MATRIX:
        x = np.stack([noise(k, n, form[0]) for k in range(len(KINDS))])
        m = np.stack([masks_of(kind, wl, n, form, seed=k) for k, kind in enumerate(KINDS)])
        _MATRIX[key] = x, m, run_float(normalised(x), m, wl, form, rest), run_pcm(x, m, wl, form, rest, np.float32), run_pcm(x, m, wl, form, rest, np.int16)
    return _MATRIX[key]


# ------------------------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wl", WINDOWS)
def test_float_out_has_the_bits_of_the_float_kernel(wl, form, rest):
    """The edge lengths -- one tile, no carry -- and, at W = 256 and 2048, 60 H + 5: the PCM instantiations against the float ones across tile
    boundaries, a handed-on carry and segment cuts, equal-length and inside the ragged batch beside the edge lengths."""
    for n in matrix_lengths(wl):
        x, m, yf, pf, pq = matrix(wl, form, rest, n)
        assert pf.dtype == np.float32 and same(pf, yf), (wl, form, rest, n)
    # ragged: every edge length in one launch, per mask kind, against the equal-length call
    for k in range(len(KINDS)):
        clips = [matrix(wl, form, rest, n)[0][k] for n in matrix_lengths(wl)]
        masks = [matrix(wl, form, rest, n)[1][k] for n in matrix_lengths(wl)]
        for n, r in zip(matrix_lengths(wl), run_pcm_ragged(clips, masks, wl, form, rest, np.float32)):
            assert same(r.reshape(matrix(wl, form, rest, n)[2][k].shape), matrix(wl, form, rest, n)[2][k]), (wl, form, rest, n, KINDS[k])


@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wl", WINDOWS)
def test_int16_out_is_the_quantised_float_output(wl, form, rest):
    for n in matrix_lengths(wl):
        x, m, yf, pf, pq = matrix(wl, form, rest, n)
        assert pq.dtype == np.int16
        y = yf[:, 0] if rest else yf
        yq = pq[:, 0] if rest else pq
        assert np.array_equal(yq, numpy_quantise(y)), (wl, form, rest, n)
        if rest:
            assert np.array_equal(pq[:, 1], int_rest(x, yq)), (wl, form, n)
    for k in range(len(KINDS)):
        clips = [matrix(wl, form, rest, n)[0][k] for n in matrix_lengths(wl)]
        masks = [matrix(wl, form, rest, n)[1][k] for n in matrix_lengths(wl)]
        for n, r in zip(matrix_lengths(wl), run_pcm_ragged(clips, masks, wl, form, rest, np.int16)):
            assert same(r.reshape(matrix(wl, form, rest, n)[4][k].shape), matrix(wl, form, rest, n)[4][k]), (wl, form, rest, n, KINDS[k])


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wl", WINDOWS)
def test_int16_out_against_the_float64_oracle(wl, form):
    """Gaussian noise at sigma = 3000 (peaks near 13000) under masks in [0, 1] and in [-2, 2]: the reference stays inside the int16 range --
    asserted --, so the bound is the quantiser's half LSB plus the family's and no saturation enters it."""
    import zafx
    w = zafx.hamming(wl)
    worst = 0.0
    for n in edge_lengths(wl):
        x = np.stack([noise(10 + k, n, form[0], sigma=3000) for k in range(len(KINDS))])
        m = np.stack([masks_of(kind, wl, n, form, seed=10 + k) for k, kind in enumerate(KINDS)])
        yq = run_pcm(x, m, wl, form)
        for k, kind in enumerate(KINDS):
            xn = x[k].astype(np.float64) / 32768
            ref = oracle_maskfilter(xn, w, m[k]) if form[0] == 1 else oracle_maskfilter_stereo(xn, w, m[k])
            bound = 0.5 + 32768 * TOL_FFT * max(np.abs(ref).max(), np.abs(xn).max())
            assert np.abs(32768 * ref).max() + bound < 32767, (wl, form, n, kind)
            err = np.abs(yq[k].astype(np.float64) - 32768 * ref).max()
            worst = max(worst, err / bound)
            assert err <= bound, (wl, form, n, kind, err, bound)
    print(f"W={wl} form={form}: worst error {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wl", WINDOWS)
def test_a_mask_of_ones_is_lossless(wl, form):
    for n in edge_lengths(wl) + [60 * (wl // 2) + 5]:
        x = np.stack([noise(20 + k, n, form[0]) for k in range(2)])
        x[0, 0], x[1, -1] = 32767, -32768
        t = mask_frames(n, wl)
        m = np.ones((2,) + ((2,) if form[1] == 2 else ()) + (wl // 2 + 1, t), np.float32)
        out = run_pcm(x, m, wl, form, rest=True)
        assert np.array_equal(out[:, 0], x) and not out[:, 1].any(), (wl, form, n)


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wl", WINDOWS)
def test_rest_is_integer_arithmetic_on_what_was_written(wl, form):
    """Full-range noise under constant masks: 2.0 filters to 2 x, so y saturates; -1.0 to -x, so rest = x - y = 2 x saturates.  The float64
    reference itself saturates in at least 100 samples of y (of rest) and stays inside in at least 100: checked here, on the CPU."""
    import zafx
    w, h = zafx.hamming(wl), wl // 2
    n = 3 * h + 7
    t = mask_frames(n, wl)
    x = np.stack([noise(30 + k, n, form[0]) for k in range(2)])
    for value, what in ((2.0, "y"), (-1.0, "rest")):
        m = np.full((2,) + ((2,) if form[1] == 2 else ()) + (h + 1, t), value, np.float32)
        xn = x[0].astype(np.float64) / 32768
        ref = 32768 * (oracle_maskfilter(xn, w, m[0]) if form[0] == 1 else oracle_maskfilter_stereo(xn, w, m[0]))
        assert np.abs(ref - value * x[0]).max() < 1e-6 * 32768   # a constant mask m filters to m x
        quantity = ref if what == "y" else x[0] - np.clip(np.rint(ref), -32768, 32767)
        outside = (quantity > 32767 + 1) | (quantity < -32768 - 1)
        assert outside.sum() >= 100 and (~outside).sum() >= 100, (wl, form, value, int(outside.sum()))
        out = run_pcm(x, m, wl, form, rest=True)
        yq, rq = out[:, 0], out[:, 1]
        assert np.array_equal(rq, int_rest(x, yq)), (wl, form, value)
        diff = x.astype(np.int32) - yq
        inside = (diff >= -32768) & (diff <= 32767)
        assert np.array_equal((yq.astype(np.int32) + rq)[inside], x.astype(np.int32)[inside])
        got = yq[0] if what == "y" else rq[0]
        assert np.array_equal(got[outside], np.where(quantity[outside] > 0, 32767, -32768)), (wl, form, value)
        assert (np.abs(got[~outside].astype(np.int32)) < 32767).sum() >= 100
        assert np.array_equal(yq, numpy_quantise(run_float(normalised(x), m, wl, form)))


# ------------------------------------------------------------------------------------------------------------------ 6
def blocks_mask(n, h, blocks):
    hit = np.zeros(n, bool)
    for b in blocks:
        if b >= 0:
            hit[min(b * h, n):min((b + 1) * h, n)] = True
    return hit


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wl", [256, 2048])
def test_non_finite_mask_values(wl, form, ragged):
    """A NaN and a +inf in mask frame 13 of the middle clip of three.  The int16 output is the quantiser of the float kernel's output on the
    same masks (NaN -> 0, +-inf -> the ends); only output blocks 12 and 13 of that clip -- for mono also those of the partner frame 12, which
    rides in the same transform: block 11 -- may differ from the clean run; the other clips keep their bits."""
    h = wl // 2
    n = 20 * h + 9
    frame = 13
    x = np.stack([noise(40 + k, n, form[0], sigma=3000) for k in range(3)])
    m = np.stack([masks_of("unit", wl, n, form, seed=40 + k) for k in range(3)])

    def run(ms, out):
        if ragged:
            return np.concatenate(run_pcm_ragged(list(x), list(ms), wl, form, out=out))
        return run_pcm(x, ms, wl, form, out=out)
    clean = run(m, np.int16)
    mp = m.copy()
    mp[(1, h // 3, frame) if form[1] == 1 else (1, 0, h // 3, frame)] = np.nan
    mp[(1, h // 5, frame) if form[1] == 1 else (1, 1, h // 5, frame)] = np.inf
    got = run(mp, np.int16)
    yf = run_float(normalised(x), mp, wl, form)
    assert not np.isfinite(yf[1]).all() and np.array_equal(got, numpy_quantise(yf)), (wl, form, ragged)
    for c in (0, 2):
        assert np.array_equal(got[c], clean[c]), (wl, form, c)
    may = blocks_mask(n, h, [frame - 1, frame] + ([frame - 2] if form[0] == 1 else []))
    assert np.array_equal(got[1][~may], clean[1][~may]) and not np.array_equal(got[1][may], clean[1][may]) and 0 < may.sum() < n
    bad = ~np.isfinite(yf[1])
    assert bad.any() and set(np.unique(got[1][bad]).tolist()) <= {0, 32767, -32768}


# ------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wl", WINDOWS)
def test_a_clip_has_the_same_bits_anywhere(monkeypatch, wl, form):
    """The clip of 60 blocks + 5 sample frames alone -- a batch too small for the device, so it is cut into segments --, in batches of 2, 3
    and 5 (other segment lengths), and in a ragged batch cut for 1, the preset number and 64 units per workgroup slot."""
    import zafx
    from maskfilter_pcm_probe import probe_case, ragged_of
    x, m = probe_case(wl, form)
    alone = run_pcm(x[2:3], m[2:3], wl, form)[0]
    assert np.array_equal(alone, numpy_quantise(run_float(normalised(x[2:3]), m[2:3], wl, form))[0])
    for order in ([2, 0], [1, 2, 0], [0, 1, 2, 3, 1]):
        assert np.array_equal(run_pcm(x[order], m[order], wl, form)[order.index(2)], alone), (wl, form, order)
    clips, masks = ragged_of(x, m, wl)
    env = "ZAFX_MASKFILTER_UNITS_PER_SLOT" if form[0] == 1 else "ZAFX_CENTER_UNITS_PER_SLOT"
    for per_slot in (None, "1", "64"):
        if per_slot:
            monkeypatch.setenv(env, per_slot)
        else:
            monkeypatch.delenv(env, raising=False)
        ys = zafx.maskfilter_pcm_ragged(clips, zafx.hamming(wl), masks)
        assert np.array_equal(ys[1], alone), (wl, form, "ragged", per_slot)


@pytest.mark.timeout(300)
def test_one_compute_unit_gives_the_same_bits(tmp_path):
    """The same clips in a fresh child process under ZAFX_COMPUTE_UNITS=1: every unit on the workgroups of one compute unit."""
    from maskfilter_pcm_probe import FORMS as PROBE_FORMS, WINDOWS as PROBE_WINDOWS, probe_case
    path = str(tmp_path / "probe.npz")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maskfilter_pcm_probe.py"), path], env=dict(os.environ, ZAFX_COMPUTE_UNITS="1"),
                         capture_output=True, timeout=240)
    assert res.returncode == 0 and b"probe ok" in res.stdout, res.stderr.decode()[-2000:]
    got = np.load(path)
    for wl in PROBE_WINDOWS:
        assert int(got[f"units{wl}"]) == 1 and plan_of(wl).compute_units > 1
        for form in PROBE_FORMS:
            x, m = probe_case(wl, form)
            here = run_pcm(x[2:3], m[2:3], wl, form)[0]
            for name in ("alone", "batch", "ragged"):
                assert same(got[f"{name}{wl}_{form[0]}{form[1]}"], here), (wl, form, name)


# ------------------------------------------------------------------------------------------------------------------ 8
class View:
    """`count` elements of `dtype` at byte `offset` of a DeviceBuffer (nothing to free)."""

    def __init__(self, buf, offset, count, dtype):
        self.dtype = np.dtype(dtype)
        self.ptr, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + offset), self.dtype.itemsize * count, (count,)


def arena(data, nbytes, base, fill, guard=4096):
    """A host array of bytes: `guard` + `base` bytes of `fill` words (uint16 or uint32 patterns), the `nbytes` of `data` (None: fill), a guard
    behind -> (bytes, the offset of the data)."""
    word = np.dtype(np.uint16 if fill <= 0xFFFF else np.uint32)
    total = guard + base + nbytes + guard
    total += -total % 4
    host = np.full(total // word.itemsize, fill, word).view(np.uint8).copy()
    if data is not None:
        host[guard + base:guard + base + nbytes] = np.ascontiguousarray(data).view(np.uint8).ravel()
    return host, guard + base


def place(sizes, gap):
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at += s + gap
    return np.array(offs, np.int64), at + 1


def ragged_lengths(wl):
    h = wl // 2
    return [0, 1, h, 3 * h + 7, 60 * h + 5, 20 * h]


_ALONE = {}


def alone_of(x, m, wl, form, rest, out, key):
    key = (wl, form, rest, np.dtype(out).str) + tuple(key)
    if key not in _ALONE:
        _ALONE[key] = run_pcm(x[None], m[None], wl, form, rest, out)[0].reshape((2 if rest else 1,) + x.shape)
    return _ALONE[key]


def run_ragged_arena(plan, clips, masks, form, out, gap, bases):
    """One zafx_execute_masked_pcm_ragged with sample frames, masks and output blocks inside poisoned arenas, `gap` elements between
    neighbours, the three arrays `bases` bytes into their allocations -> the per-clip results, after checking every other output byte."""
    import zafx
    ch = form[0]
    blocks = 2 if plan.kind == zafx.MASKFILTER_REST else 1
    lengths = np.array([len(c) for c in clips], np.int64)
    flat = [tf(m, batched=False).ravel() for m in masks]
    in_offs, in_frames = place(lengths.tolist(), gap)
    mask_offs, mask_words = place([len(f) for f in flat], gap)
    out_offs, out_frames = place((blocks * lengths).tolist(), gap)
    ob = np.dtype(out).itemsize * ch   # bytes of an output sample frame
    h_in, at_in = arena(None, 2 * ch * in_frames, bases[0], POISON16)
    for c, o in zip(clips, in_offs.tolist()):
        h_in[at_in + 2 * ch * o:at_in + 2 * ch * (o + len(c))] = np.ascontiguousarray(c).view(np.uint8).ravel()
    h_mask, at_mask = arena(None, 4 * mask_words, bases[1], FILL)
    for f, o in zip(flat, mask_offs.tolist()):
        h_mask[at_mask + 4 * o:at_mask + 4 * (o + len(f))] = f.view(np.uint8)
    sentinel = SENT16 & 0xFFFF if out == np.int16 else SENT32
    h_out, at_out = arena(None, ob * out_frames, bases[2], sentinel)
    bufs = [zafx.DeviceBuffer.from_host(a) for a in (h_in, h_mask, h_out)]
    views = [View(bufs[0], at_in, ch * in_frames, np.int16), View(bufs[1], at_mask, mask_words, np.float32), View(bufs[2], at_out, ch * out_frames, out)]
    try:
        plan.execute_masked_pcm_ragged(views[0], in_offs, lengths, views[1], mask_offs, views[2], out_offs, ch, form[1])
        plan.sync()
        if lengths.any():
            assert plan.last_kernel == ("k_maskfilter_pcm_ragged" if ch == 1 else "k_maskfilter_stereo_pcm_ragged")
        got = bufs[2].download()
    finally:
        for b in bufs:
            b.free()
    kept = np.ones(len(got), bool)
    res = []
    for o, n in zip(out_offs.tolist(), lengths.tolist()):
        lo = at_out + ob * o
        kept[lo:lo + ob * blocks * n] = False
        res.append(got[lo:lo + ob * blocks * n].view(out).reshape((blocks, n) + ((2,) if ch == 2 else ())))
    assert np.array_equal(got[kept], h_out[kept]), "written outside the clips' blocks"
    return res


@pytest.mark.parametrize("out", [np.int16, np.float32])
@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wl", [2048, 256])
def test_ragged_arena(wl, form, rest, out):
    """Clips, masks and output blocks back to back and with gaps inside poisoned arenas -- int16 words around the clips, NaN around the masks,
    sentinels in the output --: mono int16 arrays 2 bytes off the 4-byte grid, stereo ones 4 bytes off the 8-byte and off the 128-byte grid.
    Nothing outside the blocks is written, nothing at or beyond N, and no clip sees its neighbour: every block has the bits of its clip alone.
    A clip of length 0 is among them."""
    lengths = ragged_lengths(wl)
    clips = [noise(50 + i, n, form[0]) for i, n in enumerate(lengths)]
    masks = [masks_of("unit", wl, n, form, seed=50 + i) for i, n in enumerate(lengths)]
    plan = plan_of(wl, rest)
    # (in, mask, out): the int16 arrays on their own grid only; a float32 output on 4 bytes
    grids = ((0, (2, 4, 2 if out == np.int16 else 4)), (37, (6, 12, 10 if out == np.int16 else 12))) if form[0] == 1 else ((0, (4, 4, 4)), (37, (132, 12, 260)))
    for gap, bases in grids:
        if form[0] == 1:
            assert bases[0] % 4 == 2 and (out != np.int16 or bases[2] % 4 == 2)
        else:
            assert bases[0] % 8 == 4 and bases[2] % 8 == 4 and (gap == 0 or (bases[0] % 128 == 4 and bases[2] % 128 == 4))
        res = run_ragged_arena(plan, clips, masks, form, out, gap, bases)
        for i, (r, x, m) in enumerate(zip(res, clips, masks)):
            if not len(x):
                assert r.size == 0
                continue
            assert same(r, alone_of(x, m, wl, form, rest, out, (i,))), (wl, form, rest, gap, i, len(x))


@pytest.mark.parametrize("out", [np.int16, np.float32])
@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_arena_equal_length(form, rest, out):
    """zafx_execute_masked_pcm on slices of larger buffers, the int16 arrays off the wider grids; nothing but the output is written."""
    import zafx
    ch = form[0]
    for wl, n, deltas in ((2048, 9 * 1024 + 1, (2, 132, 6) if ch == 1 else (4, 132, 20)), (256, 16 * 128 - 1, (130, 4, 66) if ch == 1 else (132, 4, 68))):
        if out == np.float32:
            deltas = deltas[:2] + (deltas[2] + (-deltas[2]) % 4 + 4,)
        plan = plan_of(wl, rest)
        x = np.stack([noise(60 + k, n, ch) for k in range(3)])
        m = np.stack([masks_of("unit", wl, n, form, seed=60 + k) for k in range(3)])
        laid = tf(m)
        shape = out_shape(plan, 3, n, ch)
        n_out = int(np.prod(shape))
        h_in, at_in = arena(x, x.nbytes, deltas[0], POISON16)
        h_mask, at_mask = arena(laid, laid.nbytes, deltas[1], FILL)
        h_out, at_out = arena(None, n_out * np.dtype(out).itemsize, deltas[2], SENT16 & 0xFFFF if out == np.int16 else SENT32)
        bufs = [zafx.DeviceBuffer.from_host(a) for a in (h_in, h_mask, h_out)]
        try:
            plan.execute_masked_pcm(View(bufs[0], at_in, x.size, np.int16), View(bufs[1], at_mask, laid.size, np.float32), View(bufs[2], at_out, n_out, out), 3, n, ch, form[1])
            plan.sync()
            got = bufs[2].download()
        finally:
            for b in bufs:
                b.free()
        hi = at_out + n_out * np.dtype(out).itemsize
        assert np.array_equal(got[:at_out], h_out[:at_out]) and np.array_equal(got[hi:], h_out[hi:]), "written outside the output"
        assert same(got[at_out:hi].view(out).reshape(shape), run_pcm(x, m, wl, form, rest, out)), (wl, form, rest)


def test_empty_batches_and_zero_length_clips_write_nothing():
    import zafx
    for form in FORMS:
        plan = plan_of(512, True)
        assert run_ragged_arena(plan, [], [], form, np.int16, 0, (4, 4, 4)) == []
        clips = [noise(0, 0, form[0])] * 3
        masks = [masks_of("unit", 512, 0, form)] * 3
        assert all(r.size == 0 for r in run_ragged_arena(plan, clips, masks, form, np.int16, 5, (4, 4, 4)))
        # the equal-length call: no clips, and clips of no samples
        sent = np.full(64, SENT16, np.int16)
        d_out, d_in, d_mask = zafx.DeviceBuffer.from_host(sent), zafx.DeviceBuffer.from_host(np.zeros(64, np.int16)), zafx.DeviceBuffer.from_host(np.ones(4 * 257, np.float32))
        lib = zafx._lib.load()
        assert lib.zafx_execute_masked_pcm(plan.handle, d_in.ptr, d_mask.ptr, d_out.ptr, 0, 1000, form[0], form[1], 2) == 0
        assert lib.zafx_execute_masked_pcm(plan.handle, d_in.ptr, d_mask.ptr, d_out.ptr, 2, 0, form[0], form[1], 2) == 0
        plan.sync()
        assert np.array_equal(d_out.download(), sent)
        for b in (d_in, d_mask, d_out):
            b.free()
        assert zafx.maskfilter_pcm_batch(np.zeros((2, 0) + ((2,) if form[0] == 2 else ()), np.int16), zafx.hamming(512),
                                         np.ones((2,) + ((2,) if form[1] == 2 else ()) + (257, 1), np.float32)).shape[:2] == (2, 0)


# ------------------------------------------------------------------------------------------------------------------ the Python functions
@pytest.mark.parametrize("form", FORMS)
def test_the_python_functions_agree_with_the_plan(form):
    import zafx
    wl, n = 1024, 3 * 512 + 7
    w = zafx.hamming(wl)
    x = np.stack([noise(70 + k, n, form[0], sigma=6000) for k in range(3)])
    m = np.stack([masks_of("unit", wl, n, form, seed=70 + k) for k in range(3)])
    for out in (np.int16, np.float32):
        want = run_pcm(x, m, wl, form, True, out)
        y, r = zafx.maskfilter_pcm_batch(x, w, m, rest=True, out_dtype=out)
        assert y.dtype == out and same(y, want[:, 0]) and same(r, want[:, 1]) and y.base is r.base
        yt = zafx.maskfilter_pcm_batch(x, w, tf(m), layout="TF", out_dtype=out)
        assert same(yt, want[:, 0])
        given = np.empty(want.shape, out)
        zafx.maskfilter_pcm_batch(x, w, m, step_length=wl // 2, rest=True, out=given)
        assert same(given, want)
        one = zafx.maskfilter_pcm(x[1], w, wl // 2, m[1], out_dtype=out)
        assert one.dtype == out and same(one, want[1, 0])
        pairs = zafx.maskfilter_pcm_ragged(list(x), w, list(m), rest=True, out_dtype=out)
        assert all(same(p[0], want[i, 0]) and same(p[1], want[i, 1]) for i, p in enumerate(pairs))
    assert zafx.maskfilter_pcm(x[1], w, wl // 2, m[1]).dtype == np.int16


# ------------------------------------------------------------------------------------------------------------------ 9
def test_refusals_leave_the_output_untouched():
    import zafx
    from zafx import _lib
    lib = _lib.load()
    wl, h = 512, 256
    w = zafx.hamming(wl)
    lengths = np.array([3000, 0, 700], np.int64)
    clips = [noise(80 + i, n, 2) for i, n in enumerate(lengths.tolist())]
    masks = [masks_of("unit", wl, n, (2, 2), seed=80 + i) for i, n in enumerate(lengths.tolist())]
    plan, ft_plan, stft = plan_of(wl, True), plan_of(wl, True, layout="FT"), zafx.stft_plan(w, h)
    x = np.concatenate(clips)
    in_offs = np.array([0, 3000, 3000], np.int64)
    mask_offs, _ = plan.stereo_ragged_layout(lengths, 2)
    mask_offs = np.ascontiguousarray(mask_offs[:-1])
    out_offs = 2 * in_offs
    sentinel = np.full((2 * len(x) + 4, 2), SENT16, np.int16)
    d_in, d_out = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(sentinel)
    packed, offs, _ = zafx.pack_ragged_stereo_masks(masks, lengths, wl)
    d_mask = zafx.DeviceBuffer.from_host(packed)
    p64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731
    off = lambda buf, b: ctypes.c_void_p(buf.ptr.value + b)            # noqa: E731

    def ragged(pl, a_in=d_in.ptr, a_inoff=in_offs, a_len=lengths, a_mask=d_mask.ptr, a_moff=mask_offs, a_out=d_out.ptr, a_ooff=out_offs, n=3, ch=2, mc=2, ob=2):
        rc = lib.zafx_execute_masked_pcm_ragged(pl, a_in, None if a_inoff is None else p64(a_inoff), None if a_len is None else p64(a_len), a_mask,
                                                None if a_moff is None else p64(a_moff), a_out, None if a_ooff is None else p64(a_ooff), n, ch, mc, ob)
        return rc, (lib.zafx_last_error() or b"").decode()

    def equal(pl, a_in=d_in.ptr, a_mask=d_mask.ptr, a_out=d_out.ptr, b=1, n=3000, ch=2, mc=2, ob=2):
        return lib.zafx_execute_masked_pcm(pl, a_in, a_mask, a_out, b, n, ch, mc, ob), (lib.zafx_last_error() or b"").decode()

    def neg(a, i):
        b = a.copy()
        b[i] = -1
        return b

    big1, big2 = lengths.copy(), lengths.copy()
    big1[2], big2[2] = 1 << 28, 1 << 27
    both = [
        (dict(pl=None), "null plan"),
        (dict(a_in=None), "null device pointer"), (dict(a_mask=None), "null device pointer"), (dict(a_out=None), "null device pointer"),
        (dict(ch=0), "n_channels"), (dict(ch=3), "n_channels"), (dict(ch=3, n=0), "n_channels"),
        (dict(ch=1, mc=2), "mask_channels must be 1 with one channel"), (dict(mc=0), "mask_channels"), (dict(mc=3), "mask_channels"), (dict(mc=3, n=0), "mask_channels"),
        (dict(ob=0), "out_sample_bytes"), (dict(ob=3), "out_sample_bytes"), (dict(ob=8), "out_sample_bytes"), (dict(ob=1, n=0), "out_sample_bytes"),
        (dict(a_in=off(d_in, 2)), "d_pcm must be 4-byte aligned"), (dict(a_in=off(d_in, 1), ch=1, mc=1), "d_pcm must be 2-byte aligned"),
        (dict(a_out=off(d_out, 2)), "d_out must be 4-byte aligned (stereo int16"), (dict(a_out=off(d_out, 1), ch=1, mc=1), "d_out must be 2-byte aligned"),
        (dict(a_out=off(d_out, 2), ob=4), "d_out must be 4-byte aligned (float32)"), (dict(a_out=off(d_out, 2), ob=4, ch=1, mc=1), "d_out must be 4-byte aligned (float32)"),
        (dict(a_mask=off(d_mask, 2)), "d_mask must be 4-byte aligned"),
        (dict(pl=ft_plan.handle), "ZAFX_LAYOUT_TF"), (dict(pl=ft_plan.handle, n=0), "ZAFX_LAYOUT_TF"), (dict(pl=ft_plan.handle, ch=1, mc=1), "ZAFX_LAYOUT_TF"),
        (dict(pl=stft.handle), "ZAFX_MASKFILTER"), (dict(pl=stft.handle, ch=1, mc=1, ob=4), "ZAFX_MASKFILTER"),
    ]
    only_ragged = [
        (dict(a_inoff=None), "null argument"), (dict(a_len=None), "null argument"), (dict(a_moff=None), "null argument"), (dict(a_ooff=None), "null argument"),
        (dict(n=-1), "negative number of clips"),
        (dict(a_len=neg(lengths, 1)), "of clip 1"), (dict(a_inoff=neg(in_offs, 2)), "of clip 2"), (dict(a_moff=neg(mask_offs, 0)), "of clip 0"), (dict(a_ooff=neg(out_offs, 2)), "of clip 2"),
        (dict(a_len=big2), "2^27 sample frames or more (not supported): clip 2"), (dict(a_len=big1, mc=1), "2^28 sample frames or more (not supported): clip 2"),
        (dict(a_len=big1, ch=1, mc=1), "2^28 samples or more (not supported): clip 2"),
    ]
    only_equal = [(dict(b=-1), "negative size"), (dict(n=-1), "negative size"), (dict(n=1 << 27), "2^27"), (dict(n=1 << 27, b=0), "2^27"), (dict(n=1 << 28, mc=1), "2^28"),
                  (dict(n=1 << 28, ch=1, mc=1), "2^28")]
    for call, cases in ((ragged, both + only_ragged), (equal, [(k, t) for k, t in both if "n" not in k or k["n"] != 0] + only_equal)):
        for kw, text in cases:
            kw = dict(kw)
            kw.setdefault("pl", plan.handle)
            rc, msg = call(**kw)
            assert rc != 0 and text in msg, (call.__name__, list(kw), rc, msg)
            if "of clip" in text:
                assert "negative" in msg
    # a window that is not set, and one whose COLA sum is zero
    bare = zafx.Plan(zafx.MASKFILTER_REST, window_length=wl, step_length=h, layout="TF")
    for call in (ragged, equal):
        rc, msg = call(bare.handle)
        assert rc != 0 and "window constant not set" in msg, msg
    wz = np.array(w, np.float64)
    wz[h] = -wz[0]
    bare.set_window(wz)
    for call in (ragged, equal):
        rc, msg = call(bare.handle)
        assert rc != 0 and "is zero" in msg, msg
    bare.destroy()
    # the entry points for PCM of the forward kinds go on refusing mask-filter plans
    assert lib.zafx_execute_pcm(plan.handle, d_in.ptr, d_out.ptr, 1, 3000, 2, 2) != 0 and b"zafx_execute_masked" in lib.zafx_last_error()
    assert lib.zafx_execute_ragged_pcm(plan.handle, d_in.ptr, p64(in_offs), p64(lengths), d_out.ptr, 3, 2, 2) != 0 and b"zafx_execute_masked" in lib.zafx_last_error()
    # through the Python layer: the library's refusals arrive, wrong dtypes and sizes are caught in front of it
    first = mask_frames(3000, wl) * 2 * (h + 1)
    one_mask = View(d_mask, 0, first, np.float32)
    with pytest.raises(zafx.ZafxError, match="ZAFX_LAYOUT_TF"):
        ft_plan.execute_masked_pcm(d_in, one_mask, d_out, 1, 3000, 2, 2)
    with pytest.raises(zafx.ZafxError, match="MASKFILTER"):
        stft.execute_masked_pcm(d_in, one_mask, d_out, 1, 3000, 2, 2)
    with pytest.raises(zafx.ZafxError, match="mask_channels"):
        plan.execute_masked_pcm(d_in, one_mask, d_out, 1, 3000, 2, 3)
    with pytest.raises(zafx.ZafxError, match="n_channels"):
        plan.execute_masked_pcm(d_in, one_mask, d_out, 1, 3000, 4, 1)
    with pytest.raises(ValueError, match="int16"):
        plan.execute_masked_pcm(View(d_in, 0, 100, np.float32), one_mask, d_out, 1, 3000, 2, 2)
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_pcm(d_in, d_mask, d_out, 1, 3000, 2, 2)       # the masks of three clips for one
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_pcm(d_in, one_mask, d_out, 1, 3000, 2, 1)     # two masks where one is asked for
    with pytest.raises(ValueError, match="d_pcm"):
        plan.execute_masked_pcm(View(d_in, 0, 2 * 3000 - 1, np.int16), one_mask, d_out, 1, 3000, 2, 2)
    with pytest.raises(ValueError, match="d_out"):
        plan.execute_masked_pcm(d_in, one_mask, View(d_out, 0, 4 * 3000 - 1, np.int16), 1, 3000, 2, 2)
    with pytest.raises(ValueError, match="d_out"):
        plan.execute_masked_pcm(d_in, one_mask, View(d_out, 0, 4 * 3000 - 1, np.float32), 1, 3000, 2, 2)   # (a float32 output needs twice the bytes)
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_pcm_ragged(d_in, in_offs, lengths, View(d_mask, 0, int(offs[-1]) - 5, np.float32), mask_offs, d_out, out_offs, 2, 2)
    with pytest.raises(ValueError, match="d_out"):
        plan.execute_masked_pcm_ragged(d_in, in_offs, lengths, d_mask, mask_offs, View(d_out, 0, 4 * len(x) - 1, np.int16), out_offs, 2, 2)
    with pytest.raises(ValueError, match="d_pcm"):
        plan.execute_masked_pcm_ragged(View(d_in, 0, x.size - 1, np.int16), in_offs, lengths, d_mask, mask_offs, d_out, out_offs, 2, 2)
    with pytest.raises(ValueError, match="one entry per clip"):
        plan.execute_masked_pcm_ragged(d_in, in_offs[:2], lengths, d_mask, mask_offs, d_out, out_offs, 2, 2)
    for p in (plan, ft_plan, stft):
        p.sync()
    assert np.array_equal(d_out.download(), sentinel)
    # the same arguments unharmed are accepted: the plan is still usable
    rc, msg = ragged(plan.handle)
    assert rc == 0, msg
    plan.sync()
    assert plan.last_kernel == "k_maskfilter_stereo_pcm_ragged"
    got = d_out.download()
    assert np.array_equal(got[:3000], run_pcm(clips[0][None], masks[0][None], wl, (2, 2), True)[0, 0]) and np.array_equal(got[2 * len(x):], sentinel[2 * len(x):])
    rc, msg = equal(plan.handle)
    assert rc == 0, msg
    plan.sync()
    assert plan.last_kernel == "k_maskfilter_stereo_pcm"
    for buf in (d_in, d_mask, d_out):
        buf.free()


def test_plans_give_their_allocations_back():
    import zafx
    from zafx import _lib

    def live():
        n = ctypes.c_int64(-1)
        assert _lib.load().zafx_plan_live_allocations(ctypes.byref(n)) == 0
        return n.value
    before = live()
    wl, h = 512, 256
    plans = []
    for kind in (zafx.MASKFILTER, zafx.MASKFILTER_REST):
        for form in FORMS:
            lengths = [3 * h + 7, 0, 30 * h]
            clips = [noise(90 + i, n, form[0]) for i, n in enumerate(lengths)]
            masks = [masks_of("unit", wl, n, form, seed=90 + i) for i, n in enumerate(lengths)]
            p = zafx.Plan(kind, window_length=wl, step_length=h, layout="TF")
            p.set_window(zafx.hamming(wl))
            run_ragged_arena(p, clips, masks, form, np.int16, 3, (4, 4, 4))
            plans.append(p)
    assert live() > before
    for p in plans:
        p.destroy()
    assert live() == before
