"""The mask filter under complex masks on the GPU (k_maskfilter_c; zafx_execute_masked_complex, zafx_execute_masked_complex_ragged): parity
with the reference's composition around a complex mask and its Hermitian mirror (tests/golden/maskfilter_complex.npz) and with the float64
oracle at the block and frame-pair edges, the same bits for a clip alone, anywhere in a batch, cut into segments, in a ragged batch and under
other compute-unit counts, the rest, the fixed values (zeros, silence, the discarded imaginary parts of rows 0 and W/2), containment of
non-finite values, NaN-filled arenas at bases 4 bytes off the 8-byte grid, the refusals and the plan's allocations.

Bound: max|y - ref| <= 1e-5 max(max|ref|, max|x|) -- the project's TOL_FFT on mask_error, as for the real kind.  H = W/2 is a block, frame t
covers samples (t - 1) H .. (t + 1) H - 1, and frames 2j and 2j + 1 of a clip share a transform."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from maskfilter_complex_oracle import MASK_KINDS, TOL_FFT, golden_cases, make_complex_mask, mask_error, mask_frames, oracle_maskfilter_complex

pytestmark = pytest.mark.gpu

WINDOWS = (256, 512, 1024, 2048)
FILL = 0x7FC5A5A5   # a quiet NaN no kernel computes
SENTINEL = 0xC640E400   # -12345.0 as float32 bits: the pre-fill of an output no refused or skipped call may touch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clip(seed, n):
    return np.random.default_rng([505, seed, n]).standard_normal(n).astype(np.float32)


def tf(m):
    """Masks (..., W/2 + 1, T) as the device reads them: (..., T, W/2 + 1) complex64, compact."""
    return np.ascontiguousarray(np.swapaxes(np.asarray(m), -1, -2), np.complex64)


def plan_of(wl, rest=False, layout="TF"):
    import zafx
    return zafx.maskfilter_plan(zafx.hamming(wl), rest=rest, layout=layout)


def run_plan(x, m, wl, rest=False):
    """The raw plan on device buffers: x (B, N) float32, m (B, W/2 + 1, T) complex -> the plan's whole output array."""
    import zafx
    plan = plan_of(wl, rest)
    b, n = x.shape
    d_in, d_mask = zafx.DeviceBuffer.from_host(np.ascontiguousarray(x, np.float32)), zafx.DeviceBuffer.from_host(tf(m))
    d_out = zafx.DeviceBuffer(plan.out_shape(b, n), np.float32)
    try:
        assert d_mask.shape == plan.mask_shape(b, n)
        plan.execute_masked_complex(d_in, d_mask, d_out, b, n)
        plan.sync()
        assert plan.last_kernel == "k_maskfilter_complex" and plan.kernel_name == "k_maskfilter"
        return d_out.download()
    finally:
        for buf in (d_in, d_mask, d_out):
            buf.free()


def check(y, ref, x, what):
    err = mask_error(y, ref, x)
    print(f"{what}: {err:.3e} of the level")
    assert np.isfinite(np.asarray(y)).all() and err <= TOL_FFT, (what, err)
    return err


class View:
    """`count` elements of `dtype` at byte `offset` of a DeviceBuffer (nothing to free)."""

    def __init__(self, buf, offset, count, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        self.ptr, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + offset), self.dtype.itemsize * count, (count,)


# ------------------------------------------------------------------------------------------------------------------ 1. golden and oracle
def test_golden_parity():
    import zafx
    for wl, n, x, m, ref in golden_cases():
        w = zafx.hamming(wl)
        y = zafx.maskfilter_complex(x, w, wl // 2, m)
        assert y.dtype == np.float64 and y.shape == (n,)
        check(y, ref, x, f"maskfilter_complex W={wl} N={n}")
        yb = zafx.maskfilter_complex_batch(x[None], w, m[None])
        assert yb.dtype == np.float32 and yb.shape == (1, n)
        check(yb[0], ref, x, f"maskfilter_complex_batch W={wl} N={n}")
        yt = zafx.maskfilter_complex_batch(x[None], w, m.T[None], layout="TF")
        assert np.array_equal(bits(yt), bits(yb)), (wl, "FT and TF host layouts")
        yr, rr = zafx.maskfilter_complex_batch(x[None], w, m[None], step_length=wl // 2, rest=True)
        assert yr.shape == rr.shape == (1, n) and yr.base is rr.base and np.array_equal(bits(yr), bits(yb))
        check(rr[0], x.astype(np.float64) - ref, x, f"rest W={wl} N={n}")
        (ys,) = zafx.maskfilter_complex_ragged([x], w, [m])
        assert np.array_equal(bits(ys), bits(yb[0])), (wl, "ragged")


def edge_lengths(wl):
    h = wl // 2
    return [1, h - 1, h, h + 1, wl, 3 * h + 7]   # T = 2, 2, 2, 3, 3, 5: the last frame pairs with zeros where T is odd


@pytest.mark.parametrize("wl", WINDOWS)
def test_oracle_parity_at_the_edges(wl):
    import zafx
    w = zafx.hamming(wl)
    assert {mask_frames(n, wl) % 2 for n in edge_lengths(wl)} == {0, 1}
    worst = 0.0
    for n in edge_lengths(wl):
        x = np.stack([clip(k, n) for k in range(len(MASK_KINDS))])
        m = np.stack([make_complex_mask(kind, wl, n) for kind in MASK_KINDS])
        y = run_plan(x, m, wl)
        both = zafx.maskfilter_complex_batch(x, w, m), zafx.maskfilter_complex_batch(x, w, m.transpose(0, 2, 1), layout="TF")
        assert np.array_equal(bits(both[0]), bits(y)) and np.array_equal(bits(both[1]), bits(y)), (wl, n)
        for k, kind in enumerate(MASK_KINDS):
            worst = max(worst, check(y[k], oracle_maskfilter_complex(x[k], w, m[k]), x[k], f"W={wl} N={n} {kind}"))
    print(f"W={wl}: worst {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------------ 2. tiles, carry, segments
@pytest.mark.parametrize("wl", WINDOWS)
def test_a_clip_has_the_same_bits_anywhere(wl):
    """The clip of 60 blocks + 5 samples (several tiles: the carry is handed on) alone -- a batch too small for the device, so it is cut into
    segments --, as the first, a middle and the last clip of batches of 2, 3 and 5, and in a ragged batch."""
    import zafx
    from maskfilter_complex_probe import probe_case
    w = zafx.hamming(wl)
    x, m = probe_case(wl)
    alone = run_plan(x[2:3], m[2:3], wl)[0]
    check(alone, oracle_maskfilter_complex(x[2], w, m[2]), x[2], f"W={wl} the 60-block clip")
    for order in ([2, 0], [0, 2], [2, 1, 0], [1, 2, 0], [0, 1, 2], [2, 0, 1, 3, 0], [0, 1, 2, 3, 1], [3, 1, 0, 0, 2]):
        out = run_plan(x[order], m[order], wl)
        assert np.array_equal(bits(out[order.index(2)]), bits(alone)), (wl, order)
    ys = zafx.maskfilter_complex_ragged([x[0, :5], x[2], x[1]], w, [m[0, :, :2], m[2], m[1]])
    assert np.array_equal(bits(ys[1]), bits(alone)), (wl, "ragged")


def test_whole_clips_give_the_bits_of_segments():
    """In a batch of as many clips as the device has workgroup slots the clips stay whole; alone the clip is cut."""
    from maskfilter_complex_probe import probe_case
    wl = 256
    x, m = probe_case(wl)
    clips = 4 * plan_of(wl).compute_units   # (at most four workgroups fit a compute unit: one slot each)
    alone = run_plan(x[2:3], m[2:3], wl)[0]
    idx = np.arange(clips) % 4
    whole = run_plan(x[idx], m[idx], wl)
    for i in (2, clips - 2):
        assert idx[i] == 2 and np.array_equal(bits(whole[i]), bits(alone)), i


@pytest.mark.timeout(300)
@pytest.mark.parametrize("units", [1, 3])
def test_other_compute_unit_counts_give_the_same_bits(tmp_path, units):
    """The same clip in a fresh child process under ZAFX_COMPUTE_UNITS=1 and =3: other cuts, every unit on a few workgroups."""
    import zafx
    from maskfilter_complex_probe import WINDOWS as PROBE_WINDOWS, probe_case
    path = str(tmp_path / "probe.npz")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maskfilter_complex_probe.py"), path], env=dict(os.environ, ZAFX_COMPUTE_UNITS=str(units)),
                         capture_output=True, timeout=240)
    assert res.returncode == 0 and b"probe ok" in res.stdout, res.stderr.decode()[-2000:]
    got = np.load(path)
    for wl in PROBE_WINDOWS:
        x, m = probe_case(wl)
        assert int(got[f"units{wl}"]) == units and plan_of(wl).compute_units > units
        here = run_plan(x[2:3], m[2:3], wl)[0]
        for name in ("alone", "batch", "ragged"):
            assert np.array_equal(bits(got[f"{name}{wl}"]), bits(here)), (wl, name)


# ------------------------------------------------------------------------------------------------------------------ 3. rest
@pytest.mark.parametrize("wl", WINDOWS)
def test_rest(wl):
    h = wl // 2
    for n in (1, 3 * h + 7, 20 * h + 5):
        x = np.stack([clip(10 + k, n) for k in range(3)])
        m = np.stack([make_complex_mask("disc", wl, n, seed=k) for k in range(3)])
        both, only = run_plan(x, m, wl, rest=True), run_plan(x, m, wl)
        assert both.shape == (3, 2, n)
        assert np.array_equal(bits(both[:, 0]), bits(only)), (wl, n)
        assert np.array_equal(bits(both[:, 1]), bits(x - both[:, 0])), (wl, n)


# ------------------------------------------------------------------------------------------------------------------ 4. fixed values
@pytest.mark.parametrize("wl", WINDOWS)
def test_fixed_values(wl):
    """A mask of zeros and silence under the "big" mask give zeros; NaN in the imaginary parts of rows 0 and W/2 gives the bytes of zeros there;
    a mask without imaginary parts is within the bound of the real kind's result on a TF plan."""
    import zafx
    w, h = zafx.hamming(wl), wl // 2
    n = 9 * h + 3
    x = np.stack([clip(20 + k, n) for k in range(2)])
    t = mask_frames(n, wl)
    out = run_plan(x, np.zeros((2, h + 1, t), np.complex64), wl, rest=True)
    assert not out[:, 0].any() and np.array_equal(bits(out[:, 1]), bits(x))
    big = np.stack([make_complex_mask("big", wl, n, seed=k) for k in range(2)])
    assert not run_plan(np.zeros_like(x), big, wl, rest=True).any()
    m = np.stack([make_complex_mask("disc", wl, n, seed=k) for k in range(2)])
    zeros, nans = m.copy(), m.copy()
    for a, v in ((zeros, 0.0), (nans, np.nan)):
        a[:, 0].imag = v
        a[:, -1].imag = v
    assert np.isnan(nans[:, 0].imag).all() and np.isnan(nans[:, -1].imag).all()
    got = run_plan(x, nans, wl)
    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(run_plan(x, zeros, wl)))
    for k in range(2):
        check(got[k], oracle_maskfilter_complex(x[k], w, m[k]), x[k], f"W={wl} NaN in Im of rows 0 and W/2, clip {k}")
    real = np.stack([make_complex_mask("real", wl, n, seed=k) for k in range(2)])
    yc = run_plan(x, real, wl)
    yr = zafx.maskfilter_batch(x, w, np.ascontiguousarray(real.real.transpose(0, 2, 1)), layout="TF")
    for k in range(2):
        check(yc[k], oracle_maskfilter_complex(x[k], w, real[k]), x[k], f"W={wl} real mask against the oracle, clip {k}")
        err = mask_error(yc[k], yr[k], x[k])
        assert err <= TOL_FFT, (wl, k, err)
    print(f"W={wl}: real mask, complex kernel against k_maskfilter: bits {'agree' if np.array_equal(bits(yc), bits(yr)) else 'differ'}, "
          f"{max(mask_error(yc[k], yr[k], x[k]) for k in range(2)):.3e} of the level")


# ------------------------------------------------------------------------------------------------------------------ 5. containment
def touched(n, h, frames):
    """The samples of a clip of n that frames `frames` reach, partners included: frames 2j and 2j + 1 share a transform, frame t covers
    samples (t - 1) H .. (t + 1) H - 1."""
    hit = np.zeros(n, bool)
    for t in frames:
        for u in (t, t ^ 1):
            hit[max((u - 1) * h, 0):min((u + 1) * h, n)] = True
    return hit


@pytest.mark.parametrize("wl", [256, 2048])
def test_containment(wl):
    """A NaN sample and a NaN mask value in clip 1 of three: clips 0 and 2 have the bits of their runs alone; inside clip 1 the samples of the
    frames that hold the NaN sample or mask value, and of the frames paired with them, may be non-finite -- every other sample has the bits
    of the clean run."""
    h = wl // 2
    n = 20 * h + 9
    x = np.stack([clip(30 + k, n) for k in range(3)])
    m = np.stack([make_complex_mask("disc", wl, n, seed=30 + k) for k in range(3)])
    clean = run_plan(x, m, wl)
    s, (k, t) = 5 * h + 17, (h // 3, 13)   # sample s lies in frames 5 and 6; the mask value in frame 13
    xp, mp = x.copy(), m.copy()
    xp[1, s] = np.nan
    mp[1, k, t] = np.nan + 0j
    got = run_plan(xp, mp, wl)
    for c in (0, 2):
        assert np.array_equal(bits(got[c]), bits(run_plan(x[c:c + 1], m[c:c + 1], wl)[0])) and np.array_equal(bits(got[c]), bits(clean[c])), (wl, c)
    may = touched(n, h, [s // h, s // h + 1, t])
    assert not np.isfinite(got[1][may]).all() and np.isfinite(got[1][~may]).all()
    assert np.array_equal(bits(got[1][~may]), bits(clean[1][~may])) and 0 < may.sum() < n


# ------------------------------------------------------------------------------------------------------------------ 6, 7. ragged, arena
def ragged_lengths(wl):
    h = wl // 2
    return [0, 1, h, 60 * h + 5, 3 * h + 7, h + 1, 0, 2 * wl]


def batch_of(wl, lengths, seed=0):
    return [clip(seed + i, n) for i, n in enumerate(lengths)], [make_complex_mask("disc", wl, n, seed=seed + i) for i, n in enumerate(lengths)]


def place(sizes, gap, base):
    """-> (offsets, total): blocks of `sizes` elements, `gap` elements between them, the first at element `base`, `gap` + 1 behind the last."""
    offs, at = [], base
    for s in sizes:
        offs.append(at)
        at += s + gap
    return np.array(offs, np.int64), at + 1


def run_ragged(plan, clips, masks, gap=0, byte_bases=(0, 0, 0)):
    """One zafx_execute_masked_complex_ragged: samples, masks and output blocks each inside an arena -- NaN words around the clips and the masks,
    SENTINEL words in the output --, `gap` elements between neighbours (float32 words; complex64 elements for the masks), the three arrays
    `byte_bases` bytes into their allocations.  -> (the per-clip results (blocks, N_i), after checking every other output word kept SENTINEL)."""
    import zafx
    blocks = 2 if plan.kind == zafx.MASKFILTER_REST else 1
    lengths = np.array([len(c) for c in clips], np.int64)
    flat = [tf(m).ravel() for m in masks]
    in_offs, in_words = place(lengths.tolist(), gap, 0)
    mask_offs, mask_elems = place([len(f) for f in flat], gap, 0)
    out_offs, out_words = place((blocks * lengths).tolist(), gap, 0)
    pad = [b // 4 for b in byte_bases]
    assert all(b % 4 == 0 for b in byte_bases)
    h_in, h_mask = np.full(pad[0] + in_words, FILL, np.uint32), np.full(pad[1] + 2 * mask_elems, FILL, np.uint32)
    for c, o in zip(clips, in_offs.tolist()):
        h_in[pad[0] + o:pad[0] + o + len(c)] = bits(c)
    for f, o in zip(flat, mask_offs.tolist()):
        h_mask[pad[1] + 2 * o:pad[1] + 2 * (o + len(f))] = f.view(np.uint32)
    h_out = np.full(pad[2] + out_words, SENTINEL, np.uint32)
    bufs = [zafx.DeviceBuffer.from_host(a) for a in (h_in, h_mask, h_out)]
    views = [View(bufs[0], byte_bases[0], in_words), View(bufs[1], byte_bases[1], mask_elems, np.complex64), View(bufs[2], byte_bases[2], out_words)]
    try:
        plan.execute_masked_complex_ragged(views[0], in_offs, lengths, views[1], mask_offs, views[2], out_offs)
        plan.sync()
        if lengths.any():
            assert plan.last_kernel == "k_maskfilter_complex_ragged" and plan.kernel_name == "k_maskfilter"
        words = bufs[2].download()
    finally:
        for b in bufs:
            b.free()
    kept = np.ones(len(words), bool)
    res = []
    for o, n in zip((out_offs + pad[2]).tolist(), lengths.tolist()):
        kept[o:o + blocks * n] = False
        res.append(words[o:o + blocks * n].view(np.float32).reshape(blocks, n))
    assert (words[kept] == SENTINEL).all(), "written outside the clips' blocks"
    return res


_ALONE = {}


def alone(wl, rest, x, m, key):
    key = (wl, rest) + tuple(key)
    if key not in _ALONE:
        _ALONE[key] = run_plan(x[None], m[None], wl, rest=rest)[0].reshape(2 if rest else 1, len(x))
    return _ALONE[key]


def assert_equal_alone(res, clips, masks, wl, rest, seed, what=""):
    for i, (r, x, m) in enumerate(zip(res, clips, masks)):
        if not len(x):
            assert r.size == 0
            continue
        assert np.array_equal(bits(r), bits(alone(wl, rest, x, m, (seed, i)))), (what, wl, rest, i, len(x))


@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("wl", WINDOWS)
def test_ragged_bitwise_against_the_clip_alone(monkeypatch, wl, rest):
    clips, masks = batch_of(wl, ragged_lengths(wl))
    plan = plan_of(wl, rest)
    for per_slot in (None, "1"):
        if per_slot:
            monkeypatch.setenv("ZAFX_MASKFILTER_UNITS_PER_SLOT", per_slot)
        else:
            monkeypatch.delenv("ZAFX_MASKFILTER_UNITS_PER_SLOT", raising=False)
        assert_equal_alone(run_ragged(plan, clips, masks), clips, masks, wl, rest, 0, what=f"units per slot {per_slot}")


def test_ragged_empty_batches_write_nothing():
    plan = plan_of(512, True)
    assert run_ragged(plan, [], []) == []
    clips, masks = batch_of(512, [0, 0, 0])
    assert all(r.size == 0 for r in run_ragged(plan, clips, masks))


def test_mask_layout_is_that_of_a_ragged_onesided_tf_stft():
    """mask_offsets count complex64 elements, compact: what zafx_plan_ragged_layout gives a one-sided complex TF STFT plan of the same window."""
    import zafx
    for wl in WINDOWS:
        w, h = zafx.hamming(wl), wl // 2
        lengths = np.array(ragged_lengths(wl), np.int64)
        spec = zafx.stft_plan(w, h, layout="TF", onesided=True)
        offs, frames, _ = spec.ragged_layout(lengths)
        assert spec.out_dtype == np.complex64 and plan_of(wl).mask_ragged_layout(lengths).tolist() == offs.tolist(), wl
        assert frames.tolist() == [mask_frames(n, wl) for n in lengths.tolist()]


@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("wl", [2048, 256])
def test_ragged_arena(wl, rest):
    """Clips, masks and output blocks back to back and with gaps, NaN between the clips and between the masks, the arrays 4 bytes off the
    16-byte grid -- the complex mask 4 bytes off the 8-byte grid --: nothing outside the blocks is written, and no clip sees its neighbour's
    samples or mask."""
    clips, masks = batch_of(wl, ragged_lengths(wl))
    plan = plan_of(wl, rest)
    for gap, bases in ((0, (4, 4, 4)), (37, (20, 12, 36))):
        assert bases[0] % 16 == 4 and bases[1] % 8 == 4 and bases[2] % 16 == 4
        res = run_ragged(plan, clips, masks, gap=gap, byte_bases=bases)
        for r in res:
            assert np.isfinite(r).all()
        assert_equal_alone(res, clips, masks, wl, rest, 0, what=f"gap {gap}")


@pytest.mark.parametrize("rest", [False, True])
def test_arena_equal_length(rest):
    """zafx_execute_masked_complex on slices of larger buffers: samples and output 4 bytes off the 16-byte grid, the mask 4 bytes off the 8-byte
    grid, NaN around the inputs; nothing but the output is written."""
    import zafx
    guard = 64 * 1024
    for wl, n, deltas in ((2048, 9 * 1024 + 1, (4, 132, 20)), (256, 16 * 128 - 1, (132, 4, 68))):
        plan = plan_of(wl, rest)
        x = np.stack([clip(40 + k, n) for k in range(3)])
        m = np.stack([make_complex_mask("disc", wl, n, seed=40 + k) for k in range(3)])
        laid = tf(m)
        n_out = int(np.prod(plan.out_shape(3, n)))
        arenas, views = [], []
        for data, words, delta, dtype, fill in ((bits(x), x.size, deltas[0], np.float32, FILL), (laid.view(np.uint32), 2 * laid.size, deltas[1], np.complex64, FILL),
                                                (None, n_out, deltas[2], np.float32, SENTINEL)):
            assert delta % 8 == 4
            host = np.full((2 * guard + delta) // 4 + words, fill, np.uint32)
            lo = (guard + delta) // 4
            if data is not None:
                host[lo:lo + words] = data.ravel()
            buf = zafx.DeviceBuffer.from_host(host)
            arenas.append((buf, host, lo, words))
            views.append(View(buf, guard + delta, words // (2 if dtype is np.complex64 else 1), dtype))
        try:
            plan.execute_masked_complex(views[0], views[1], views[2], 3, n)
            plan.sync()
            buf, host, lo, words = arenas[2]
            got = buf.download()
        finally:
            for a in arenas:
                a[0].free()
        assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + words:], host[lo + words:]), "written outside the output"
        out = got[lo:lo + words].view(np.float32).reshape(plan.out_shape(3, n))
        assert np.array_equal(bits(out), bits(run_plan(x, m, wl, rest=rest))), (wl, rest)


# ------------------------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_output_untouched():
    import zafx
    from zafx import _lib
    lib = _lib.load()
    wl, h = 512, 256
    w = zafx.hamming(wl)
    lengths = np.array([3000, 0, 700], np.int64)
    clips, masks = batch_of(wl, lengths.tolist(), seed=50)
    plan, ft_plan, stft = plan_of(wl, True), plan_of(wl, True, layout="FT"), zafx.stft_plan(w, h)
    x = np.concatenate(clips)
    in_offs = np.array([0, 3000, 3000], np.int64)
    mask_offs = plan.mask_ragged_layout(lengths)
    assert mask_offs.tolist() == np.concatenate(([0], np.cumsum([mask_frames(n, wl) * (h + 1) for n in lengths.tolist()]))).tolist()
    out_offs = 2 * in_offs
    sentinel = np.full(2 * len(x), -12345.5, np.float32)
    d_in, d_out = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(sentinel)
    packed = np.concatenate([tf(m).ravel() for m in masks])
    d_mask = zafx.DeviceBuffer.from_host(packed)
    real_mask = zafx.DeviceBuffer.from_host(np.ascontiguousarray(packed.real))
    p64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731

    def ragged(pl, a_in=d_in.ptr, a_inoff=in_offs, a_len=lengths, a_mask=d_mask.ptr, a_moff=mask_offs, a_out=d_out.ptr, a_ooff=out_offs, n=3):
        rc = lib.zafx_execute_masked_complex_ragged(pl, a_in, None if a_inoff is None else p64(a_inoff), None if a_len is None else p64(a_len), a_mask,
                                                    None if a_moff is None else p64(a_moff), a_out, None if a_ooff is None else p64(a_ooff), n)
        return rc, (lib.zafx_last_error() or b"").decode()

    def equal(pl, a_in=d_in.ptr, a_mask=d_mask.ptr, a_out=d_out.ptr, b=1, n=3000):
        return lib.zafx_execute_masked_complex(pl, a_in, a_mask, a_out, b, n), (lib.zafx_last_error() or b"").decode()

    def neg(a, i):
        b = a.copy()
        b[i] = -1
        return b

    # the parent's bytes of the real entry points on the same plan, before and after
    def real_kinds():
        res = []
        for call in (lambda o: plan.execute_masked(d_in, View(real_mask, 0, mask_frames(3000, wl) * (h + 1)), o, 1, 3000),
                     lambda o: plan.execute_masked_ragged(d_in, in_offs, lengths, real_mask, mask_offs, o, out_offs)):
            o = zafx.DeviceBuffer.from_host(sentinel)
            call(o)
            plan.sync()
            res.append(o.download())
            o.free()
        return res
    before = real_kinds()

    big = lengths.copy()
    big[2] = 1 << 27
    cases = [
        (dict(pl=None), "null plan"),
        (dict(a_in=None), "null device pointer"), (dict(a_mask=None), "null device pointer"), (dict(a_out=None), "null device pointer"),
        (dict(a_inoff=None), "null argument"), (dict(a_len=None), "null argument"), (dict(a_moff=None), "null argument"), (dict(a_ooff=None), "null argument"),
        (dict(n=-1), "negative number of clips"),
        (dict(a_len=neg(lengths, 1)), "of clip 1"), (dict(a_inoff=neg(in_offs, 2)), "of clip 2"), (dict(a_moff=neg(mask_offs, 0)), "of clip 0"),
        (dict(a_ooff=neg(out_offs, 2)), "of clip 2"),
        (dict(a_len=big), "2^27 samples or more (not supported): clip 2"),   # by `lengths` alone: the buffers are those of the small batch
        (dict(pl=ft_plan.handle), "ZAFX_LAYOUT_TF"), (dict(pl=ft_plan.handle, n=0), "ZAFX_LAYOUT_TF"),
        (dict(pl=stft.handle), "ZAFX_MASKFILTER"),
    ]
    for kw, text in cases:
        kw.setdefault("pl", plan.handle)
        rc, msg = ragged(**kw)
        assert rc != 0 and text in msg, (list(kw), rc, msg)
        if "of clip" in text:
            assert "negative" in msg
    for kw, text in [(dict(pl=None), "null plan"), (dict(a_in=None), "null device pointer"), (dict(a_mask=None), "null device pointer"),
                     (dict(a_out=None), "null device pointer"), (dict(b=-1), "negative size"), (dict(n=-1), "negative size"),
                     (dict(n=1 << 27), "2^27"), (dict(n=1 << 27, b=0), "2^27"), (dict(pl=ft_plan.handle), "ZAFX_LAYOUT_TF"),
                     (dict(pl=ft_plan.handle, b=0), "ZAFX_LAYOUT_TF"), (dict(pl=stft.handle), "ZAFX_MASKFILTER")]:
        kw.setdefault("pl", plan.handle)
        rc, msg = equal(**kw)
        assert rc != 0 and text in msg, (list(kw), rc, msg)
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
    # through the Python layer: the library's refusals arrive, wrong dtypes and sizes are caught in front of it
    with pytest.raises(zafx.ZafxError, match="ZAFX_LAYOUT_TF"):
        ft_plan.execute_masked_complex(d_in, d_mask, d_out, 1, 3000)
    with pytest.raises(zafx.ZafxError, match="ZAFX_LAYOUT_TF"):
        ft_plan.execute_masked_complex_ragged(d_in, in_offs, lengths, d_mask, mask_offs, d_out, out_offs)
    with pytest.raises(zafx.ZafxError, match="MASKFILTER"):
        stft.execute_masked_complex(d_in, d_mask, d_out, 1, 3000)
    with pytest.raises(ValueError, match="complex64"):
        plan.execute_masked_complex(d_in, real_mask, d_out, 1, 3000)
    with pytest.raises(ValueError, match="complex64"):
        plan.execute_masked_complex_ragged(d_in, in_offs, lengths, real_mask, mask_offs, d_out, out_offs)
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_complex(d_in, d_mask, d_out, 1, 3000)   # the masks of three clips for one
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_complex_ragged(d_in, in_offs, lengths, View(d_mask, 0, int(mask_offs[-1]) - 5, np.complex64), mask_offs, d_out, out_offs)
    with pytest.raises(ValueError, match="d_out"):
        plan.execute_masked_complex_ragged(d_in, in_offs, lengths, d_mask, mask_offs, View(d_out, 0, len(sentinel) - 1), out_offs)
    with pytest.raises(ValueError, match="one entry per clip"):
        plan.execute_masked_complex_ragged(d_in, in_offs[:2], lengths, d_mask, mask_offs, d_out, out_offs)
    # the real functions keep refusing complex masks, the other entry points the kind
    with pytest.raises(ValueError, match="real"):
        zafx.maskfilter_batch(clips[0][None], w, masks[0][None])
    with pytest.raises(zafx.ZafxError, match="zafx_execute_masked"):
        plan.execute(d_in, d_out, 1, 3000)
    for p in (plan, ft_plan, stft):
        p.sync()
    assert np.array_equal(bits(d_out.download()), bits(sentinel))
    # ... the real entry points on the same plan give their earlier bytes, and the same arguments unharmed are accepted
    after = real_kinds()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before, after))
    rc, msg = ragged(plan.handle)
    assert rc == 0, msg
    plan.sync()
    assert plan.last_kernel == "k_maskfilter_complex_ragged"
    rc, msg = equal(plan.handle)
    assert rc == 0, msg
    plan.sync()
    assert plan.last_kernel == "k_maskfilter_complex"
    for buf in (d_in, d_mask, real_mask, d_out):
        buf.free()


# ------------------------------------------------------------------------------------------------------------------ 9. allocations
def test_plans_give_their_allocations_back():
    import zafx
    from zafx import _lib

    def live():
        n = ctypes.c_int64(-1)
        assert _lib.load().zafx_plan_live_allocations(ctypes.byref(n)) == 0
        return n.value
    before = live()
    wl, h = 512, 256
    clips, masks = batch_of(wl, [3 * h + 7, 0, 30 * h], seed=70)
    plans = []
    for kind in (zafx.MASKFILTER, zafx.MASKFILTER_REST):
        p = zafx.Plan(kind, window_length=wl, step_length=h, layout="TF")
        p.set_window(zafx.hamming(wl))
        res = run_ragged(p, clips, masks)
        assert all(np.isfinite(r).all() for r in res)
        plans.append(p)
    assert live() > before
    for p in plans:
        p.destroy()
    assert live() == before
