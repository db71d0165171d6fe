"""Mask filter on the GPU (k_maskfilter; ZAFX_MASKFILTER, ZAFX_MASKFILTER_REST): parity with the reference's composition of zaf.stft /
zaf.istft around a real mask (tests/golden/maskfilter.npz) and with the oracle's at the pair, tile and segment edges in every mask layout,
the identity, the fixed edge values, bit-level agreement of the two kinds, independence of the clips of a batch and of the compute-unit
count, arrays inside larger buffers with NaN guards, the center / sides extraction as a cross-check, a window replaced on a used plan, and
the refusals.

Bound: max|y - ref| <= 1e-5 max(max|ref|, max|x|) -- the project's TOL_FFT for a float32 transform chain against float64, at the larger of
the reference's and the input's level (a sparse mask leaves a reference far below the input whose rounding error it inherits).  Test masks
lie in [0, 1] but "signed_wide", uniform in [-2, 2].  F is the number of packed transforms per tile, so a tile is 2 F frames."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from maskfilter_oracle import TOL_FFT, golden_cases, make_mask, mask_error, mask_frames, oracle_maskfilter

pytestmark = pytest.mark.gpu

WINDOWS = (256, 512, 1024, 2048)
LAYOUTS = (("FT", 0), ("FT", 32), ("TF", 0))   # (layout, row_align)
FILL = 0x7FC5A5A5   # a quiet NaN no kernel computes


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clip(seed, n):
    return np.random.default_rng([303, seed, n]).standard_normal(n).astype(np.float32)


def lay_out(plan, m, n, pad=np.nan):
    """Masks (B, W/2 + 1, T) as the array the plan reads: (B, W/2 + 1, pitch) with `pad` in the row padding, or (B, T, W/2 + 1)."""
    import zafx
    shape = plan.mask_shape(m.shape[0], n)
    if plan.layout == zafx.LAYOUT_TF:
        out = np.ascontiguousarray(m.transpose(0, 2, 1), np.float32)
    else:
        out = np.full(shape, pad, np.float32)
        out[:, :, :m.shape[2]] = m
    assert out.shape == shape, (out.shape, shape)
    return out


def run_plan(x, m, w, rest=False, layout="FT", row_align=0, plan=None):
    """The raw plan on device buffers: x (B, N), m (B, W/2 + 1, T) -> the plan's whole output array."""
    import zafx
    plan = plan or zafx.maskfilter_plan(w, rest=rest, layout=layout, row_align=row_align)
    b, n = x.shape
    d_in, d_mask = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(lay_out(plan, m, n))
    d_out = zafx.DeviceBuffer(plan.out_shape(b, n), np.float32)
    try:
        plan.execute_masked(d_in, d_mask, d_out, b, n)
        plan.sync()
        assert plan.last_kernel == "k_maskfilter" and plan.kernel_name == "k_maskfilter"
        return d_out.download()
    finally:
        for buf in (d_in, d_mask, d_out):
            buf.free()


def check(y, ref, x, what):
    err = mask_error(y, ref, x)
    print(f"{what}: {err:.3e} of the level")
    assert np.isfinite(np.asarray(y)).all() and err <= TOL_FFT, (what, err)
    return err


def test_golden_parity():
    import zafx
    for wl, n, x, m, ref in golden_cases():
        w = zafx.hamming(wl)
        y = zafx.maskfilter(x, w, wl // 2, m)
        assert y.dtype == np.float64 and y.shape == (n,)
        check(y, ref, x, f"maskfilter W={wl} N={n}")
        yb = zafx.maskfilter_batch(x[None], w, m[None])
        assert yb.dtype == np.float32 and yb.shape == (1, n)
        check(yb[0], ref, x, f"maskfilter_batch W={wl} N={n}")
        yr, rr = zafx.maskfilter_batch(x[None], w, m[None], step_length=wl // 2, rest=True)
        assert yr.shape == rr.shape == (1, n) and yr.base is rr.base
        check(yr[0], ref, x, f"maskfilter_batch rest W={wl} N={n}")
        check(rr[0], x.astype(np.float64) - ref, x, f"rest W={wl} N={n}")
        yt = zafx.maskfilter_batch(x[None], w, m.T[None], layout="TF")
        check(yt[0], ref, x, f"maskfilter_batch TF W={wl} N={n}")
        raw = run_plan(x[None], m[None], w, rest=True, row_align=32)
        assert raw.shape == (1, 2, n)
        check(raw[0, 0], ref, x, f"raw plan W={wl} N={n}")
        plan = zafx.maskfilter_plan(w, rest=True, row_align=32)
        t = mask_frames(n, wl)
        assert plan.mask_dims(n) == (wl // 2 + 1, t) and plan.row_pitch(n) == -(-t // 32) * 32 and plan.out_dims(n) == (2 * n, 1)
        assert plan.clip_bytes(n) == (4 * n, 8 * n) and zafx.maskfilter_plan(w, layout="TF").row_pitch(n) == wl // 2 + 1


def edge_lengths(wl):
    import zafx
    h, f = wl // 2, zafx.maskfilter_tile_transforms(wl)
    assert f in (4, 8)
    return [1, h - 1, h, h + 1, 2 * h - 1, 2 * h, 2 * h + 1, 2 * f * h - 1, 2 * f * h, 2 * f * h + 1, 4 * f * h + 3, 44100]


EDGE_MASKS = ("ones", "uniform", "sparse", "signed_wide")   # ones, uniform [0.25, 1], 2 % sparse, uniform [-2, 2]


@pytest.fixture(scope="module")
def edge_cases():
    """Per W: [(N, x (4, N), masks (4, W/2 + 1, T): EDGE_MASKS, refs)], the oracle computed once."""
    import zafx
    cases = {}
    for wl in WINDOWS:
        w = zafx.hamming(wl)
        cases[wl] = []
        for n in edge_lengths(wl):
            x = np.stack([clip(k, n) for k in range(len(EDGE_MASKS))])
            m = np.stack([make_mask(kind, wl, n) for kind in EDGE_MASKS])
            cases[wl].append((n, x, m, [oracle_maskfilter(x[k], w, m[k]) for k in range(len(EDGE_MASKS))]))
    return cases


@pytest.mark.parametrize("layout, row_align", LAYOUTS)
@pytest.mark.parametrize("wl", WINDOWS)
def test_oracle_parity_at_the_edges(edge_cases, wl, layout, row_align):
    import zafx
    w = zafx.hamming(wl)
    worst = 0.0
    for n, x, m, refs in edge_cases[wl]:
        y = run_plan(x, m, w, layout=layout, row_align=row_align)
        for k, kind in enumerate(EDGE_MASKS):
            worst = max(worst, check(y[k], refs[k], x[k], f"W={wl} N={n} {layout}/{row_align} {kind}"))
    print(f"W={wl} {layout}/{row_align}: worst {worst:.3e}")


@pytest.mark.parametrize("wl", WINDOWS)
def test_identity(wl):
    """Hamming at H = W/2 is COLA: a mask of ones returns the clip."""
    import zafx
    n = 9 * wl + 5
    x = np.stack([clip(k, n) for k in range(2)])
    y = run_plan(x, np.ones((2, wl // 2 + 1, mask_frames(n, wl)), np.float32), zafx.hamming(wl))
    for k in range(2):
        check(y[k], x[k], x[k], f"identity W={wl}")


@pytest.mark.parametrize("layout, row_align", LAYOUTS)
def test_zeros(layout, row_align):
    import zafx
    for wl in (2048, 256):
        w, n = zafx.hamming(wl), 7 * wl + 3
        x = np.stack([clip(k, n) for k in range(2)])
        t = mask_frames(n, wl)
        out = run_plan(x, np.zeros((2, wl // 2 + 1, t), np.float32), w, rest=True, layout=layout, row_align=row_align)
        assert not out[:, 0].any() and np.array_equal(bits(out[:, 1]), bits(x))
        wild = (np.random.default_rng(wl).random((2, wl // 2 + 1, t)) * 2e30 - 1e30).astype(np.float32)
        out = run_plan(np.zeros_like(x), wild, w, rest=True, layout=layout, row_align=row_align)
        assert not out.any()


def test_two_kinds_agree_bitwise():
    import zafx
    for wl, n in [(2048, 50001), (1024, 30000), (512, 9999), (256, 5000)]:
        w = zafx.hamming(wl)
        x = np.stack([clip(7 * i + wl, n) for i in range(5)])
        m = np.stack([make_mask("unit", wl, n, seed=i) for i in range(5)])
        for layout, row_align in LAYOUTS:
            both, only = run_plan(x, m, w, True, layout, row_align), run_plan(x, m, w, False, layout, row_align)
            assert np.array_equal(bits(both[:, 0]), bits(only)), (wl, layout)
            assert np.array_equal(bits(both[:, 1]), bits(x - both[:, 0])), (wl, layout)


@pytest.mark.parametrize("layout, row_align", LAYOUTS)
def test_batch_independence(layout, row_align):
    import zafx
    wl, n = 512, 40 * 256 + 11
    w = zafx.hamming(wl)
    x = np.stack([clip(i % 30, n) for i in range(37)])   # clips 30 .. 36 repeat clips 0 .. 6, samples and masks
    m = np.stack([make_mask("unit", wl, n, seed=i % 30) for i in range(37)])
    out = run_plan(x, m, w, True, layout, row_align)
    for i in range(30, 37):
        assert np.array_equal(bits(out[i]), bits(out[i - 30])), i
    for i in (0, 5, 17, 36):
        assert np.array_equal(bits(run_plan(x[i:i + 1], m[i:i + 1], w, True, layout, row_align)[0]), bits(out[i])), i
    check(out[17, 0], oracle_maskfilter(x[17], w, m[17]), x[17], "clip 17 of 37")


def touched(n, h, frames):
    """The samples of a clip of n that frames `frames` reach, partners included: frames 2j and 2j + 1 share a transform, frame t covers
    samples (t - 1) H .. (t + 1) H - 1."""
    hit = np.zeros(n, bool)
    for t in frames:
        for u in (t, t ^ 1):
            hit[max((u - 1) * h, 0):min((u + 1) * h, n)] = True
    return hit


@pytest.mark.parametrize("layout, row_align", LAYOUTS)
@pytest.mark.parametrize("wl", [256, 2048])
def test_containment(wl, layout, row_align):
    """A NaN sample and a NaN mask value in clip 1 of three (the "FT" forms stage several frames of mask in LDS): clips 0 and 2 have the bits of
    their runs alone and of the clean batch; inside clip 1 the samples of the frames that hold the NaN sample or mask value, and of the frames
    paired with them, may be non-finite -- every other sample has the bits of the clean run."""
    import zafx
    w, h = zafx.hamming(wl), wl // 2
    n = 20 * h + 9
    x = np.stack([clip(30 + k, n) for k in range(3)])
    m = np.stack([make_mask("unit", wl, n, seed=30 + k) for k in range(3)])
    clean = run_plan(x, m, w, layout=layout, row_align=row_align)
    s, (k, t) = 5 * h + 17, (h // 3, 13)   # sample s lies in frames 5 and 6; the mask value in frame 13
    xp, mp = x.copy(), m.copy()
    xp[1, s] = np.nan
    mp[1, k, t] = np.nan
    got = run_plan(xp, mp, w, layout=layout, row_align=row_align)
    for c in (0, 2):
        alone = run_plan(x[c:c + 1], m[c:c + 1], w, layout=layout, row_align=row_align)[0]
        assert np.array_equal(bits(got[c]), bits(alone)) and np.array_equal(bits(got[c]), bits(clean[c])), (wl, layout, c)
    may = touched(n, h, [s // h, s // h + 1, t])
    assert not np.isfinite(got[1][may]).all() and np.isfinite(got[1][~may]).all()
    assert np.array_equal(bits(got[1][~may]), bits(clean[1][~may])) and 0 < may.sum() < n


def test_segments_give_the_bits_of_whole_clips():
    """One 60-block clip alone is cut into segments; in a batch of as many clips as the device has workgroup slots the clips stay whole."""
    import zafx
    from maskfilter_probe import probe_case
    wl = 256
    w = zafx.hamming(wl)
    x, m = probe_case(wl)
    plan = zafx.maskfilter_plan(w)
    clips = 4 * plan.compute_units   # (four workgroups of k_maskfilter fit a compute unit at W = 256: one slot each)
    alone = run_plan(x[2:3], m[2:3], w)[0]
    idx = np.arange(clips) % 4
    whole = run_plan(x[idx], m[idx], w)
    for i in (2, clips - 2):
        assert idx[i] == 2 and np.array_equal(bits(whole[i]), bits(alone)), i
    check(alone, oracle_maskfilter(x[2], w, m[2]), x[2], "the 60-block clip")


@pytest.mark.timeout(300)
def test_one_compute_unit_gives_the_same_bits(tmp_path):
    """The same clips in a fresh child process with ZAFX_COMPUTE_UNITS=1 (other segment cuts, whole clips in a batch of four)."""
    import zafx
    from maskfilter_probe import WINDOWS as PROBE_WINDOWS, probe_case
    path = str(tmp_path / "probe.npz")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maskfilter_probe.py"), path], env=dict(os.environ, ZAFX_COMPUTE_UNITS="1"),
                         capture_output=True, timeout=240)
    assert res.returncode == 0 and b"probe ok" in res.stdout, res.stderr.decode()[-2000:]
    got = np.load(path)
    for wl in PROBE_WINDOWS:
        w = zafx.hamming(wl)
        x, m = probe_case(wl)
        assert int(got[f"units{wl}"]) == 1 and zafx.maskfilter_plan(w).compute_units > 1
        here = run_plan(x[2:3], m[2:3], w)[0]
        assert np.array_equal(bits(got[f"alone{wl}"]), bits(here)) and np.array_equal(bits(got[f"batch{wl}"]), bits(here)), wl


class View:
    """`count` float32 at byte `offset` of a DeviceBuffer, to hand to execute_masked (nothing to free)."""

    def __init__(self, buf, offset, count):
        self.ptr, self.dtype, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + offset), np.dtype(np.float32), 4 * count, (count,)


@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("layout, row_align", LAYOUTS)
def test_arena(layout, row_align, rest):
    """Samples, mask and output are slices of larger buffers at bases 4 bytes off the 8-byte and the 128-byte grid; everything around them --
    in front, behind, the mask's row padding (the columns from T on of the wider pitch), the output from N on -- is NaN."""
    import zafx
    guard = 64 * 1024
    for wl, n, deltas in ((2048, 9 * 1024 + 1, (4, 132, 12)), (256, 16 * 128 - 1, (132, 4, 68)), (512, 1, (12, 68, 4))):
        w = zafx.hamming(wl)
        plan = zafx.maskfilter_plan(w, rest=rest, layout=layout, row_align=row_align)
        x = np.stack([clip(k, n) for k in range(3)])
        m = np.stack([make_mask("unit", wl, n, seed=k) for k in range(3)])
        laid = lay_out(plan, m, n)
        if layout == "FT" and row_align:
            assert np.isnan(laid).sum() == 3 * (wl // 2 + 1) * (plan.row_pitch(n) - mask_frames(n, wl)) > 0
        n_out = int(np.prod(plan.out_shape(3, n)))
        arenas, views = [], []
        for data, count, delta in ((x, x.size, deltas[0]), (laid, laid.size, deltas[1]), (None, n_out, deltas[2])):
            assert delta % 8 == 4 and delta % 128 != 0
            host = np.full((2 * guard + delta) // 4 + count, FILL, np.uint32)
            lo = (guard + delta) // 4
            if data is not None:
                host[lo:lo + count] = bits(data).ravel()
            buf = zafx.DeviceBuffer.from_host(host)
            arenas.append((buf, host, lo, count))
            views.append(View(buf, guard + delta, count))
        try:
            plan.execute_masked(views[0], views[1], views[2], 3, n)
            plan.sync()
            buf, host, lo, count = arenas[2]
            got = buf.download()
        finally:
            for a in arenas:
                a[0].free()
        assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + count:], host[lo + count:]), "written outside the output"
        out = got[lo:lo + count].view(np.float32).reshape(plan.out_shape(3, n))
        assert np.isfinite(out).all()
        for k in range(3):
            ref = oracle_maskfilter(x[k], w, m[k])
            check(out[k, 0] if rest else out[k], ref, x[k], f"arena W={wl} N={n} {layout}/{row_align} clip {k}")
            if rest:
                check(out[k, 1], x[k].astype(np.float64) - ref, x[k], f"arena rest W={wl} clip {k}")


def test_cross_check_with_the_center():
    """For the golden stereo clips: each channel's mask from the oracle's magnitudes, in the library's comparison form; maskfilter per channel
    against centersides's center (2e-5), both against one reference (1e-5)."""
    import zafx
    from center_oracle import oracle_center
    from oracle import zaf_oracle as orc
    g = np.load(os.path.join(GOLDEN, "center.npz"))
    for i in range(len([k for k in g.files if k.startswith("w")])):
        wl, n = (int(v) for v in g[f"w{i}"])
        x, w, h = g[f"x{i}"], zafx.hamming(wl), wl // 2
        s = [orc.stft(x[:, c].astype(np.float64), w, h) for c in (0, 1)]
        a, b = np.abs(s[0][:h + 1]), np.abs(s[1][:h + 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            masks = [np.where(b < a, b / a, 1.0), np.where(a < b, a / b, 1.0)]
        ref = oracle_center(x, w)
        center = zafx.centersides(x, w, h)[0]
        for c in (0, 1):
            xc = np.ascontiguousarray(x[:, c])
            m32 = masks[c].astype(np.float32)
            y = zafx.maskfilter(xc, w, h, m32)
            level = max(np.abs(ref[:, c]).max(), np.abs(xc).max())
            d = np.abs(y - center[:, c]).max() / level
            print(f"W={wl} N={n} channel {c}: maskfilter against center {d:.3e}")
            assert d <= 2e-5, (wl, c, d)
            check(y, ref[:, c], xc, f"maskfilter against the center's reference W={wl} channel {c}")
            check(center[:, c], ref[:, c], xc, f"center against its reference W={wl} channel {c}")


def test_window_replaced_on_a_used_plan():
    import windows as win
    import zafx
    for wl, n in ((2048, 20000), (256, 3001)):
        wa, wb = zafx.hamming(wl), win.skew(wl)
        x = np.stack([clip(k, n) for k in range(2)])
        m = np.stack([make_mask("unit", wl, n, seed=k) for k in range(2)])
        fresh = {}
        for tag, w in (("a", wa), ("b", wb)):
            p = zafx.Plan(zafx.MASKFILTER, window_length=wl, step_length=wl // 2)
            p.set_window(w)
            fresh[tag] = run_plan(x, m, w, plan=p)
            p.destroy()
        used = zafx.Plan(zafx.MASKFILTER, window_length=wl, step_length=wl // 2)
        for tag, w in (("a", wa), ("b", wb), ("a", wa)):
            used.set_window(w)
            y = run_plan(x, m, w, plan=used)
            assert np.array_equal(bits(y), bits(fresh[tag])), (wl, tag)
            for k in range(2):
                check(y[k], oracle_maskfilter(x[k], w, m[k]), x[k], f"window {tag} W={wl}")
        used.destroy()
        assert not np.array_equal(bits(fresh["a"]), bits(fresh["b"]))


def test_refusals_leave_the_output_untouched():
    import zafx
    from zafx import _lib
    wl, n = 512, 3000
    w = zafx.hamming(wl)
    x = clip(1, n)[None]
    sentinel = np.full((1, 2, n), -12345.5, np.float32)
    d_in, d_out = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(sentinel)
    i64p = ctypes.POINTER(ctypes.c_int64)
    lens, offs = np.array([n], np.int64), np.zeros(1, np.int64)
    pcm = np.zeros((1, 8, 1), np.int16)
    host_out = np.full((1, n), -1.0, np.float32)
    for kind_rest in (False, True):
        plan = zafx.maskfilter_plan(w, rest=kind_rest)
        d_mask = zafx.DeviceBuffer.from_host(np.ones(plan.mask_shape(1, n), np.float32))
        lib = _lib.load()
        with pytest.raises(zafx.ZafxError, match="zafx_execute_masked"):
            plan.execute(d_in, d_out, 1, n)
        with pytest.raises(zafx.ZafxError, match="zafx_execute_masked"):
            _lib.check(lib.zafx_execute_ragged(plan.handle, d_in.ptr, offs.ctypes.data_as(i64p), lens.ctypes.data_as(i64p), d_out.ptr, 1), "zafx_execute_ragged")
        with pytest.raises(zafx.ZafxError, match="zafx_execute_masked"):
            _lib.check(lib.zafx_execute_pcm(plan.handle, d_in.ptr, d_out.ptr, 1, 8, 1, 2), "zafx_execute_pcm")
        with pytest.raises(zafx.ZafxError, match="zafx_execute_masked"):
            _lib.check(lib.zafx_run_host(plan.handle, x.ctypes.data_as(ctypes.c_void_p), host_out.ctypes.data_as(ctypes.c_void_p), 1, n, 0), "zafx_run_host")
        with pytest.raises(zafx.ZafxError, match="zafx_execute_masked"):
            _lib.check(lib.zafx_run_host_pcm(plan.handle, pcm.ctypes.data_as(ctypes.c_void_p), host_out.ctypes.data_as(ctypes.c_void_p), 1, 8, 1, 2, 0), "zafx_run_host_pcm")
        assert (host_out == -1.0).all()
        # a mask array of the wrong size, through the Python layer
        short = zafx.DeviceBuffer((plan.mask_shape(1, n)[1], plan.mask_shape(1, n)[2] - 1), np.float32)
        with pytest.raises(ValueError, match="d_mask"):
            plan.execute_masked(d_in, short, d_out, 1, n)
        with pytest.raises(ValueError, match="shape"):
            zafx.maskfilter_batch(x, w, np.ones((1, wl // 2 + 1, mask_frames(n, wl) + 1), np.float32), rest=kind_rest)
        short.free(), d_mask.free()
    stft = zafx.stft_plan(w, wl // 2)
    d_mask = zafx.DeviceBuffer.from_host(np.ones((1, wl // 2 + 1, mask_frames(n, wl)), np.float32))
    with pytest.raises(zafx.ZafxError, match="MASKFILTER"):
        stft.execute_masked(d_in, d_mask, d_out, 1, n)
    dims = (ctypes.c_int64 * 2)()
    assert _lib.load().zafx_plan_mask_dims(stft.handle, n, dims) != 0 and b"MASKFILTER" in _lib.load().zafx_last_error()
    stft.sync()
    assert np.array_equal(bits(d_out.download()), bits(sentinel))
    for buf in (d_in, d_mask, d_out):
        buf.free()
