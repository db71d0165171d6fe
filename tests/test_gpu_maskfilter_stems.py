"""Mask filter stems on the GPU (k_maskfilter_stems; zafx_execute_masked_stems): S masks per clip over one forward transform.  Stem s of every
clip is held BIT FOR BIT to execute_masked on a "TF" plan with that mask alone and the rest to the float32 subtraction chain of the
downloaded stems; on top of that parity with the float64 oracle, masks that sum to one, the fixed values, independence of the segment cut,
the place in the batch and the compute-unit count, arrays inside larger buffers with NaN guards, the one-mask kind after the new one on
the same plan, a window replaced on a used plan, and the refusals.

Bounds: bit identity; against the oracle max|y - ref| <= 1e-5 max(max|ref|, max|x|) per stem (TOL_FFT at mask_error's level, as
tests/test_gpu_maskfilter.py); for S masks that sum to one the per-stem bound added up, S * TOL_FFT of max|x|, for the sum of the stems
against x and for the rest against 0.  F is the number of packed transforms per tile, so a tile is 2 F frames."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from maskfilter_oracle import TOL_FFT, make_mask, mask_error, mask_frames, oracle_maskfilter

pytestmark = pytest.mark.gpu

WINDOWS = (256, 512, 1024, 2048)
STEMS = (1, 2, 3, 8)
FILL = 0x7FC5A5A5   # a quiet NaN no kernel computes


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clip(seed, n):
    return np.random.default_rng([404, seed, n]).standard_normal(n).astype(np.float32)


def lengths(wl):
    """The pair and tile edges, both parities of the frame count."""
    import zafx
    h, f = wl // 2, zafx.maskfilter_tile_transforms(wl)
    return [1, h, 2 * h + 1, 2 * f * h - 1, 2 * f * h, 2 * f * h + 1, 4 * f * h + 3]


def tf(m):
    """Masks (..., W/2 + 1, T) -> (..., T, W/2 + 1), contiguous float32."""
    return np.ascontiguousarray(np.swapaxes(m, -1, -2), np.float32)


def chain(x, y):
    """((x - y_0) - y_1) - ... in float32, left to right; x (B, N), y (B, S, N)."""
    r = np.asarray(x, np.float32).copy()
    for s in range(y.shape[1]):
        r = r - y[:, s]
    assert r.dtype == np.float32
    return r


def run_stems(x, m, w, rest=False, plan=None):
    """The raw plan on device buffers: x (B, N), m (B, S, T, W/2 + 1) -> the plan's whole output array, (B, S [+ 1], N)."""
    import zafx
    plan = plan or zafx.maskfilter_plan(w, rest=rest, layout="TF")
    b, n = x.shape
    s = m.shape[1]
    assert m.shape == plan.stems_mask_shape(b, n, s), (m.shape, plan.stems_mask_shape(b, n, s))
    d_in, d_mask = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(m)
    d_out = zafx.DeviceBuffer(plan.stems_out_shape(b, n, s), np.float32)
    try:
        plan.execute_masked_stems(d_in, d_mask, d_out, b, n, s)
        plan.sync()
        assert plan.last_kernel == "k_maskfilter_stems"
        return d_out.download()
    finally:
        for buf in (d_in, d_mask, d_out):
            buf.free()


def run_single(x, m, w, rest=False, plan=None):
    """execute_masked on a "TF" plan: x (B, N), m (B, T, W/2 + 1) -> (B, N) or (B, 2, N)."""
    import zafx
    plan = plan or zafx.maskfilter_plan(w, rest=rest, layout="TF")
    b, n = x.shape
    d_in, d_mask = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(m)
    d_out = zafx.DeviceBuffer(plan.out_shape(b, n), np.float32)
    try:
        plan.execute_masked(d_in, d_mask, d_out, b, n)
        plan.sync()
        assert plan.last_kernel == "k_maskfilter"
        return d_out.download()
    finally:
        for buf in (d_in, d_mask, d_out):
            buf.free()


def singles(x, m, w):
    """Every (clip, stem) as a clip of its own under the one-mask kind, in one launch: x (B, N), m (B, S, T, W/2 + 1) -> (B, S, N)."""
    b, s = m.shape[:2]
    return run_single(np.repeat(x, s, axis=0), m.reshape((b * s,) + m.shape[2:]), w).reshape(b, s, x.shape[1])


@pytest.fixture(scope="module")
def cases():
    """Per W: [(N, x (3, N), masks (3, 8, T, W/2 + 1) "unit" -- stem 1 "signed_wide", uniform in [-2, 2] -- with a seed per (clip, stem), refs (3, 8, N) float64, one (3, 8, N): the one-mask
    kind's bits)]; S stems are the first S masks.  The oracle and the one-mask kind run once."""
    import zafx
    out = {}
    for wl in WINDOWS:
        w = zafx.hamming(wl)
        out[wl] = []
        for n in lengths(wl):
            x = np.stack([clip(k, n) for k in range(3)])
            m = np.stack([np.stack([make_mask("signed_wide" if s == 1 else "unit", wl, n, seed=10 * k + s) for s in range(8)]) for k in range(3)])
            refs = np.stack([np.stack([oracle_maskfilter(x[k], w, m[k, s]) for s in range(8)]) for k in range(3)])
            mt = tf(m)
            out[wl].append((n, x, mt, refs, singles(x, mt, w)))
    return out


@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("wl", WINDOWS)
def test_stems_have_the_bits_of_the_single_mask_kind(cases, wl, rest):
    import zafx
    w = zafx.hamming(wl)
    worst = 0.0
    for n, x, m, refs, one in cases[wl]:
        for s in STEMS:
            out = run_stems(x, m[:, :s], w, rest)
            assert out.shape == (3, s + int(rest), n)
            for k in range(3):
                for j in range(s):
                    assert np.array_equal(bits(out[k, j]), bits(one[k, j])), (wl, n, s, rest, k, j)
                    err = mask_error(out[k, j], refs[k, j], x[k])
                    worst = max(worst, err)
                    assert err <= TOL_FFT, (wl, n, s, k, j, err)
            if rest:
                assert np.array_equal(bits(out[:, s]), bits(chain(x, out[:, :s]))), (wl, n, s, "rest")
    print(f"W={wl} rest={rest}: worst error against the oracle {worst:.3e} of the level")


@pytest.mark.parametrize("wl", WINDOWS)
def test_masks_that_sum_to_one(wl):
    """Hamming at H = W/2 is COLA: S masks that sum to one in every bin return the clip between them and leave no rest."""
    import zafx
    w = zafx.hamming(wl)
    n = 9 * wl + 5
    x = np.stack([clip(k, n) for k in range(2)])
    for s in (2, 4, 8):
        r = np.random.default_rng([5, wl, s]).random((2, s, mask_frames(n, wl), wl // 2 + 1)) + 0.05
        m = (r / r.sum(axis=1, keepdims=True)).astype(np.float32)
        out = run_stems(x, m, w, True)
        for k in range(2):
            level = np.abs(x[k]).max()
            total = np.abs(out[k, :s].astype(np.float64).sum(axis=0) - x[k]).max() / level
            left = np.abs(out[k, s]).max() / level
            print(f"W={wl} S={s} clip {k}: sum of the stems {total:.3e}, rest {left:.3e} of the level (bound {s * TOL_FFT:.0e})")
            assert total <= s * TOL_FFT and left <= s * TOL_FFT, (wl, s, k, total, left)


def test_fixed_values():
    """A stem of zeros is exact zeros while its neighbours keep their bits; silence under wild finite masks is all zeros."""
    import zafx
    for wl in (2048, 256):
        w, n = zafx.hamming(wl), 7 * wl + 3
        x = np.stack([clip(k, n) for k in range(2)])
        t = mask_frames(n, wl)
        m = tf(np.stack([np.stack([make_mask("unit", wl, n, seed=10 * k + s) for s in range(3)]) for k in range(2)]))
        full = run_stems(x, m, w, True)
        m0 = m.copy()
        m0[:, 1] = 0
        out = run_stems(x, m0, w, True)
        assert not out[:, 1].any()
        assert np.array_equal(bits(out[:, 0]), bits(full[:, 0])) and np.array_equal(bits(out[:, 2]), bits(full[:, 2]))
        assert np.array_equal(bits(out[:, 3]), bits(chain(x, out[:, :3])))
        wild = (np.random.default_rng(wl).random((2, 3, t, wl // 2 + 1)) * 2e30 - 1e30).astype(np.float32)
        assert not run_stems(np.zeros_like(x), wild, w, True).any()
        bad = x.copy()
        bad[0, n // 2] = np.nan   # a non-finite value stays within its own clip
        out = run_stems(bad, m, w, True)
        assert np.isnan(out[0]).any() and np.array_equal(bits(out[1]), bits(full[1]))


def touched(n, h, frames):
    """The samples of a clip of n that frames `frames` reach, partners included: frames 2j and 2j + 1 share a transform, frame t covers
    samples (t - 1) H .. (t + 1) H - 1."""
    hit = np.zeros(n, bool)
    for t in frames:
        for u in (t, t ^ 1):
            hit[max((u - 1) * h, 0):min((u + 1) * h, n)] = True
    return hit


def containment_case(wl):
    """-> (h, n, x (3, N), masks (3, 3, T, W/2 + 1) "unit")."""
    h = wl // 2
    n = 20 * h + 9
    x = np.stack([clip(30 + k, n) for k in range(3)])
    return h, n, x, tf(np.stack([np.stack([make_mask("unit", wl, n, seed=10 * (30 + k) + j) for j in range(3)]) for k in range(3)]))


@pytest.mark.parametrize("wl", [256, 2048])
def test_containment(wl):
    """A NaN sample in clip 1 of three and a NaN in the mask of its stem 0, with the rest: clips 0 and 2 have the bits of their runs alone and of
    the clean batch; inside clip 1 only the samples of the frames that hold the NaN sample or mask value, and of the frames paired with them,
    may be non-finite, in any stem or the rest -- every other sample has the bits of the clean run."""
    import zafx
    w = zafx.hamming(wl)
    h, n, x, m = containment_case(wl)
    clean = run_stems(x, m, w, True)
    s, (k, t) = 5 * h + 17, (h // 3, 13)   # sample s lies in frames 5 and 6; the mask value in frame 13
    xp, mp = x.copy(), m.copy()
    xp[1, s] = np.nan
    mp[1, 0, t, k] = np.nan
    got = run_stems(xp, mp, w, True)
    for c in (0, 2):
        assert np.array_equal(bits(got[c]), bits(run_stems(x[c:c + 1], m[c:c + 1], w, True)[0])) and np.array_equal(bits(got[c]), bits(clean[c])), (wl, c)
    may = touched(n, h, [s // h, s // h + 1, t])
    assert 0 < may.sum() < n
    for j in range(4):
        assert not np.isfinite(got[1, j][may]).all() and np.isfinite(got[1, j][~may]).all(), (wl, j)
        assert np.array_equal(bits(got[1, j][~may]), bits(clean[1, j][~may])), (wl, j)


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("wl", [256, 2048])
def test_a_stem_s_mask_stays_out_of_the_other_stems(wl, bad):
    """The stems share ONE forward transform.  A NaN, then +inf, in the mask of stem 1 of clip 1 alone: stems 0 and 2 of every clip have the bits
    of the clean run everywhere; stem 1 and the rest are non-finite only in the samples of that frame and of its partner."""
    import zafx
    w = zafx.hamming(wl)
    h, n, x, m = containment_case(wl)
    clean = run_stems(x, m, w, True)
    k, t = h // 3, 13
    mp = m.copy()
    mp[1, 1, t, k] = bad
    got = run_stems(x, mp, w, True)
    for c in (0, 2):
        assert np.array_equal(bits(got[c]), bits(clean[c])), (wl, c)
    for j in (0, 2):
        assert np.array_equal(bits(got[1, j]), bits(clean[1, j])), (wl, "stem", j)
    may = touched(n, h, [t])
    assert 0 < may.sum() < n
    for j in (1, 3):
        assert not np.isfinite(got[1, j][may]).all() and np.isfinite(got[1, j][~may]).all(), (wl, j)
        assert np.array_equal(bits(got[1, j][~may]), bits(clean[1, j][~may])), (wl, j)


def test_segments_give_the_bits_of_whole_clips():
    """The 60-block clip with three stems alone is cut into segments; in a batch of four clips per compute unit the clips stay whole."""
    import zafx
    from maskfilter_stems_probe import stems_case
    wl = 256
    w = zafx.hamming(wl)
    x, m = stems_case(wl)
    plan = zafx.maskfilter_plan(w, layout="TF")
    clips = 4 * plan.compute_units   # (at most four workgroups of k_maskfilter_stems share a compute unit)
    for rest in (False, True):
        alone = run_stems(x[2:3], m[2:3], w, rest)[0]
        idx = np.arange(clips) % 4
        whole = run_stems(x[idx], m[idx], w, rest)
        for i in (2, clips - 2):
            assert idx[i] == 2 and np.array_equal(bits(whole[i]), bits(alone)), (i, rest)
        assert np.array_equal(bits(alone[:3]), bits(singles(x[2:3], m[2:3], w)[0]))


@pytest.mark.timeout(300)
def test_one_compute_unit_gives_the_same_bits(tmp_path):
    """The same clips in a fresh child process with ZAFX_COMPUTE_UNITS=1 (other segment cuts, whole clips in a batch of four)."""
    import zafx
    from maskfilter_stems_probe import WINDOWS as PROBE_WINDOWS, stems_case
    path = str(tmp_path / "probe.npz")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maskfilter_stems_probe.py"), path], env=dict(os.environ, ZAFX_COMPUTE_UNITS="1"),
                         capture_output=True, timeout=240)
    assert res.returncode == 0 and b"probe ok" in res.stdout, res.stderr.decode()[-2000:]
    got = np.load(path)
    for wl in PROBE_WINDOWS:
        w = zafx.hamming(wl)
        x, m = stems_case(wl)
        assert int(got[f"units{wl}"]) == 1 and zafx.maskfilter_plan(w, layout="TF").compute_units > 1
        for rest, tag in ((False, f"{wl}"), (True, f"{wl}r")):
            here = run_stems(x[2:3], m[2:3], w, rest)[0]
            assert np.array_equal(bits(got[f"alone{tag}"]), bits(here)) and np.array_equal(bits(got[f"batch{tag}"]), bits(here)), (wl, rest)


class View:
    """`count` float32 at byte `offset` of a DeviceBuffer, to hand to execute_masked_stems (nothing to free)."""

    def __init__(self, buf, offset, count):
        self.ptr, self.dtype, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + offset), np.dtype(np.float32), 4 * count, (count,)


@pytest.mark.parametrize("rest", [False, True])
def test_arena(rest):
    """Samples, masks and output are slices of larger buffers at bases 4 bytes off the 8-byte and the 128-byte grid; everything around them is
    NaN.  Every word outside the output is unchanged, every word inside is finite and within the bound."""
    import zafx
    guard, s = 64 * 1024, 3
    for wl, n, deltas in ((2048, 9 * 1024 + 1, (4, 132, 12)), (256, 16 * 128 - 1, (132, 4, 68)), (512, 1, (12, 68, 4))):
        w = zafx.hamming(wl)
        plan = zafx.maskfilter_plan(w, rest=rest, layout="TF")
        x = np.stack([clip(k, n) for k in range(3)])
        m = np.stack([np.stack([make_mask("unit", wl, n, seed=10 * k + j) for j in range(s)]) for k in range(3)])
        laid = tf(m)
        shape = plan.stems_out_shape(3, n, s)
        n_out = int(np.prod(shape))
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
            plan.execute_masked_stems(views[0], views[1], views[2], 3, n, s)
            plan.sync()
            buf, host, lo, count = arenas[2]
            got = buf.download()
        finally:
            for a in arenas:
                a[0].free()
        assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + count:], host[lo + count:]), "written outside the output"
        out = got[lo:lo + count].view(np.float32).reshape(shape)
        assert np.isfinite(out).all()
        for k in range(3):
            rem = x[k].astype(np.float64)
            for j in range(s):
                ref = oracle_maskfilter(x[k], w, m[k, j])
                rem = rem - ref
                err = mask_error(out[k, j], ref, x[k])
                assert err <= TOL_FFT, (wl, n, k, j, err)
            if rest:   # the per-stem bound added up
                assert np.abs(out[k, s] - rem).max() <= s * TOL_FFT * np.abs(x[k]).max(), (wl, n, k, "rest")


def test_the_single_mask_kind_after_the_stems_on_one_plan():
    import zafx
    for wl, n in ((2048, 20000), (256, 3001)):
        w = zafx.hamming(wl)
        x = np.stack([clip(k, n) for k in range(2)])
        m = tf(np.stack([np.stack([make_mask("unit", wl, n, seed=10 * k + s) for s in range(3)]) for k in range(2)]))
        for rest in (False, True):
            kind = zafx.MASKFILTER_REST if rest else zafx.MASKFILTER
            fresh = zafx.Plan(kind, window_length=wl, step_length=wl // 2, layout="TF")
            fresh.set_window(w)
            want = run_single(x, m[:, 1], w, plan=fresh)
            fresh.destroy()
            used = zafx.Plan(kind, window_length=wl, step_length=wl // 2, layout="TF")
            used.set_window(w)
            stems = run_stems(x, m, w, plan=used)
            got = run_single(x, m[:, 1], w, plan=used)
            assert used.last_kernel == "k_maskfilter" and used.kernel_name == "k_maskfilter"
            assert np.array_equal(bits(got), bits(want)), (wl, rest)
            assert np.array_equal(bits(stems[:, 1]), bits(want[:, 0] if rest else want)), (wl, rest)
            used.destroy()


def test_window_replaced_on_a_used_plan():
    import windows as win
    import zafx
    for wl, n in ((2048, 20000), (256, 3001)):
        wa, wb = zafx.hamming(wl), win.skew(wl)
        x = np.stack([clip(k, n) for k in range(2)])
        m = tf(np.stack([np.stack([make_mask("unit", wl, n, seed=10 * k + s) for s in range(3)]) for k in range(2)]))
        fresh = {}
        for tag, w in (("a", wa), ("b", wb)):
            p = zafx.Plan(zafx.MASKFILTER_REST, window_length=wl, step_length=wl // 2, layout="TF")
            p.set_window(w)
            fresh[tag] = run_stems(x, m, w, plan=p)
            p.destroy()
        used = zafx.Plan(zafx.MASKFILTER_REST, window_length=wl, step_length=wl // 2, layout="TF")
        for tag, w in (("a", wa), ("b", wb), ("a", wa)):
            used.set_window(w)
            assert np.array_equal(bits(run_stems(x, m, w, plan=used)), bits(fresh[tag])), (wl, tag)
        used.destroy()
        assert not np.array_equal(bits(fresh["a"]), bits(fresh["b"]))
        for k in range(2):
            assert mask_error(fresh["b"][k, 2], oracle_maskfilter(x[k], wb, m[k, 2].T), x[k]) <= TOL_FFT


def test_refusals_leave_the_output_untouched():
    import zafx
    from zafx import _lib
    wl, n, s = 512, 3000, 2
    w = zafx.hamming(wl)
    x = clip(1, n)[None]
    sentinel = np.full((1, s + 1, n), -12345.5, np.float32)
    d_in, d_out = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(sentinel)
    lib = _lib.load()
    for rest in (False, True):
        plan = zafx.maskfilter_plan(w, rest=rest, layout="TF")
        d_mask = zafx.DeviceBuffer.from_host(np.ones(plan.stems_mask_shape(1, n, s), np.float32))
        for stems in (0, 9):
            with pytest.raises(zafx.ZafxError, match="n_stems"):
                plan.execute_masked_stems(d_in, d_mask, d_out, 1, n, stems)
        with pytest.raises(zafx.ZafxError, match="2\\^28"):   # on small buffers: refused before anything is read
            _lib.check(lib.zafx_execute_masked_stems(plan.handle, d_in.ptr, d_mask.ptr, d_out.ptr, 1, 1 << 28, s), "zafx_execute_masked_stems")
        # a mask array of the wrong size, through the Python layer
        short = zafx.DeviceBuffer((1, s, plan.mask_dims(n)[1] - 1, wl // 2 + 1), np.float32)
        with pytest.raises(ValueError, match="d_mask"):
            plan.execute_masked_stems(d_in, short, d_out, 1, n, s)
        with pytest.raises(ValueError, match="d_mask"):
            plan.execute_masked_stems(d_in, d_mask, d_out, 1, n, s + 1)
        with pytest.raises(ValueError, match="shape"):
            zafx.maskfilter_stems_batch(x, w, np.ones((1, s, wl // 2 + 1, mask_frames(n, wl) + 1), np.float32), rest=rest)
        ft = zafx.maskfilter_plan(w, rest=rest, layout="FT")
        with pytest.raises(zafx.ZafxError, match="ZAFX_LAYOUT_TF"):
            ft.execute_masked_stems(d_in, d_mask, d_out, 1, n, s)
        ft.sync(), plan.sync()
        short.free(), d_mask.free()
    stft = zafx.stft_plan(w, wl // 2)
    d_mask = zafx.DeviceBuffer.from_host(np.ones((1, s, mask_frames(n, wl), wl // 2 + 1), np.float32))
    with pytest.raises(zafx.ZafxError, match="MASKFILTER"):
        stft.execute_masked_stems(d_in, d_mask, d_out, 1, n, s)
    stft.sync()
    assert np.array_equal(bits(d_out.download()), bits(sentinel))
    for buf in (d_in, d_mask, d_out):
        buf.free()


def test_host_functions():
    """maskfilter_stems_batch in both mask layouts and with `out`, and the drop-in form, against maskfilter_batch per stem."""
    import zafx
    wl, n, s = 1024, 7001, 4
    w = zafx.hamming(wl)
    x = np.stack([clip(k, n) for k in range(2)])
    m = np.stack([np.stack([make_mask("unit", wl, n, seed=10 * k + j) for j in range(s)]) for k in range(2)])
    y = zafx.maskfilter_stems_batch(x, w, m)
    assert y.dtype == np.float32 and y.shape == (2, s, n)
    for j in range(s):
        assert np.array_equal(bits(y[:, j]), bits(zafx.maskfilter_batch(x, w, tf(m[:, j]), layout="TF"))), j
    buf = np.empty((2, s + 1, n), np.float32)
    ys, r = zafx.maskfilter_stems_batch(x, w, tf(m), step_length=wl // 2, rest=True, layout="TF", out=buf)
    assert ys.base is buf and r.base is buf and ys.shape == (2, s, n) and r.shape == (2, n)
    assert np.array_equal(bits(ys), bits(y)) and np.array_equal(bits(r), bits(chain(x, ys)))
    d = zafx.maskfilter_stems(x[0].astype(np.float64), w, wl // 2, m[0])
    assert d.dtype == np.float64 and d.shape == (s, n) and np.array_equal(d, y[0].astype(np.float64))
