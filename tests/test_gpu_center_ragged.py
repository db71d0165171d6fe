"""Ragged stereo batches of the center / sides extraction on the GPU (k_center's RAGGED form; zafx_execute_center_ragged,
centersides_ragged): every clip of a batch has the bits the equal-length launch gives for that clip alone -- at the lengths around the
kernel's tile and segment edges, with clips packed back to back, for clips cut into many segments and for more units than workgroups --,
parity with the reference's composition (tests/golden/center.npz), no write outside the clips' blocks, independence of the order of the
clips, two calls enqueued back to back, and the errors the entry point reports.

Bounds of the parity test: center <= 1e-5 normwise, sides <= 1e-5 of max|x| -- those tests/test_gpu_center.py holds the equal-length kernel
to on the same inputs."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5
NAME = "k_center_ragged"


def stereo(seed, n):
    g = np.random.default_rng([909, seed])
    c, n1, n2 = g.standard_normal(n), g.standard_normal(n), g.standard_normal(n)
    return np.stack([c + 0.5 * n1, 0.8 * c + 0.5 * n2], axis=1).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_SOLO = {}


def solo(x, w, key):
    """(center, sides) of one clip alone through the equal-length launch; computed once per (window, clip) and shared."""
    import zafx
    if key not in _SOLO:
        if len(x) == 0:
            _SOLO[key] = (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
        else:
            c, s = zafx.centersides_batch(x[None], w)
            _SOLO[key] = (c[0].copy(), s[0].copy())
    return _SOLO[key]


def last_kernel(w, sides):
    import zafx
    return zafx.center_plan(w, sides=sides).last_kernel


def run_ragged(clips, w, sides):
    import zafx
    res = zafx.centersides_ragged(clips, w, sides=sides)
    assert last_kernel(w, sides) == NAME
    assert len(res) == len(clips)
    return res


def assert_bitwise(clips, keys, w, sides):
    res = run_ragged(clips, w, sides)
    for i, (x, key) in enumerate(zip(clips, keys)):
        c_ref, s_ref = solo(x, w, key)
        c = res[i][0] if sides else res[i]
        assert c.dtype == np.float32 and c.shape == x.shape, (i, c.shape)
        assert np.array_equal(bits(c), bits(c_ref)), (key, "center")
        if sides:
            assert res[i][1].shape == x.shape and np.array_equal(bits(res[i][1]), bits(s_ref)), (key, "sides")


@pytest.mark.parametrize("sides", [False, True])
@pytest.mark.parametrize("wl", [256, 512, 1024, 2048])
def test_bitwise_against_the_clip_alone(wl, sides):
    import zafx
    w, h, f = zafx.hamming(wl), wl // 2, zafx.center_tile_frames(wl)
    lengths = [0, 1, h - 1, h, h + 1, f * h - 1, f * h, f * h + 1, (2 * f - 1) * h, 2 * f * h + 3, 44100]
    clips = [stereo(n, n) for n in lengths]   # packed back to back: a clip's neighbour lies right behind it
    assert_bitwise(clips, [(wl, n) for n in lengths], w, sides)
    res = run_ragged(clips, w, sides)
    views = [r[0] for r in res] if sides else res
    assert all(v.base is views[0].base for v in views)   # views of the one result buffer


@pytest.mark.parametrize("sides", [False, True])
def test_cut_clips_and_more_units_than_workgroups(sides):
    import zafx
    wl = 256
    w, h = zafx.hamming(wl), wl // 2
    # few clips: the long one is cut into many segments
    lengths = [300_000, 5_000]
    assert_bitwise([stereo(n, n) for n in lengths], [(wl, n) for n in lengths], w, sides)
    # 600 clips of 1 .. 3H sample frames: more units than workgroups
    rng = np.random.default_rng(17)
    lengths = rng.integers(1, 3 * h + 1, 600).tolist()
    lengths[:6] = [1, h, h + 1, 2 * h, 2 * h + 1, 3 * h]
    assert_bitwise([stereo(n, n) for n in lengths], [(wl, n) for n in lengths], w, sides)


def golden_cases():
    g = np.load(os.path.join(GOLDEN, "center.npz"))
    for i in range(len([k for k in g.files if k.startswith("w")])):
        wl, n = (int(v) for v in g[f"w{i}"])
        yield wl, n, g[f"x{i}"], g[f"c{i}"]


def test_oracle_parity_on_the_golden_cases():
    import zafx
    cases = list(golden_cases())
    for wl in sorted({c[0] for c in cases}):
        mine = [c for c in cases if c[0] == wl]
        w = zafx.hamming(wl)
        res = run_ragged([c[2] for c in mine], w, True)   # all cases of this window in one ragged batch
        for (_, n, x, ref), (center, sides) in zip(mine, res):
            e_c = relerr(np.asarray(center, np.float64), ref)
            scale = max(float(np.abs(x).max()), 1e-30)
            e_s = float(np.abs(np.asarray(sides, np.float64) - (x.astype(np.float64) - ref)).max()) / scale if n else 0.0
            print(f"W={wl} N={n}: center {e_c:.3e} normwise, sides {e_s:.3e} of max|x|")
            assert e_c <= TOL and e_s <= TOL, (wl, n, e_c, e_s)


@pytest.mark.parametrize("sides", [False, True])
def test_writes_nothing_but_the_clips(sides):
    """Gaps between the blocks and a tail, offsets that are no multiples of 16 sample frames (only the 8-byte alignment holds), a zero-length
    clip in the middle: every sample frame of every block is written, every other one keeps the sentinel bit for bit."""
    import zafx
    blocks = 2 if sides else 1
    for wl, lengths in [(2048, [10241, 0, 1, 4096, 3000]), (256, [1, 127, 129, 5000, 40000])]:
        w = zafx.hamming(wl)
        plan = zafx.center_plan(w, sides=sides)
        clips = [stereo(100 + i, n) for i, n in enumerate(lengths)]
        in_offsets, out_offsets, at_in, at_out = [], [], 3, 5
        for i, n in enumerate(lengths):
            in_offsets.append(at_in)
            out_offsets.append(at_out)
            at_in += n + (1, 7, 0, 13, 2)[i]            # odd gaps: offsets off every grid but the sample frame's
            at_out += blocks * n + (9, 3, 1, 21, 6)[i]
        assert any(o % 16 for o in in_offsets) and any(o % 16 for o in out_offsets)
        x = np.full((at_in + 11, 2), 7.25, np.float32)   # what lies between the clips is loud: read as a clip's tail it would show
        for c, o in zip(clips, in_offsets):
            x[o:o + len(c)] = c
        sentinel = np.full((at_out + 50, 2), -12345.5, np.float32)
        d_in = zafx.DeviceBuffer.from_host(x)
        d_out = zafx.DeviceBuffer(sentinel.shape, np.float32).upload(sentinel)
        plan.execute_center_ragged(d_in, in_offsets, lengths, d_out, out_offsets)
        plan.sync()
        assert plan.last_kernel == NAME
        got = d_out.download()
        d_in.free(), d_out.free()
        inside = np.zeros(len(got), bool)
        for i, (c, o, n) in enumerate(zip(clips, out_offsets, lengths)):
            assert not inside[o:o + blocks * n].any()
            inside[o:o + blocks * n] = True
            c_ref, s_ref = solo(c, w, (wl, "gap", i, n))
            assert np.array_equal(bits(got[o:o + n]), bits(c_ref)), (wl, i)
            if sides:
                assert np.array_equal(bits(got[o + n:o + 2 * n]), bits(s_ref)), (wl, i)
        assert not (got[inside] == -12345.5).any()
        assert np.array_equal(bits(got[~inside]), bits(sentinel[~inside]))


def test_permutation_of_the_clips():
    import zafx
    wl = 1024
    w = zafx.hamming(wl)
    lengths = [30000, 1, 511, 512, 513, 70001, 4096, 0, 12345, 100000]
    clips = [stereo(200 + i, n) for i, n in enumerate(lengths)]
    order = np.random.default_rng(3).permutation(len(clips)).tolist()
    a = run_ragged(clips, w, True)
    b = run_ragged([clips[i] for i in order], w, True)
    for j, i in enumerate(order):
        assert np.array_equal(bits(a[i][0]), bits(b[j][0])) and np.array_equal(bits(a[i][1]), bits(b[j][1])), i


def test_back_to_back_calls_each_see_their_own_table():
    import zafx
    wl = 512
    w = zafx.hamming(wl)
    plan = zafx.center_plan(w, sides=True)
    batches = [[20000, 300, 7777, 1], [5, 64000, 0, 2049, 900, 15000, 256]]
    state = []
    for k, lengths in enumerate(batches):
        clips = [stereo(300 + 10 * k + i, n) for i, n in enumerate(lengths)]
        x, in_offsets, lens = zafx.pack_ragged_stereo(clips)
        d_in = zafx.DeviceBuffer.from_host(x)
        d_out = zafx.DeviceBuffer((2 * len(x), 2), np.float32)
        d_out.fill_zero()
        state.append((clips, in_offsets, lens, d_in, d_out))
    for clips, in_offsets, lens, d_in, d_out in state:   # no sync between the two calls
        plan.execute_center_ragged(d_in, in_offsets, lens, d_out, 2 * in_offsets)
    plan.sync()
    assert plan.last_kernel == NAME
    for k, (clips, in_offsets, lens, d_in, d_out) in enumerate(state):
        got = d_out.download()
        d_in.free(), d_out.free()
        for i, (c, o, n) in enumerate(zip(clips, (2 * in_offsets).tolist(), lens.tolist())):
            c_ref, s_ref = solo(c, w, (wl, "b2b", k, i))
            assert np.array_equal(bits(got[o:o + n]), bits(c_ref)) and np.array_equal(bits(got[o + n:o + 2 * n]), bits(s_ref)), (k, i)


def test_errors_are_reported():
    import zafx
    from zafx import _lib
    w = zafx.hamming(512)
    plan = zafx.center_plan(w)
    d = zafx.DeviceBuffer((4096, 2), np.float32)
    ok = [0, 100]
    with pytest.raises(zafx.ZafxError, match="negative length or offset of clip 1"):
        plan.execute_center_ragged(d, ok, [10, -1], d, ok)
    with pytest.raises(zafx.ZafxError, match="negative length or offset of clip 0"):
        plan.execute_center_ragged(d, [-4, 100], [10, 10], d, ok)
    with pytest.raises(zafx.ZafxError, match="negative length or offset of clip 1"):
        plan.execute_center_ragged(d, ok, [10, 10], d, [0, -100])
    i64p = ctypes.POINTER(ctypes.c_int64)

    def raw(handle, offs, lens, outs, n=None):
        offs, lens, outs = (np.asarray(v, np.int64) for v in (offs, lens, outs))
        return _lib.load().zafx_execute_center_ragged(handle, d.ptr, offs.ctypes.data_as(i64p), lens.ctypes.data_as(i64p), d.ptr, outs.ctypes.data_as(i64p),
                                                      len(lens) if n is None else n)
    with pytest.raises(zafx.ZafxError, match="2\\^28"):
        _lib.check(raw(plan.handle, [0], [1 << 28], [0]), "zafx_execute_center_ragged")
    with pytest.raises(zafx.ZafxError, match="negative number of clips"):
        _lib.check(raw(plan.handle, [0], [8], [0], n=-1), "zafx_execute_center_ragged")
    other = zafx.stft_plan(w, 256)
    with pytest.raises(zafx.ZafxError, match="ZAFX_CENTER"):
        other.execute_center_ragged(d, [0], [8], d, [0])
    with pytest.raises(zafx.ZafxError, match="ZAFX_CENTER"):
        _lib.check(raw(other.handle, [0], [8], [0]), "zafx_execute_center_ragged")
    # and a good call still goes through afterwards
    plan.execute_center_ragged(d, [0], [8], d, [2000])
    plan.sync()
    assert plan.last_kernel == NAME
    d.free()
