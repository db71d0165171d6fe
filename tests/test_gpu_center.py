"""Center / sides extraction on the GPU (k_center; ZAFX_CENTER, ZAFX_CENTER_SIDES): parity with the reference's composition of
zaf.stft / zaf.istft (tests/golden/center.npz) and with the oracle's at the clip lengths around the kernel's tile and segment
edges, bit-level agreement of the two kinds, independence of the clips of a batch, special signals, no writes past the end,
the host pipeline, the full-size batch and the fenced build.

Bounds: center <= 1e-5 normwise (the project's TOL_FFT for a float32 transform chain against float64), sides <= 1e-5 max|x|
absolute (sides = x - center: the same absolute error, measured against the input's level)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from center_oracle import oracle_center
from conftest import GOLDEN, ROOT, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-5
PKG = os.path.join(ROOT, "zaf-python_amd", "zafx")


def stereo(seed, n):
    g = np.random.default_rng([909, seed])
    c, n1, n2 = g.standard_normal(n), g.standard_normal(n), g.standard_normal(n)
    return np.stack([c + 0.5 * n1, 0.8 * c + 0.5 * n2], axis=1).astype(np.float32)


def check(center, sides, x, ref, what):
    e_c = relerr(np.asarray(center, np.float64), ref)
    scale = max(float(np.abs(x).max()), 1e-30)
    e_s = float(np.abs(np.asarray(sides, np.float64) - (x.astype(np.float64) - ref)).max()) / scale if sides is not None else 0.0
    print(f"{what}: center {e_c:.3e} normwise, sides {e_s:.3e} of max|x|")
    assert e_c <= TOL and e_s <= TOL, (what, e_c, e_s)


def golden_cases():
    g = np.load(os.path.join(GOLDEN, "center.npz"))
    for i in range(len([k for k in g.files if k.startswith("w")])):
        wl, n = (int(v) for v in g[f"w{i}"])
        yield wl, n, g[f"x{i}"], g[f"c{i}"]


def run_plan(x, w, sides=True):
    """The raw plan on device buffers: x (B, N, 2) -> the plan's whole output array."""
    import zafx
    plan = zafx.center_plan(w, sides=sides)
    d_in = zafx.DeviceBuffer.from_host(x)
    d_out = zafx.DeviceBuffer(plan.out_shape(x.shape[0], x.shape[1]), plan.out_dtype)
    plan.execute(d_in, d_out, x.shape[0], x.shape[1])
    plan.sync()
    assert plan.last_kernel == "k_center" and plan.kernel_name == "k_center"
    out = d_out.download()
    d_in.free(), d_out.free()
    return out


def test_golden_parity():
    import zafx
    for wl, n, x, ref in golden_cases():
        w = zafx.hamming(wl)
        c, s = zafx.centersides(x, w, wl // 2)
        assert c.dtype == np.float64 and c.shape == (n, 2) and s.shape == (n, 2)
        check(c, s, x, ref, f"centersides W={wl} N={n}")
        cb, sb = zafx.centersides_batch(x[None], w)
        assert cb.dtype == np.float32 and cb.shape == (1, n, 2) and cb.base is sb.base
        check(cb[0], sb[0], x, ref, f"centersides_batch W={wl} N={n}")
        only = zafx.centersides_batch(x[None], w, step_length=wl // 2, sides=False)
        check(only[0], None, x, ref, f"center only W={wl} N={n}")
        raw = run_plan(x[None], w)
        assert raw.shape == (1, 2, n, 2)
        check(raw[0, 0], raw[0, 1], x, ref, f"raw plan W={wl} N={n}")


@pytest.mark.parametrize("wl", [256, 512, 1024, 2048])
def test_oracle_parity_around_tile_edges(wl):
    import zafx
    w, h, f = zafx.hamming(wl), wl // 2, zafx.center_tile_frames(wl)
    assert f in (4, 8, 16)
    lengths = [1, h - 1, h, h + 1, f * h - 1, f * h, f * h + 1, 2 * f * h + 3, 44100, 123457]
    for f_alt in (8, 16):   # (the lengths of an 8- and a 16-frame tile as well, whatever the kernel's own is)
        lengths += [f_alt * h - 1, f_alt * h, f_alt * h + 1, 2 * f_alt * h + 3]
    for n in sorted(set(lengths)):
        x = stereo(n, n)
        c, s = zafx.centersides_batch(x[None], w)
        check(c[0], s[0], x, oracle_center(x, w), f"W={wl} N={n}")


def test_two_kinds_agree_bitwise():
    import zafx
    for wl, n in [(2048, 50001), (1024, 30000), (512, 9999), (256, 5000)]:
        w = zafx.hamming(wl)
        x = np.stack([stereo(7 * i + wl, n) for i in range(5)])
        both, only = run_plan(x, w, True), run_plan(x, w, False)
        assert np.array_equal(both[:, 0].view(np.uint32), only.view(np.uint32))
        assert np.array_equal(both[:, 1].view(np.uint32), (x - both[:, 0]).view(np.uint32))


def test_batch_independence():
    import zafx
    wl, n = 2048, 40000
    w = zafx.hamming(wl)
    x = np.stack([stereo(i % 30, n) for i in range(37)])   # clips 30 .. 36 repeat clips 0 .. 6
    out = run_plan(x, w)
    for i in (0, 5, 17, 36):
        assert np.array_equal(run_plan(x[i:i + 1], w)[0].view(np.uint32), out[i].view(np.uint32)), i
    for i in range(30, 37):
        assert np.array_equal(out[i].view(np.uint32), out[i - 30].view(np.uint32)), i


def test_special_signals():
    import zafx
    for wl in (2048, 512):
        w, n = zafx.hamming(wl), 30000
        c, s = zafx.centersides_batch(np.zeros((2, n, 2), np.float32), w)
        assert not c.any() and not s.any()
        m = np.random.default_rng(3).standard_normal(n).astype(np.float32)
        x = np.stack([m, m], axis=1)
        c, s = zafx.centersides_batch(x[None], w)
        assert np.isfinite(c).all() and relerr(c[0], x) <= TOL and np.abs(s).max() <= TOL * np.abs(x).max()
        x = np.stack([m, np.zeros_like(m)], axis=1)
        c, s = zafx.centersides_batch(x[None], w)
        assert np.isfinite(c).all() and np.abs(c).max() <= TOL * np.abs(x).max() and np.abs(s[0] - x).max() <= TOL * np.abs(x).max()


@pytest.mark.parametrize("sides", [False, True])
def test_no_writes_past_the_end(sides):
    import zafx
    for wl, n in [(2048, 10241), (256, 1), (1024, 512 * 9)]:
        w = zafx.hamming(wl)
        plan = zafx.center_plan(w, sides=sides)
        x = np.stack([stereo(i, n) for i in range(3)])
        shape = plan.out_shape(3, n)
        d_in = zafx.DeviceBuffer.from_host(x)
        d_out = zafx.DeviceBuffer((4,) + shape[1:], np.float32)   # one clip more than the plan writes
        sentinel = np.full(d_out.shape, -12345.5, np.float32)
        d_out.upload(sentinel)
        plan.execute(d_in, d_out, 3, n)
        plan.sync()
        got = d_out.download()
        assert np.array_equal(got[3].view(np.uint32), sentinel[3].view(np.uint32))
        assert not (got[:3] == -12345.5).any()
        d_in.free(), d_out.free()


def test_run_host_chunks_match_device_resident():
    import zafx
    wl, n = 1024, 25000
    w = zafx.hamming(wl)
    x = np.stack([stereo(i, n) for i in range(11)])
    plan = zafx.center_plan(w, sides=True)
    assert plan.clip_bytes(n) == (n * 8, n * 16) and plan.out_dims(n) == (2 * n, 2) and plan.row_pitch(n) == 2
    assert zafx.center_plan(w, sides=False).out_dims(n) == (n, 2)
    assert plan.in_dtype == np.float32 and plan.out_dtype == np.float32
    host = plan.run_host(x, n, chunk_clips=4)   # 4 + 4 + 3
    assert np.array_equal(host.view(np.uint32), run_plan(x, w).view(np.uint32))


def test_unsupported_entry_points_say_so():
    import zafx
    from zafx import _lib
    plan = zafx.center_plan(zafx.hamming(512))
    d = zafx.DeviceBuffer((64,), np.float32)
    lens = np.array([8], np.int64)
    offs = np.zeros(1, np.int64)
    with pytest.raises(zafx.ZafxError, match="center"):
        plan.execute_ragged(d, offs, lens, d)
    i64p = ctypes.POINTER(ctypes.c_int64)
    with pytest.raises(zafx.ZafxError, match="center"):
        _lib.check(_lib.load().zafx_execute_ragged(plan.handle, d.ptr, offs.ctypes.data_as(i64p), lens.ctypes.data_as(i64p), d.ptr, 1), "zafx_execute_ragged")
    with pytest.raises(zafx.ZafxError, match="center"):
        _lib.check(_lib.load().zafx_execute_pcm(plan.handle, d.ptr, d.ptr, 1, 8, 2, 2), "zafx_execute_pcm")
    pcm = np.zeros((1, 8, 2), np.int16)
    with pytest.raises(zafx.ZafxError, match="center"):
        _lib.check(_lib.load().zafx_run_host_pcm(plan.handle, pcm.ctypes.data_as(ctypes.c_void_p), d.ptr, 1, 8, 2, 2, 0), "zafx_run_host_pcm")
    d.free()


@pytest.mark.timeout(900)
def test_full_size():
    """1024 x 441 000 x 2, device-resident: 29 distinct clips repeated over the batch."""
    import zafx
    wl, n, b, distinct = 2048, 441000, 1024, 29
    w = zafx.hamming(wl)
    plan = zafx.center_plan(w, sides=True)
    try:
        d_in = zafx.DeviceBuffer((b, n, 2), np.float32)
        d_out = zafx.DeviceBuffer(plan.out_shape(b, n), np.float32)
    except zafx.ZafxError as e:
        pytest.skip(f"device allocation failed: {e}")
    x = np.stack([stereo(i, n) for i in range(distinct)])
    d_x = zafx.DeviceBuffer.from_host(x)
    clip = n * 8
    for i in range(b):
        d_in.copy_from(d_x, nbytes=clip, dst_offset=i * clip, src_offset=(i % distinct) * clip)
    plan.execute(d_in, d_out, b, n)
    plan.sync()
    for i in (0, 511, 1023):
        got = d_out.download(i, 1)[0]
        check(got[0], got[1], x[i % distinct], oracle_center(x[i % distinct], w), f"full size clip {i}")
    first = d_out.download(3, 1)[0]
    for i in range(3 + distinct, b, distinct):
        assert np.array_equal(d_out.download(i, 1)[0].view(np.uint32), first.view(np.uint32)), i
    for buf in (d_in, d_out, d_x):
        buf.free()


_PROBE = """
import sys, numpy as np
sys.path.insert(0, sys.argv[2])
import zafx
res = {}
for wl, n in [(256, 3001), (512, 9000), (1024, 20000), (2048, 50000)]:
    g = np.random.default_rng([41, wl])
    x = g.standard_normal((3, n, 2)).astype(np.float32)
    c, s = zafx.centersides_batch(x, zafx.hamming(wl))
    res[f"c{wl}"], res[f"s{wl}"] = c, s
np.savez(sys.argv[1], **res)
print(zafx.library_path())
"""


@pytest.mark.timeout(600)
def test_fenced_build_is_bit_identical(tmp_path):
    fence = os.path.join(PKG, "libzafx_fence.so")
    if not os.path.exists(fence):
        subprocess.run(["make", "-C", os.path.join(ROOT, "zaf-python_amd", "csrc"), "fence", "-j", "8"], check=True, stdout=subprocess.DEVNULL)
    outs = {}
    for tag, lib in (("default", os.path.join(PKG, "libzafx.so")), ("fence", fence)):
        path = str(tmp_path / f"{tag}.npz")
        res = subprocess.run([sys.executable, "-c", _PROBE, path, os.path.join(ROOT, "zaf-python_amd")], env=dict(os.environ, ZAFX_LIBRARY=lib),
                             capture_output=True, timeout=280)
        assert res.returncode == 0, res.stderr.decode()[-2000:]
        assert os.path.basename(lib) in res.stdout.decode()
        outs[tag] = np.load(path)
    assert sorted(outs["default"].files) == sorted(outs["fence"].files) and len(outs["default"].files) == 8
    for key in outs["default"].files:
        a, b = outs["default"][key], outs["fence"][key]
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a).all(), key
