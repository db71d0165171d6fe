"""Ragged batches of the IMDCT on the GPU (-m gpu): coefficient blocks of different frame counts in one launch of k_imdct's RAGGED form
(zafx.imdct_ragged, Plan.execute_imdct_ragged, zafx_execute_imdct_ragged) -- against the CPU oracle, bit for bit against every block alone on
the same plan, and on the routes that stay on one execute per clip.  A tile is 32 frames of one clip: the frame counts sit around whole
tiles."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr
from oracle import zaf_oracle as orc

pytestmark = pytest.mark.gpu

TOL_IMDCT = 1e-5       # the IMDCT against the float64 oracle
TOL_F64 = 1e-12        # the float64 kernels
TOL_ROUND_TRIP = 1e-5  # |imdct(mdct(x)) - x| on unit-variance noise, absolute
NATIVE = "k_imdct_ragged"
WINDOWS = [512, 1024, 2048]
FRAMES = [1, 2, 3, 31, 32, 33, 34, 63, 64, 65, 97, 130]


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    return z


def frames_for(w, seed=1):
    return FRAMES + np.random.default_rng([seed, w]).integers(1, 200, 4).tolist()


def noise_blocks(w, frames, seed):
    return [np.random.default_rng([seed, w, i]).standard_normal((w // 2, t)).astype(np.float32) for i, t in enumerate(frames)]


def out_len(w, t):
    return max((w // 2) * (t - 1) - 1, 0)


def grid_plan(zafx, window):
    return zafx.mdct_plan(window, inverse=True, row_align=32)


def alone(plan, block):
    """The block alone on the same plan: what zafx_execute gives for it."""
    return plan.run_host(block[None], block.shape[1])[0]


def assert_blocks_equal_alone(zafx, w, blocks, sample=None):
    window = zafx.kaiser_bessel_derived(w)
    got = zafx.imdct_ragged(blocks, window)
    plan = grid_plan(zafx, window)
    assert plan.last_kernel == NATIVE, plan.last_kernel
    assert len(got) == len(blocks)
    for i in (range(len(blocks)) if sample is None else sample):
        ref = alone(plan, blocks[i])
        assert got[i].shape == ref.shape == (out_len(w, blocks[i].shape[1]),), (i, got[i].shape, ref.shape)
        assert np.array_equal(got[i], ref), (i, blocks[i].shape)
    return got


# ------------------------------------------------------------------ 1 and 2: against the oracle and against the block alone
@pytest.fixture(scope="module")
def cases(zafx):
    """Per window length: frame counts, blocks, imdct_ragged's result and the kernel that ran -- computed once, shared (tests 1, 2, 6)."""
    res = {}
    for w in WINDOWS:
        window = zafx.kaiser_bessel_derived(w)
        frames = frames_for(w)
        blocks = noise_blocks(w, frames, 2)
        got = zafx.imdct_ragged(blocks, window)
        res[w] = (window, frames, blocks, got, grid_plan(zafx, window).last_kernel)
    return res


@pytest.mark.parametrize("w", WINDOWS)
def test_imdct_ragged_against_oracle(cases, w):
    window, frames, blocks, got, kernel = cases[w]
    assert kernel == NATIVE, kernel
    assert len(got) == len(blocks)
    empty = []
    for i, (g, b) in enumerate(zip(got, blocks)):
        assert g.dtype == np.float32 and g.shape == (out_len(w, frames[i]),), (i, frames[i], g.shape)
        if not g.size:
            empty.append(i)
            continue
        ref = orc.imdct(b.astype(np.float64), window)
        assert ref.shape == g.shape, (i, ref.shape, g.shape)
        err = relerr(g, ref)
        print(f"W {w} block {i} T {frames[i]} relerr {err:.3e}")
        assert err <= TOL_IMDCT, (i, frames[i], err)
    assert empty == [i for i, t in enumerate(frames) if t == 1]   # exactly the one-frame blocks give no samples


@pytest.mark.parametrize("w", WINDOWS)
def test_every_block_has_the_bits_of_the_block_alone(zafx, cases, w):
    window, frames, blocks, got, kernel = cases[w]
    assert kernel == NATIVE
    plan = grid_plan(zafx, window)
    for i, (g, b) in enumerate(zip(got, blocks)):
        assert np.array_equal(g, alone(plan, b)), (i, frames[i])


# ------------------------------------------------------------------ 3: order does not matter
@pytest.mark.parametrize("w", WINDOWS)
def test_permutation_gives_identical_clips(zafx, w):
    frames = np.random.default_rng([10, w]).integers(1, 200, 46).tolist() + [1, 33, 64, 130]
    blocks = noise_blocks(w, frames, 11)
    perm = np.random.default_rng(12).permutation(len(blocks))
    window = zafx.kaiser_bessel_derived(w)
    a = zafx.imdct_ragged(blocks, window)
    b = zafx.imdct_ragged([blocks[i] for i in perm], window)
    assert grid_plan(zafx, window).last_kernel == NATIVE
    for j, i in enumerate(perm.tolist()):
        assert np.array_equal(a[i], b[j]), i


# ------------------------------------------------------------------ 4: cutting and striding
def test_more_units_than_workgroups(zafx):
    """1500 blocks of 1-3 tiles (about 3000 tiles against at most 512 resident workgroups): every workgroup strides through several units and
    prefetches across unit boundaries."""
    w = 512
    rng = np.random.default_rng(20)
    frames = [int(rng.integers(32 * (k - 1) + 2, 32 * k + 1)) for k in rng.integers(1, 4, 1500).tolist()]
    assert 2500 <= sum(-(-t // 32) for t in frames) <= 3500
    assert_blocks_equal_alone(zafx, w, noise_blocks(w, frames, 21))


def test_long_blocks_are_cut_into_segments(zafx):
    """3 blocks of 41 tiles on hundreds of workgroups: every clip is cut (segments of 3 tiles) and the carry-only prelude runs at each cut."""
    w = 512
    assert_blocks_equal_alone(zafx, w, noise_blocks(w, [40 * 32 + 5] * 3, 22))


def test_one_long_block_among_short_ones(zafx):
    w = 512
    rng = np.random.default_rng(23)
    frames = rng.integers(2, 70, 300).tolist()
    frames.insert(137, 40 * 32 + 5)
    assert_blocks_equal_alone(zafx, w, noise_blocks(w, frames, 24))


# ------------------------------------------------------------------ 5: the round trip, mdct_ragged's views as they lie
@pytest.mark.parametrize("w", WINDOWS)
def test_round_trip_from_mdct_ragged(zafx, w):
    m = w // 2
    lengths = [0, 1, m - 1, m, m + 1, 31 * m, 31 * m + 1, 44100]
    clips = [np.random.default_rng([30, w, i]).standard_normal(n).astype(np.float32) for i, n in enumerate(lengths)]
    window = zafx.kaiser_bessel_derived(w)
    spectra = zafx.mdct_ragged(clips, window)
    # (a clip of a whole number of hops comes back one sample short: zaf.imdct trims y[M : -M - 1], so T = N / M + 1 frames give N - 1 samples)
    keep = [min(n, out_len(w, s.shape[1])) for n, s in zip(lengths, spectra)]
    assert keep == [n - 1 if n and n % m == 0 else n for n in lengths]
    back = zafx.imdct_ragged(spectra, window, lengths=keep)
    assert grid_plan(zafx, window).last_kernel == NATIVE
    for i, (y, x) in enumerate(zip(back, clips)):
        x = x[:keep[i]]
        assert y.shape == x.shape and y.dtype == np.float32, (i, y.shape)
        err = float(np.max(np.abs(y - x))) if x.size else 0.0
        print(f"W {w} clip {i} n {lengths[i]} max|y - x| {err:.3e}")
        assert err <= TOL_ROUND_TRIP, (i, lengths[i], err)


# ------------------------------------------------------------------ 6: nothing outside, nothing missed, no neighbour
def packed_with_nan_pads(blocks, pitch_of):
    m = blocks[0].shape[0]
    pitches = [pitch_of(b.shape[1]) for b in blocks]
    in_off = np.concatenate([[0], np.cumsum([m * p for p in pitches])[:-1]]).astype(np.int64)
    packed = np.full(max(int(sum(m * p for p in pitches)), 1), np.nan, np.float32)
    for b, o, p in zip(blocks, in_off.tolist(), pitches):
        packed[o:o + m * p].reshape(m, p)[:, :b.shape[1]] = b
    return packed, in_off


@pytest.mark.parametrize("w", WINDOWS)
def test_writes_the_clips_and_nothing_else(zafx, cases, w):
    """NaN-filled arena, gaps between the clips, odd offsets among them, NaN in every block's pad columns: every gap keeps its NaN, no NaN
    comes into a clip, and every clip -- on an 8-byte boundary or on a 4-byte one only -- has the bits of the block alone (test 2)."""
    window, frames, blocks, got, kernel = cases[w]
    plan = grid_plan(zafx, window)
    packed, in_off = packed_with_nan_pads(blocks, plan.row_pitch)   # pad columns T_i ... TP_i - 1: NaN
    lens = [out_len(w, t) for t in frames]
    gaps = [3, 1, 32, 7, 2, 33, 64, 5]   # odd and even gaps: clips on 8-byte boundaries and on 4-byte ones only
    out_off, pos = [], 5
    for i, n in enumerate(lens):
        out_off.append(pos)
        pos += n + gaps[i % len(gaps)]
    assert any(o % 2 for o, n in zip(out_off, lens) if n) and any(o % 2 == 0 for o, n in zip(out_off, lens) if n)
    arena = np.full(pos + 64, np.nan, np.float32)
    d_in = zafx.DeviceBuffer.from_host(packed, plan.device)
    d_out = zafx.DeviceBuffer.from_host(arena, plan.device)
    plan.execute_imdct_ragged(d_in, in_off, frames, d_out, out_off)
    plan.sync()
    assert plan.last_kernel == NATIVE
    res = d_out.download()
    inside = np.zeros(len(arena), bool)
    for i, (o, n) in enumerate(zip(out_off, lens)):
        inside[o:o + n] = True
        bad = np.flatnonzero(res[o:o + n] != got[i])
        if bad.size:
            ulp = np.abs(res[o:o + n].view(np.int32)[bad].astype(np.int64) - got[i].view(np.int32)[bad])
            print(f"W {w} clip {i} T {frames[i]} at offset {o}: {bad.size} of {n} samples differ, first at {bad[0]}, last at {bad[-1]}, up to {int(ulp.max())} ulp")
    for i, (o, n) in enumerate(zip(out_off, lens)):
        assert np.array_equal(res[o:o + n], got[i]), (i, frames[i], o)   # (got: the bits of the block alone, test 2)
    assert np.all(np.isnan(res[~inside]))
    assert not np.any(np.isnan(res[inside]))


# ------------------------------------------------------------------ 7: the staging copy of the table
def test_back_to_back_calls_each_see_their_own_table(zafx):
    w = 1024
    plan = grid_plan(zafx, zafx.kaiser_bessel_derived(w))
    rng = np.random.default_rng(14)
    calls = []
    for b in range(2):
        frames = rng.integers(1, 120, 700 - 300 * b).tolist()
        packed, in_off = packed_with_nan_pads(noise_blocks(w, frames, 15 + b), plan.row_pitch)
        lens = np.array([out_len(w, t) for t in frames], np.int64)
        out_off = np.concatenate([[0], np.cumsum((lens + 31) // 32 * 32)[:-1]]).astype(np.int64)
        calls.append((zafx.DeviceBuffer.from_host(packed), in_off, frames, out_off, int(out_off[-1] + lens[-1]) + 32))
    outs = [zafx.DeviceBuffer((n,), np.float32) for *_, n in calls]
    expect = []
    for (d_in, in_off, frames, out_off, n), d_out in zip(calls, outs):   # one call at a time
        d_out.upload(np.zeros(n, np.float32))
        plan.execute_imdct_ragged(d_in, in_off, frames, d_out, out_off)
        plan.sync()
        assert plan.last_kernel == NATIVE
        expect.append(d_out.download())
        d_out.upload(np.zeros(n, np.float32))
    for (d_in, in_off, frames, out_off, n), d_out in zip(calls, outs):   # both enqueued, no sync between them
        plan.execute_imdct_ragged(d_in, in_off, frames, d_out, out_off)
    plan.sync()
    for e, d_out in zip(expect, outs):
        assert np.array_equal(d_out.download(), e)


# ------------------------------------------------------------------ 8: the routes that stay on one execute per clip
PER_CLIP = {
    "TF": dict(w=2048, layout="TF", f64=False, tol=TOL_IMDCT),
    "f64": dict(w=2048, layout="FT", f64=True, tol=TOL_F64),
    "W = 4096": dict(w=4096, layout="FT", f64=False, tol=TOL_IMDCT),
    "W = 256": dict(w=256, layout="FT", f64=False, tol=TOL_IMDCT),
}


@pytest.mark.parametrize("name", list(PER_CLIP))
def test_other_routes_stay_per_clip(zafx, name):
    c = PER_CLIP[name]
    w = c["w"]
    window = zafx.kaiser_bessel_derived(w)
    frames = [2, 33, 1, 70, 17]
    blocks = noise_blocks(w, frames, 40)
    given = [b.T.copy() for b in blocks] if c["layout"] == "TF" else blocks
    got = zafx.imdct_ragged(given, window, layout=c["layout"], f64=c["f64"])
    plan = zafx.mdct_plan(window, c["layout"], inverse=True, row_align=(16 if c["f64"] else 32) if c["layout"] == "FT" else 0, f64=c["f64"])   # (the plan imdct_ragged ran: rows of whole lines)
    assert plan.last_kernel and plan.last_kernel != NATIVE, (name, plan.last_kernel)
    for i, (g, b) in enumerate(zip(got, blocks)):
        assert g.dtype == (np.float64 if c["f64"] else np.float32) and g.shape == (out_len(w, frames[i]),), (name, i, g.shape)
        if g.size:
            err = relerr(g, orc.imdct(b.astype(np.float64), window))
            assert err <= c["tol"], (name, i, err)


def test_compact_pitch_off_the_grid_stays_per_clip(zafx):
    w = 2048
    window = zafx.kaiser_bessel_derived(w)
    plan = zafx.mdct_plan(window, inverse=True)   # compact rows: the pitch is T
    frames = [33, 2, 70, 17, 131]
    assert all(t % 4 for t in frames)
    blocks = noise_blocks(w, frames, 41)
    packed, in_off = packed_with_nan_pads(blocks, lambda t: t)
    lens = [out_len(w, t) for t in frames]
    out_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    d_in = zafx.DeviceBuffer.from_host(packed, plan.device)
    d_out = zafx.DeviceBuffer((sum(lens),), np.float32, plan.device)
    plan.execute_imdct_ragged(d_in, in_off, frames, d_out, out_off)
    plan.sync()
    assert plan.last_kernel and plan.last_kernel != NATIVE, plan.last_kernel
    res = d_out.download()
    for i, (o, n, b) in enumerate(zip(out_off.tolist(), lens, blocks)):
        err = relerr(res[o:o + n], orc.imdct(b.astype(np.float64), window))
        assert err <= TOL_IMDCT, (i, err)


CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {pkg!r}]
import zafx
w = 1024
frames = {frames!r}
blocks = [np.random.default_rng([50, w, i]).standard_normal((w // 2, t)).astype(np.float32) for i, t in enumerate(frames)]
window = zafx.kaiser_bessel_derived(w)
got = zafx.imdct_ragged(blocks, window)
kernel = zafx.mdct_plan(window, inverse=True, row_align=32).last_kernel
np.savez({out!r}, kernel=np.array(kernel), **{{f"y{{i}}": g for i, g in enumerate(got)}})
"""


def test_the_measurement_switch_keeps_a_batch_per_clip(zafx, tmp_path):
    """ZAFX_RAGGED_IMDCT_NATIVE=0, set in a fresh child process: the per-clip path, array_equal to the one launch."""
    w = 1024
    frames = FRAMES + [150]
    blocks = noise_blocks(w, frames, 50)
    window = zafx.kaiser_bessel_derived(w)
    native = zafx.imdct_ragged(blocks, window)
    assert grid_plan(zafx, window).last_kernel == NATIVE
    out = str(tmp_path / "per_clip.npz")
    script = CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "zaf-python_amd"), frames=frames, out=out)
    env = dict(os.environ, ZAFX_RAGGED_IMDCT_NATIVE="0")
    res = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-1000:]
    child = np.load(out)
    assert str(child["kernel"]) != NATIVE and str(child["kernel"]), child["kernel"]
    for i, g in enumerate(native):
        assert np.array_equal(child[f"y{i}"], g), (i, frames[i])


# ------------------------------------------------------------------ 9: errors through the C-ABI
def raw_call(zafx, plan, d_in, in_off, frames, d_out, out_off):
    from zafx import _lib
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (in_off, frames, out_off)]
    p = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) for a in arrs]
    lib = _lib.load()
    rc = lib.zafx_execute_imdct_ragged(plan.handle, d_in.ptr, p[0], p[1], d_out.ptr, p[2], len(arrs[1]))
    return rc, (lib.zafx_last_error() or b"").decode()


def test_errors_come_with_a_message_and_leave_the_plan_usable(zafx):
    w = 512
    window = zafx.kaiser_bessel_derived(w)
    plan = grid_plan(zafx, window)
    blocks = noise_blocks(w, [3, 40], 60)
    packed, in_off = packed_with_nan_pads(blocks, plan.row_pitch)
    d_in = zafx.DeviceBuffer.from_host(packed, plan.device)
    d_out = zafx.DeviceBuffer((2 * 40 * 256,), np.float32, plan.device)
    out_off = [0, 1024]
    for other in (zafx.mdct_plan(window, row_align=32), zafx.stft_plan(zafx.hamming(w), w // 2)):
        rc, msg = raw_call(zafx, other, d_in, in_off, [3, 40], d_out, out_off)
        assert rc != 0 and "zafx_execute_imdct_ragged" in msg and "inverse MDCT" in msg, (rc, msg)
    rc, msg = raw_call(zafx, plan, d_in, in_off, [3, -40], d_out, out_off)
    assert rc != 0 and "negative" in msg and "clip 1" in msg, (rc, msg)
    rc, msg = raw_call(zafx, plan, d_in, [-1, int(in_off[1])], [3, 40], d_out, out_off)
    assert rc != 0 and "negative" in msg and "clip 0" in msg, (rc, msg)
    rc, msg = raw_call(zafx, plan, d_in, in_off, [3, 40], d_out, [0, -8])
    assert rc != 0 and "negative" in msg and "clip 1" in msg, (rc, msg)
    with pytest.raises(zafx.ZafxError, match="negative"):
        plan.execute_imdct_ragged(d_in, in_off, [3, -40], d_out, out_off)
    plan.execute_imdct_ragged(d_in, in_off, [3, 40], d_out, out_off)   # a later valid call on the same plan
    plan.sync()
    assert plan.last_kernel == NATIVE
    res = d_out.download()
    for b, o in zip(blocks, out_off):
        ref = alone(plan, b)
        assert np.array_equal(res[o:o + len(ref)], ref)
