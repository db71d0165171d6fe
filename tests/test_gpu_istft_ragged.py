"""Ragged batches of the inverse STFT on the GPU (-m gpu): spectra of different frame counts in one launch of k_istft_ft16's RAGGED form
(zafx.istft_ragged, Plan.execute_istft_ragged, zafx_execute_istft_ragged) -- against the CPU oracle, bit for bit against every block alone on
the same plan, and on the routes that stay on one execute per clip.  A tile is 16 frames of one clip: the frame counts sit around whole
tiles."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import signals
from conftest import ROOT, relerr
from oracle import zaf_oracle as orc

pytestmark = pytest.mark.gpu

TOL_ISTFT = 1e-5       # the ISTFT against the float64 oracle (TOL_FFT elsewhere in the suite)
TOL_F64 = 1e-12        # the float64 kernels
NATIVE = "k_istft_ragged"
WINDOWS = [256, 512, 1024, 2048]
FRAMES = [1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 49, 65, 130]
TILE = 16


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    return z


def frames_for(w, seed=1):
    return FRAMES + np.random.default_rng([seed, w]).integers(1, 201, 4).tolist()


def rows_of(w, onesided):
    return w // 2 + 1 if onesided else w


def noise_blocks(w, frames, seed, onesided=False):
    res = []
    for i, t in enumerate(frames):
        g = np.random.default_rng([seed, w, i]).standard_normal((2, rows_of(w, onesided), t))
        res.append((g[0] + 1j * g[1]).astype(np.complex64))
    return res


def out_len(w, h, t):
    return max(t * h - (w - h), 0)


def two_sided(block, w):
    """A one-sided block completed by conjugate symmetry: what the oracle takes."""
    b = block.astype(np.complex128)
    return b if b.shape[0] == w else np.concatenate([b, np.conj(b[w // 2 - 1:0:-1])], axis=0)


def oracle(block, window, h):
    return orc.istft(two_sided(block, len(window)), window, h)


def grid_plan(zafx, window, h, onesided=False):
    return zafx.istft_plan(window, h, onesided=onesided, row_align=16)


def alone(plan, block):
    """The block alone on the same plan: what zafx_execute gives for it."""
    return plan.run_host(block[None], block.shape[1])[0]


def assert_blocks_equal_alone(zafx, w, h, blocks, onesided=False, sample=None):
    window = zafx.hamming(w)
    got = zafx.istft_ragged(blocks, window, h, onesided=onesided)
    plan = grid_plan(zafx, window, h, onesided)
    assert plan.last_kernel == NATIVE, plan.last_kernel
    assert len(got) == len(blocks)
    for i, g in enumerate(got):
        assert g.dtype == np.float32 and g.shape == (out_len(w, h, blocks[i].shape[1]),), (i, g.shape)
    for i in (range(len(blocks)) if sample is None else sample):
        if not got[i].size:
            continue
        ref = alone(plan, blocks[i])
        assert ref.shape == got[i].shape, (i, got[i].shape, ref.shape)
        assert np.array_equal(got[i], ref), (i, blocks[i].shape)
    return got


# ------------------------------------------------------------------ 1: against the oracle (hop W / 2, two-sided and one-sided)
@pytest.fixture(scope="module")
def cases(zafx):
    """Per (window length, one-sided): frame counts, blocks, istft_ragged's result and the kernel that ran -- computed once, shared (tests 1, 2, 6)."""
    res = {}
    for w in WINDOWS:
        for onesided in (False, True):
            window = zafx.hamming(w)
            frames = frames_for(w)
            blocks = noise_blocks(w, frames, 2, onesided)
            got = zafx.istft_ragged(blocks, window, w // 2, onesided=onesided)
            res[w, onesided] = (window, frames, blocks, got, grid_plan(zafx, window, w // 2, onesided).last_kernel)
    return res


@pytest.mark.parametrize("onesided", [False, True])
@pytest.mark.parametrize("w", WINDOWS)
def test_istft_ragged_against_oracle(cases, w, onesided):
    window, frames, blocks, got, kernel = cases[w, onesided]
    h = w // 2
    assert kernel == NATIVE, kernel
    assert len(got) == len(blocks)
    empty = []
    for i, (g, b) in enumerate(zip(got, blocks)):
        assert g.dtype == np.float32 and g.shape == (out_len(w, h, frames[i]),), (i, frames[i], g.shape)
        if not g.size:
            empty.append(i)
            continue
        ref = oracle(b, window, h)
        assert ref.shape == g.shape, (i, ref.shape, g.shape)
        err = relerr(g, ref)
        print(f"W {w} onesided {onesided} block {i} T {frames[i]} relerr {err:.3e}")
        assert err <= TOL_ISTFT, (i, frames[i], err)
    assert empty == [i for i, t in enumerate(frames) if t == 1]   # hop W / 2: exactly the one-frame blocks give no samples


# ------------------------------------------------------------------ 2: bit for bit against the block alone, all three overlap-add forms
HOPS = {"sweep": lambda w: w // 2, "pairs": lambda w: 3 * w // 4, "generic W/4": lambda w: w // 4, "generic W/2+1": lambda w: w // 2 + 1}
BITS = [(w, form, onesided) for w in WINDOWS for form in HOPS for onesided in ((False, True) if w == 512 else (w == 2048,))]


@pytest.mark.parametrize("w,form,onesided", BITS)
def test_every_block_has_the_bits_of_the_block_alone(zafx, w, form, onesided):
    h = HOPS[form](w)
    frames = frames_for(w)
    got = assert_blocks_equal_alone(zafx, w, h, noise_blocks(w, frames, 3, onesided), onesided)
    assert [i for i, g in enumerate(got) if not g.size] == [i for i, t in enumerate(frames) if t * h <= w - h]


def packed_with_nan_pads(blocks, pitch_of, lead=0):
    """The blocks back to back at their pitches behind `lead` complex elements, NaN in every pad column: -> (packed, in_offsets)."""
    rows = blocks[0].shape[0]
    pitches = [pitch_of(b.shape[1]) for b in blocks]
    in_off = (lead + np.concatenate([[0], np.cumsum([rows * p for p in pitches])[:-1]])).astype(np.int64)
    packed = np.full(lead + max(int(sum(rows * p for p in pitches)), 1), np.nan + 1j * np.nan, np.complex64)
    for b, o, p in zip(blocks, in_off.tolist(), pitches):
        packed[o:o + rows * p].reshape(rows, p)[:, :b.shape[1]] = b
    return packed, in_off


@pytest.mark.parametrize("w", [512, 2048])
def test_a_spectrum_array_on_four_bytes_only(zafx, cases, w):
    """The array at 4 mod 8 bytes: the 8-byte gather (FV = 1); the same bits."""
    window, frames, blocks, got, kernel = cases[w, False]
    h = w // 2
    plan = grid_plan(zafx, window, h)
    packed, in_off = packed_with_nan_pads(blocks, plan.row_pitch)
    raw = np.concatenate([np.zeros(1, np.float32), packed.view(np.float32), np.zeros(1, np.float32)])
    d_raw = zafx.DeviceBuffer.from_host(raw, plan.device)
    d_in = zafx.DeviceBuffer(packed.shape, np.complex64, plan.device, _ptr_from_pool=ctypes.c_void_p(d_raw.ptr.value + 4))
    assert d_in.ptr.value % 8 == 4
    lens = np.array([out_len(w, h, t) for t in frames], np.int64)
    out_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    d_out = zafx.DeviceBuffer((int(lens.sum()),), np.float32, plan.device)
    plan.execute_istft_ragged(d_in, in_off, frames, d_out, out_off)
    plan.sync()
    d_in.ptr = ctypes.c_void_p()   # (a view, not an allocation: nothing to free)
    assert plan.last_kernel == NATIVE
    res = d_out.download()
    for i, (o, n) in enumerate(zip(out_off.tolist(), lens.tolist())):
        assert np.array_equal(res[o:o + n], got[i]), (i, frames[i])


# ------------------------------------------------------------------ 3: order does not matter
@pytest.mark.parametrize("w", WINDOWS)
def test_permutation_gives_identical_clips(zafx, w):
    frames = np.random.default_rng([10, w]).integers(1, 201, 46).tolist() + [1, 17, 32, 130]
    blocks = noise_blocks(w, frames, 11, onesided=True)
    perm = np.random.default_rng(12).permutation(len(blocks))
    window = zafx.hamming(w)
    a = zafx.istft_ragged(blocks, window, w // 2, onesided=True)
    b = zafx.istft_ragged([blocks[i] for i in perm], window, w // 2, onesided=True)
    assert grid_plan(zafx, window, w // 2, True).last_kernel == NATIVE
    for j, i in enumerate(perm.tolist()):
        assert np.array_equal(a[i], b[j]), i


# ------------------------------------------------------------------ 4: cutting and striding (W = 256, one-sided: small)
def test_more_units_than_workgroups(zafx):
    """1500 blocks of 1-3 tiles (about 3000 tiles against at most 512 resident workgroups): every workgroup strides through several units and
    prefetches across unit boundaries.  Every clip's shape is checked, a sample of them against the block alone."""
    w = 256
    rng = np.random.default_rng(20)
    frames = [int(rng.integers(TILE * (k - 1) + 2, TILE * k + 1)) for k in rng.integers(1, 4, 1500).tolist()]
    assert 2500 <= sum(-(-t // TILE) for t in frames) <= 3500
    sample = sorted(set(rng.integers(0, 1500, 120).tolist()) | {0, 1, 2, 1497, 1498, 1499})
    assert_blocks_equal_alone(zafx, w, w // 2, noise_blocks(w, frames, 21, True), True, sample=sample)


def test_long_blocks_are_cut_into_segments(zafx):
    """3 blocks of 41 tiles on hundreds of workgroups: every clip is cut (segments of 3 tiles) and the carry-only prelude runs at each cut --
    in all three overlap-add forms."""
    w = 256
    for form in HOPS:
        assert_blocks_equal_alone(zafx, w, HOPS[form](w), noise_blocks(w, [40 * TILE + 5] * 3, 22, True), True)


def test_one_long_block_among_short_ones(zafx):
    w = 256
    rng = np.random.default_rng(23)
    frames = rng.integers(2, 70, 300).tolist()
    frames.insert(137, 40 * TILE + 5)
    sample = sorted(set(rng.integers(0, 301, 60).tolist()) | {136, 137, 138, 0, 300})
    assert_blocks_equal_alone(zafx, w, w // 2, noise_blocks(w, frames, 24, True), True, sample=sample)


# ------------------------------------------------------------------ 5: the round trip, stft_ragged's views as they lie
@pytest.mark.parametrize("onesided", [False, True])
@pytest.mark.parametrize("w", WINDOWS)
def test_round_trip_from_stft_ragged(zafx, w, onesided):
    """The residual max|y - x| of the ragged pair is held to twice the largest residual of the equal-length pair istft_batch(stft_batch(x)) on
    the same clips: the arithmetic is the same, only the launch differs."""
    h = w // 2
    lengths = [0, 1, h - 1, h, h + 1, 31 * h, 31 * h + 1, 44100]
    clips = [np.random.default_rng([30, w, i]).standard_normal(n).astype(np.float32) for i, n in enumerate(lengths)]
    window = zafx.hamming(w)
    equal = 0.0
    for x in clips:
        if x.size:
            y = zafx.istft_batch(zafx.stft_batch(x[None], window, h, onesided=onesided), window, h, onesided=onesided)[0]
            equal = max(equal, float(np.max(np.abs(y[:x.size] - x))))
    bound = 2.0 * equal
    spectra = zafx.stft_ragged(clips, window, h, onesided=onesided)
    back = zafx.istft_ragged(spectra, window, h, onesided=onesided, lengths=lengths)
    assert grid_plan(zafx, window, h, onesided).last_kernel == NATIVE
    worst = 0.0
    for i, (y, x, s) in enumerate(zip(back, clips, spectra)):
        assert y.shape == x.shape and y.dtype == np.float32, (i, y.shape)
        if x.size:   # (the spectrum alone through the equal-length call, cut to the length)
            ref = zafx.istft_batch(np.ascontiguousarray(s)[None], window, h, onesided=onesided)[0][:lengths[i]]
            assert np.array_equal(y, ref), i
        err = float(np.max(np.abs(y - x))) if x.size else 0.0
        worst = max(worst, err)
        print(f"W {w} onesided {onesided} clip {i} n {lengths[i]} max|y - x| {err:.3e}")
    print(f"W {w} onesided {onesided}: equal-length pair residual {equal:.3e}, bound {bound:.3e}, ragged pair {worst:.3e}")
    assert 0.0 < equal < 1e-4, equal   # (the yardstick itself is sane: float32 round-off on unit noise)
    assert worst <= bound, (worst, bound)


# ------------------------------------------------------------------ 6: nothing outside, nothing missed, no neighbour
GAPS = [3, 1, 32, 7, 2, 33, 64, 5]   # odd and even gaps: clips on 8-byte boundaries and on 4-byte ones only


def run_in_arena(zafx, plan, blocks, frames, w, h):
    """-> (arena after the call, output offsets, lengths): NaN arena, NaN pad columns, GAPS between the clips."""
    packed, in_off = packed_with_nan_pads(blocks, plan.row_pitch)
    lens = [out_len(w, h, t) for t in frames]
    out_off, pos = [], 5
    for i, n in enumerate(lens):
        out_off.append(pos)
        pos += n + GAPS[i % len(GAPS)]
    assert any(o % 2 for o, n in zip(out_off, lens) if n) and any(o % 2 == 0 for o, n in zip(out_off, lens) if n)
    arena = np.full(pos + 64, np.nan, np.float32)
    d_in = zafx.DeviceBuffer.from_host(packed, plan.device)
    d_out = zafx.DeviceBuffer.from_host(arena, plan.device)
    plan.execute_istft_ragged(d_in, in_off, frames, d_out, out_off)
    plan.sync()
    assert plan.last_kernel == NATIVE
    return d_out.download(), out_off, lens


def assert_only_the_clips(res, out_off, lens):
    inside = np.zeros(len(res), bool)
    for o, n in zip(out_off, lens):
        inside[o:o + n] = True
    assert np.all(np.isnan(res[~inside]))
    assert not np.any(np.isnan(res[inside]))


@pytest.mark.parametrize("onesided", [False, True])
@pytest.mark.parametrize("w", WINDOWS)
def test_writes_the_clips_and_nothing_else(zafx, cases, w, onesided):
    """NaN-filled arena, gaps between the clips, odd offsets among them, NaN in every block's pad columns: every gap keeps its NaN, no NaN
    comes into a clip, and every clip -- on an 8-byte boundary or on a 4-byte one only -- has the bits of the block alone."""
    window, frames, blocks, got, kernel = cases[w, onesided]
    h = w // 2
    plan = grid_plan(zafx, window, h, onesided)
    res, out_off, lens = run_in_arena(zafx, plan, blocks, frames, w, h)
    for i, (o, n) in enumerate(zip(out_off, lens)):
        assert np.array_equal(res[o:o + n], got[i]), (i, frames[i], o)
        if n and i in (2, 5, 12):   # (got against the block alone: all of it in test 2; here where the clip sits on 4 bytes only, too)
            assert np.array_equal(got[i], alone(plan, blocks[i])), i
    assert_only_the_clips(res, out_off, lens)


def test_signals_in_the_arena(zafx):
    """Silence, DC, impulses and tones (tests/signals.py) through stft_ragged, then through the arena run: silence comes back exactly zero,
    the others meet the oracle."""
    w, h = signals.W, signals.HOP
    names = ["silence", "dc", "impulse", "sine_bin", "sine_half", "two_tones"]
    lengths = [3072, 5000, 3072, 16 * h, 17 * h + 3, 44100]
    window = zafx.hamming(w)
    spectra = [np.ascontiguousarray(s) for s in zafx.stft_ragged([signals.signal(n, k) for n, k in zip(names, lengths)], window, h)]
    frames = [s.shape[1] for s in spectra]
    plan = grid_plan(zafx, window, h)
    res, out_off, lens = run_in_arena(zafx, plan, spectra, frames, w, h)
    assert_only_the_clips(res, out_off, lens)
    for name, s, o, n in zip(names, spectra, out_off, lens):
        y = res[o:o + n]
        if name == "silence":
            assert n and not np.any(y), name
        else:
            err = relerr(y, oracle(s, window, h))
            print(f"{name}: relerr {err:.3e}")
            assert err <= TOL_ISTFT, (name, err)


# ------------------------------------------------------------------ 7: the staging copy of the table
def test_back_to_back_calls_each_see_their_own_table(zafx):
    w, h = 512, 256
    plan = grid_plan(zafx, zafx.hamming(w), h, True)
    rng = np.random.default_rng(14)
    calls = []
    for b in range(2):
        frames = rng.integers(1, 80, 400 - 150 * b).tolist()
        packed, in_off = packed_with_nan_pads(noise_blocks(w, frames, 15 + b, True), plan.row_pitch)
        lens = np.array([out_len(w, h, t) for t in frames], np.int64)
        out_off = np.concatenate([[0], np.cumsum((lens + 31) // 32 * 32)[:-1]]).astype(np.int64)
        calls.append((zafx.DeviceBuffer.from_host(packed), in_off, frames, out_off, int(out_off[-1] + lens[-1]) + 32))
    outs = [zafx.DeviceBuffer((n,), np.float32) for *_, n in calls]
    expect = []
    for (d_in, in_off, frames, out_off, n), d_out in zip(calls, outs):   # one call at a time
        d_out.upload(np.zeros(n, np.float32))
        plan.execute_istft_ragged(d_in, in_off, frames, d_out, out_off)
        plan.sync()
        assert plan.last_kernel == NATIVE
        expect.append(d_out.download())
        d_out.upload(np.zeros(n, np.float32))
    for (d_in, in_off, frames, out_off, n), d_out in zip(calls, outs):   # both enqueued, no sync between them
        plan.execute_istft_ragged(d_in, in_off, frames, d_out, out_off)
    plan.sync()
    for e, d_out in zip(expect, outs):
        assert np.array_equal(d_out.download(), e)


# ------------------------------------------------------------------ 8: the routes that stay on one execute per clip
PER_CLIP = {
    "TF": dict(w=2048, h=1024, layout="TF", f64=False, tol=TOL_ISTFT),
    "f64": dict(w=2048, h=1024, layout="FT", f64=True, tol=TOL_F64),
    "W = 4096": dict(w=4096, h=2048, layout="FT", f64=False, tol=TOL_ISTFT),
    "W = 128": dict(w=128, h=64, layout="FT", f64=False, tol=TOL_ISTFT),
    "halo >= 16": dict(w=256, h=15, layout="FT", f64=False, tol=TOL_ISTFT),   # ceil(256 / 15) - 1 = 17 frames before a sample's last: the gather form
}


@pytest.mark.parametrize("name", list(PER_CLIP))
def test_other_routes_stay_per_clip(zafx, name):
    c = PER_CLIP[name]
    w, h = c["w"], c["h"]
    window = zafx.hamming(w)
    frames = [2, 33, 1, 70, 17]
    blocks = noise_blocks(w, frames, 40)
    given = [b.T.copy() for b in blocks] if c["layout"] == "TF" else blocks
    got = zafx.istft_ragged(given, window, h, layout=c["layout"], f64=c["f64"])
    plan = zafx.istft_plan(window, h, c["layout"], f64=c["f64"], row_align=(8 if c["f64"] else 16) if c["layout"] == "FT" else 0)   # (the plan istft_ragged ran: rows of whole lines)
    assert plan.last_kernel and plan.last_kernel != NATIVE, (name, plan.last_kernel)
    for i, (g, b) in enumerate(zip(got, blocks)):
        assert g.dtype == (np.float64 if c["f64"] else np.float32) and g.shape == (out_len(w, h, frames[i]),), (name, i, g.shape)
        if g.size:
            err = relerr(g, oracle(b, window, h))
            assert err <= c["tol"], (name, i, err)


# ------------------------------------------------------------------ 9: the measurement switch
CHILD = """
import sys
import numpy as np
sys.path[:0] = [{root!r}, {pkg!r}]
import zafx
w = 1024
frames = {frames!r}
blocks = []
for i, t in enumerate(frames):
    g = np.random.default_rng([50, w, i]).standard_normal((2, w, t))
    blocks.append((g[0] + 1j * g[1]).astype(np.complex64))
window = zafx.hamming(w)
got = zafx.istft_ragged(blocks, window, w // 2)
kernel = zafx.istft_plan(window, w // 2, row_align=16).last_kernel
np.savez({out!r}, kernel=np.array(kernel), **{{f"y{{i}}": g for i, g in enumerate(got)}})
"""


def test_the_measurement_switch_keeps_a_batch_per_clip(zafx, tmp_path):
    """ZAFX_RAGGED_ISTFT_NATIVE=0, set in a fresh child process: the per-clip path, array_equal to the one launch."""
    w = 1024
    frames = FRAMES + [150]
    blocks = noise_blocks(w, frames, 50)
    window = zafx.hamming(w)
    native = zafx.istft_ragged(blocks, window, w // 2)
    assert grid_plan(zafx, window, w // 2).last_kernel == NATIVE
    out = str(tmp_path / "per_clip.npz")
    script = CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "zaf-python_amd"), frames=frames, out=out)
    env = dict(os.environ, ZAFX_RAGGED_ISTFT_NATIVE="0")
    res = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-1000:]
    child = np.load(out)
    assert str(child["kernel"]) != NATIVE and str(child["kernel"]), child["kernel"]
    for i, g in enumerate(native):
        assert np.array_equal(child[f"y{i}"], g), (i, frames[i])


# ------------------------------------------------------------------ 10: errors through the C-ABI
def raw_call(zafx, plan, d_in, in_off, frames, d_out, out_off):
    from zafx import _lib
    arrs = [np.ascontiguousarray(a, dtype=np.int64) for a in (in_off, frames, out_off)]
    p = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) for a in arrs]
    lib = _lib.load()
    rc = lib.zafx_execute_istft_ragged(plan.handle, d_in.ptr, p[0], p[1], d_out.ptr, p[2], len(arrs[1]))
    return rc, (lib.zafx_last_error() or b"").decode()


def test_errors_come_with_a_message_and_leave_the_plan_usable(zafx):
    w, h = 512, 256
    window = zafx.hamming(w)
    plan = grid_plan(zafx, window, h)
    blocks = noise_blocks(w, [3, 40], 60)
    packed, in_off = packed_with_nan_pads(blocks, plan.row_pitch)
    d_in = zafx.DeviceBuffer.from_host(packed, plan.device)
    d_out = zafx.DeviceBuffer((2 * 40 * 256,), np.float32, plan.device)
    out_off = [0, 1024]
    for other in (zafx.stft_plan(window, h, row_align=16), zafx.mdct_plan(zafx.kaiser_bessel_derived(w), inverse=True, row_align=32)):
        rc, msg = raw_call(zafx, other, d_in, in_off, [3, 40], d_out, out_off)
        assert rc != 0 and "zafx_execute_istft_ragged" in msg and "inverse STFT" in msg, (rc, msg)
    rc, msg = raw_call(zafx, plan, d_in, in_off, [3, -40], d_out, out_off)
    assert rc != 0 and "negative" in msg and "clip 1" in msg, (rc, msg)
    rc, msg = raw_call(zafx, plan, d_in, [-1, int(in_off[1])], [3, 40], d_out, out_off)
    assert rc != 0 and "negative" in msg and "clip 0" in msg, (rc, msg)
    rc, msg = raw_call(zafx, plan, d_in, in_off, [3, 40], d_out, [0, -8])
    assert rc != 0 and "negative" in msg and "clip 1" in msg, (rc, msg)
    from zafx import _lib
    rc = _lib.load().zafx_execute_istft_ragged(plan.handle, d_in.ptr, None, None, d_out.ptr, None, -1)
    assert rc != 0 and b"negative number of clips" in _lib.load().zafx_last_error()
    with pytest.raises(zafx.ZafxError, match="negative"):
        plan.execute_istft_ragged(d_in, in_off, [3, -40], d_out, out_off)
    plan.execute_istft_ragged(d_in, in_off, [3, 40], d_out, out_off)   # a later valid call on the same plan
    plan.sync()
    assert plan.last_kernel == NATIVE
    res = d_out.download()
    for b, o in zip(blocks, out_off):
        ref = alone(plan, b)
        assert np.array_equal(res[o:o + len(ref)], ref)
