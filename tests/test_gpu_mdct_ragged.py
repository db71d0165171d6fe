"""Ragged batches of the MDCT on the GPU (-m gpu): clips of different lengths in one launch of k_mdct_ft32's RAGGED form (zafx.mdct_ragged,
zafx_execute_ragged), against the CPU oracle, against the padded equal-length batch on the same plan, and on the routes that stay on one
execute per clip.  A tile is 32 frames of one clip and T = ceil(n / M) + 1 with M = W / 2: the lengths sit around whole tiles."""
import numpy as np
import pytest

from conftest import relerr
from oracle import zaf_oracle as orc

pytestmark = pytest.mark.gpu

TOL_MDCT = 1e-5        # the MDCT against the float64 oracle
TOL_FORMS = 1e-6       # two float32 forms of the same arithmetic (the bound test_gpu_ragged.py uses across forms)
TOL_ROUND_TRIP = 1e-5  # |imdct(mdct(x)) - x| on unit-variance noise, absolute
NATIVE = "k_mdct_ft32_ragged"
WINDOWS = [512, 1024, 2048]


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    return z


def lengths_for(w, seed, n_random=4):
    m = w // 2
    rng = np.random.default_rng([seed, w])
    return [0, 1, m - 1, m, m + 1, 30 * m + 1, 31 * m, 31 * m + 1, 63 * m + 1, 44100, 123457] + rng.integers(0, 50000, n_random).tolist()


def noise_clips(lengths, seed):
    return [np.random.default_rng([seed, i]).standard_normal(n).astype(np.float32) for i, n in enumerate(lengths)]


def family(name):
    return name[: -len("_ragged")] if name.endswith("_ragged") else name


def grid_plan(zafx, window):
    return zafx.mdct_plan(window, row_align=32)


def padded_reference(plan, clips):
    """The padded equal-length batch on the same plan: (B, F, T) results and the kernel that ran."""
    nmax = max(len(c) for c in clips)
    x = np.zeros((len(clips), nmax), plan.in_dtype)
    for i, c in enumerate(clips):
        x[i, : len(c)] = c
    out = plan.run_host(x, nmax)
    return out, plan.last_kernel


def frames_of(n, w):
    return -(-n // (w // 2)) + 1


# ------------------------------------------------------------------ 1: against the oracle, native path taken
@pytest.fixture(scope="module")
def oracle_cases(zafx):
    """Per (window length, form): lengths, clips, the oracle's result per clip and mdct_ragged's -- computed once, shared (tests 1 and 8)."""
    cases = {}
    for w in WINDOWS:
        window = zafx.kaiser_bessel_derived(w)
        for form in ("aligned", "edge"):
            lengths = lengths_for(w, 1)
            if form == "aligned":
                lengths = [n - n % 4 for n in lengths]
            clips = noise_clips(lengths, 2)
            refs = [orc.mdct(c.astype(np.float64), window) for c in clips]
            got = zafx.mdct_ragged(clips, window)
            cases[w, form] = (window, lengths, clips, refs, got, grid_plan(zafx, window).last_kernel)
    return cases


@pytest.mark.parametrize("form", ["aligned", "edge"])
@pytest.mark.parametrize("w", WINDOWS)
def test_mdct_ragged_against_oracle(oracle_cases, w, form):
    window, lengths, clips, refs, got, kernel = oracle_cases[w, form]
    assert kernel == NATIVE, kernel
    assert len(got) == len(clips)
    for i, (g, r) in enumerate(zip(got, refs)):
        assert g.shape == r.shape == (w // 2, frames_of(lengths[i], w)), (i, lengths[i], g.shape, r.shape)
        assert g.dtype == np.float32
        err = relerr(g, r)
        print(f"W {w} {form} clip {i} n {lengths[i]} relerr {err:.3e}")
        assert err <= TOL_MDCT, (i, lengths[i], err)


# ------------------------------------------------------------------ 2: against the padded batch on the same plan
@pytest.mark.parametrize("lengths_are", ["multiples of 4", "any"])
@pytest.mark.parametrize("w", WINDOWS)
def test_mdct_ragged_equals_padded_batch(zafx, w, lengths_are):
    lengths = np.random.default_rng([5, w]).integers(0, 40000, 64)
    if lengths_are == "multiples of 4":
        lengths -= lengths % 4   # (the longest one too: the padded batch runs the buffer-load form as well)
    clips = noise_clips(lengths.tolist(), 6)
    window = zafx.kaiser_bessel_derived(w)
    got = zafx.mdct_ragged(clips, window)
    plan = grid_plan(zafx, window)
    assert plan.last_kernel == NATIVE
    pad, pad_kernel = padded_reference(plan, clips)
    assert family(pad_kernel) == "k_mdct_ft32", pad_kernel
    for i, g in enumerate(got):
        ref = pad[i][:, : g.shape[1]]
        assert g.shape[1] == frames_of(int(lengths[i]), w)
        if lengths_are == "multiples of 4":
            assert np.array_equal(g, ref), i
        else:
            err = relerr(g, ref)
            assert err <= TOL_FORMS, (i, int(lengths[i]), err)


# ------------------------------------------------------------------ 3: order does not matter
@pytest.mark.parametrize("w", WINDOWS)
def test_permutation_gives_identical_clips(zafx, w):
    lengths = np.random.default_rng([10, w]).integers(0, 30000, 48).tolist() + [0, 31 * (w // 2) + 1]
    clips = noise_clips(lengths, 11)
    perm = np.random.default_rng(12).permutation(len(clips))
    window = zafx.kaiser_bessel_derived(w)
    for cut in (1, 4):   # the edge form and the buffer-load form
        batch = [c[: len(c) - len(c) % cut] for c in clips]
        a = zafx.mdct_ragged(batch, window)
        b = zafx.mdct_ragged([batch[i] for i in perm], window)
        assert grid_plan(zafx, window).last_kernel == NATIVE
        for j, i in enumerate(perm.tolist()):
            assert np.array_equal(a[i], b[j]), (cut, i)


# ------------------------------------------------------------------ 4: more tiles than workgroups
def test_more_tiles_than_workgroups(zafx):
    """1500 clips of 1-3 tiles (about 3000 tiles against at most 512 resident workgroups): every workgroup strides through several clips and
    prefetches across clip boundaries."""
    w, m = 512, 256
    rng = np.random.default_rng(20)
    tiles = rng.integers(1, 4, 1500)
    lengths = [int(rng.integers(max(32 * (k - 1) * m - m + 1, 0), 31 * m + 32 * (k - 1) * m + 1)) for k in tiles.tolist()]
    assert all(-(-frames_of(n, w) // 32) == k for n, k in zip(lengths, tiles.tolist()))
    assert 2500 <= int(tiles.sum()) <= 3500
    clips = noise_clips(lengths, 21)
    window = zafx.kaiser_bessel_derived(w)
    a = zafx.mdct_ragged(clips, window)
    assert grid_plan(zafx, window).last_kernel == NATIVE
    for i in np.random.default_rng(22).choice(len(clips), 32, replace=False).tolist():
        ref = orc.mdct(clips[i].astype(np.float64), window)
        assert a[i].shape == ref.shape and relerr(a[i], ref) <= TOL_MDCT, (i, lengths[i])
    perm = np.random.default_rng(23).permutation(len(clips))
    b = zafx.mdct_ragged([clips[i] for i in perm], window)
    for j, i in enumerate(perm.tolist()):
        assert np.array_equal(a[i], b[j]), i


# ------------------------------------------------------------------ 5: nothing but the clips is written
@pytest.mark.parametrize("cut", [1, 4])
@pytest.mark.parametrize("w", WINDOWS)
def test_ragged_writes_nothing_but_the_clips(zafx, w, cut):
    lengths = [n - n % cut for n in [0, 1, 3 * w + 7, 5000, 77, 20000]]
    clips = noise_clips(lengths, 9)
    plan = grid_plan(zafx, zafx.kaiser_bessel_derived(w))
    x, in_off, lens = zafx.pack_ragged(clips)
    offs, frames, pitch = plan.ragged_layout(lens)
    rows = plan.out_dims(0)[0]
    total = int(offs[-1]) + 64
    sentinel = np.full(total, np.nan, plan.out_dtype)
    d_in = zafx.DeviceBuffer.from_host(x, plan.device)
    d_out = zafx.DeviceBuffer.from_host(sentinel, plan.device)
    plan.execute_ragged(d_in, in_off, lens, d_out)
    plan.sync()
    assert plan.last_kernel == NATIVE
    res = d_out.download()
    real = np.zeros(total, bool)
    for o, t, p in zip(offs.tolist(), frames.tolist(), pitch.tolist()):
        block = real[o: o + rows * p].reshape(rows, p)
        block[:, :t] = True
    assert np.all(np.isfinite(res[real]))
    assert np.all(np.isnan(res[~real]))


# ------------------------------------------------------------------ 6: the routes that stay on one execute per clip
def _per_clip_cases(zafx):
    kbd = zafx.kaiser_bessel_derived
    return [
        ("compact rows", zafx.mdct_plan(kbd(2048)), lambda c: zafx.mdct_batch(c[None], kbd(2048), row_align=0)[0]),
        ("W = 4096", zafx.mdct_plan(kbd(4096), row_align=32), lambda c: zafx.mdct_batch(c[None], kbd(4096), row_align=32)[0]),
        ("W = 256", zafx.mdct_plan(kbd(256), row_align=32), lambda c: zafx.mdct_batch(c[None], kbd(256), row_align=32)[0]),
        ("TF", zafx.mdct_plan(kbd(2048), layout="TF"), lambda c: zafx.mdct_batch(c[None], kbd(2048), layout="TF")[0]),
    ]


@pytest.mark.parametrize("case", range(4))
def test_other_routes_stay_per_clip(zafx, case):
    name, plan, per_clip = _per_clip_cases(zafx)[case]
    clips = noise_clips([1, 3000, 44100, 100003, 25000], 13)
    x, in_off, lens = zafx.pack_ragged(clips)
    offs, frames, pitch = plan.ragged_layout(lens)
    rows = plan.out_dims(0)[0]
    d_in = zafx.DeviceBuffer.from_host(x, plan.device)
    d_out = zafx.DeviceBuffer((max(int(offs[-1]), 1),), plan.out_dtype, plan.device)
    plan.execute_ragged(d_in, in_off, lens, d_out)
    plan.sync()
    assert plan.last_kernel.startswith("per-clip "), (name, plan.last_kernel)
    res = d_out.download()
    for i, c in enumerate(clips):
        o, t, p = int(offs[i]), int(frames[i]), int(pitch[i])
        got = res[o: o + rows * p].reshape(rows, p)[:, :t] if plan.layout == zafx.LAYOUT_FT else res[o: o + t * rows].reshape(t, rows)
        assert np.array_equal(got, per_clip(c)), (name, i)


# ------------------------------------------------------------------ 7: the staging copy of the table
def test_back_to_back_calls_each_see_their_own_table(zafx):
    plan = grid_plan(zafx, zafx.kaiser_bessel_derived(1024))
    rng = np.random.default_rng(14)
    batches = []
    for b in range(2):
        lengths = rng.integers(0, 20000, 1024 - 300 * b).tolist()
        clips = noise_clips(lengths, 15 + b)
        x, in_off, lens = zafx.pack_ragged(clips)
        offs, frames, pitch = plan.ragged_layout(lens)
        batches.append((zafx.DeviceBuffer.from_host(x), in_off, lens, int(offs[-1])))
    outs = [zafx.DeviceBuffer((n,), plan.out_dtype) for *_, n in batches]
    expect = []
    for (d_in, in_off, lens, _), d_out in zip(batches, outs):   # one call at a time
        plan.execute_ragged(d_in, in_off, lens, d_out)
        plan.sync()
        assert plan.last_kernel == NATIVE
        expect.append(d_out.download())
        d_out.upload(np.zeros(d_out.shape, plan.out_dtype))
    for (d_in, in_off, lens, _), d_out in zip(batches, outs):   # both enqueued, no sync between them
        plan.execute_ragged(d_in, in_off, lens, d_out)
    plan.sync()
    for e, d_out in zip(expect, outs):
        assert np.array_equal(d_out.download(), e)


# ------------------------------------------------------------------ 8: the views are usable as they lie
@pytest.mark.parametrize("w", WINDOWS)
def test_round_trip_through_the_inverse(zafx, oracle_cases, w):
    window, lengths, clips, refs, got, kernel = oracle_cases[w, "edge"]
    assert kernel == NATIVE
    for i in (7, 8, 9):   # 31 M + 1, 63 M + 1 and 44100 samples
        n = lengths[i]
        y = zafx.imdct_batch(got[i][None], window)[0][:n]
        assert len(y) == n
        err = float(np.max(np.abs(y - clips[i])))
        assert err < TOL_ROUND_TRIP, (i, n, err)
