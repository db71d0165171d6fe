"""The stereo mask filter on the GPU (k_maskfilter_stereo; zafx_execute_masked_stereo, zafx_execute_masked_stereo_ragged): parity with the
reference's composition around masks of the caller's on either channel (tests/golden/maskfilter_stereo.npz) and with the float64 oracle at
the block edges, cross-checks against the mono kind and the center extraction, the same bits for a clip alone, anywhere in a batch, cut into
segments, in a ragged batch and under other compute-unit counts, the rest, containment of non-finite values, NaN-filled arenas at bases 4
bytes off the 8-byte grid, the refusals and the plan's allocations.

Bound: max|y - ref| <= 1e-5 max(max|ref|, max|x|), the level taken over both channels -- the project's TOL_FFT on mask_error.  H = W/2 is a
block, frame t covers sample frames (t - 1) H .. (t + 1) H - 1 and contributes to output blocks t - 1 and t; the two channels of a frame share
a transform."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from maskfilter_stereo_oracle import MASK_KINDS, TOL_FFT, golden_cases, make_stereo_masks, mask_error, mask_frames, oracle_maskfilter_stereo, stereo_error

pytestmark = pytest.mark.gpu

WINDOWS = (256, 512, 1024, 2048)
FILL = 0x7FC5A5A5   # a quiet NaN no kernel computes
SENTINEL = 0xC640E400   # -12345.0 as float32 bits: the pre-fill of an output no refused or skipped call may touch


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clip(seed, n):
    return np.random.default_rng([606, seed, n]).standard_normal((n, 2)).astype(np.float32)


def channels_of(m, batched=True):
    return 1 if np.ndim(m) == (3 if batched else 2) else 2


def tf_clip(m):
    """The masks of ONE clip, (W/2 + 1, T) or (2, W/2 + 1, T), as the device reads them: (T, W/2 + 1) or (T, 2, W/2 + 1) float32, compact;
    tf_batch: the same for a batch."""
    m = np.asarray(m, np.float32)
    return np.ascontiguousarray(m.T if m.ndim == 2 else m.transpose(2, 0, 1))


def tf_batch(m):
    m = np.asarray(m, np.float32)
    return np.ascontiguousarray(m.transpose(0, 2, 1) if m.ndim == 3 else m.transpose(0, 3, 1, 2))


def plan_of(wl, rest=False, layout="TF"):
    import zafx
    return zafx.maskfilter_plan(zafx.hamming(wl), rest=rest, layout=layout)


def run_plan(x, m, wl, rest=False):
    """The raw plan on device buffers: x (B, N, 2) float32, m (B, W/2 + 1, T) or (B, 2, W/2 + 1, T) -> the plan's whole output array."""
    import zafx
    plan = plan_of(wl, rest)
    b, n = x.shape[:2]
    mc = channels_of(m)
    d_in, d_mask = zafx.DeviceBuffer.from_host(np.ascontiguousarray(x, np.float32)), zafx.DeviceBuffer.from_host(tf_batch(m))
    d_out = zafx.DeviceBuffer(plan.stereo_out_shape(b, n), np.float32)
    try:
        assert d_mask.shape == plan.stereo_mask_shape(b, n, mc)
        plan.execute_masked_stereo(d_in, d_mask, d_out, b, n, mc)
        plan.sync()
        assert plan.last_kernel == "k_maskfilter_stereo" and plan.kernel_name == "k_maskfilter"
        return d_out.download()
    finally:
        for buf in (d_in, d_mask, d_out):
            buf.free()


def check(y, ref, x, what):
    err = stereo_error(y, ref, x)
    print(f"{what}: {err:.3e} of the level")
    assert np.isfinite(np.asarray(y)).all() and err <= TOL_FFT, (what, err)
    return err


class View:
    """`count` elements of `dtype` at byte `offset` of a DeviceBuffer (nothing to free)."""

    def __init__(self, buf, offset, count, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        self.ptr, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + offset), self.dtype.itemsize * count, (count,)


# ------------------------------------------------------------------------------------------------------------------ 1. golden
def test_golden_parity():
    import zafx
    for wl, n, x, m, y2, y1 in golden_cases():
        w = zafx.hamming(wl)
        for masks, ref in ((m, y2), (m[0], y1)):
            mc = masks.ndim - 1
            y = zafx.maskfilter_stereo(x, w, wl // 2, masks)
            assert y.dtype == np.float64 and y.shape == (n, 2)
            check(y, ref, x, f"maskfilter_stereo W={wl} N={n} mask_channels={mc}")
            yb = zafx.maskfilter_stereo_batch(x[None], w, masks[None])
            assert yb.dtype == np.float32 and yb.shape == (1, n, 2)
            check(yb[0], ref, x, f"maskfilter_stereo_batch W={wl} N={n} mask_channels={mc}")
            assert plan_of(wl).last_kernel == "k_maskfilter_stereo"
            yt = zafx.maskfilter_stereo_batch(x[None], w, tf_clip(masks)[None], layout="TF")
            assert np.array_equal(bits(yt), bits(yb)), (wl, mc, "FT and TF host layouts")
            yr, rr = zafx.maskfilter_stereo_batch(x[None], w, masks[None], step_length=wl // 2, rest=True)
            assert yr.shape == rr.shape == (1, n, 2) and yr.base is rr.base and np.array_equal(bits(yr), bits(yb))
            check(rr[0], x.astype(np.float64) - ref, x, f"rest W={wl} N={n} mask_channels={mc}")
            (ys,) = zafx.maskfilter_stereo_ragged([x], w, [masks])
            assert plan_of(wl).last_kernel == "k_maskfilter_stereo_ragged"
            assert ys.shape == (n, 2) and np.array_equal(bits(ys), bits(yb[0])), (wl, mc, "ragged")


# ------------------------------------------------------------------------------------------------------------------ 2. oracle at the edges
def edge_lengths(wl):
    h = wl // 2
    return [1, h - 1, h, h + 1, wl, 3 * h + 7]


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("wl", WINDOWS)
def test_oracle_parity_at_the_edges(wl, channels):
    import zafx
    w = zafx.hamming(wl)
    worst = 0.0
    for n in edge_lengths(wl):
        x = np.stack([clip(k, n) for k in range(len(MASK_KINDS))])
        m = np.stack([make_stereo_masks(kind, wl, n, channels) for kind in MASK_KINDS])
        y = run_plan(x, m, wl)
        both = zafx.maskfilter_stereo_batch(x, w, m), zafx.maskfilter_stereo_batch(x, w, tf_batch(m), layout="TF")
        assert np.array_equal(bits(both[0]), bits(y)) and np.array_equal(bits(both[1]), bits(y)), (wl, n)
        for k, kind in enumerate(MASK_KINDS):
            worst = max(worst, check(y[k], oracle_maskfilter_stereo(x[k], w, m[k]), x[k], f"W={wl} N={n} {kind} mask_channels={channels}"))
    print(f"W={wl} mask_channels={channels}: worst {worst:.3e}")


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("wl", WINDOWS)
def test_a_quiet_channel_beside_a_loud_one(wl, channels):
    """L = noise beside R = zeros, and L at unit level beside R at -90 dB: both channels are held to the one bound, whose level is the loud
    channel's; the cross-talk into the quiet channel is printed."""
    import zafx
    w, h = zafx.hamming(wl), wl // 2
    n = 9 * h + 3
    m = make_stereo_masks("unit", wl, n, channels, seed=3)
    for name, scale in (("R = zeros", 0.0), ("R at -90 dB", 10 ** (-90 / 20))):
        x = clip(70, n)
        x[:, 1] *= np.float32(scale)
        y = run_plan(x[None], m[None], wl)[0]
        ref = oracle_maskfilter_stereo(x, w, m)
        talk = np.abs(y[:, 1] - ref[:, 1]).max() / np.abs(x).max()
        print(f"W={wl} mask_channels={channels} {name}: cross-talk into R {talk:.3e} of the loud level")
        check(y, ref, x, f"W={wl} mask_channels={channels} {name}")
        for c in (0, 1):
            assert np.abs(y[:, c] - ref[:, c]).max() <= TOL_FFT * max(np.abs(ref).max(), np.abs(x).max()), (wl, channels, name, c)


# ------------------------------------------------------------------------------------------------------------------ 3. cross-checks
@pytest.mark.parametrize("wl", WINDOWS)
def test_shared_mask_against_the_mono_kind(wl):
    """Channel c of the shared-mask result against maskfilter_batch of the planar channel with the same mask: within the bound, not bitwise."""
    import zafx
    w, h = zafx.hamming(wl), wl // 2
    n = 9 * h + 3
    x = clip(80, n)
    m = make_stereo_masks("unit", wl, n, 1, seed=4)
    y = run_plan(x[None], m[None], wl)[0]
    mono = zafx.maskfilter_batch(np.ascontiguousarray(x.T), w, np.stack([m, m]))
    level = max(np.abs(mono).max(), np.abs(x).max())
    for c in (0, 1):
        err = np.abs(y[:, c].astype(np.float64) - mono[c]).max() / level
        print(f"W={wl} channel {c}: {err:.3e} of the level from k_maskfilter")
        assert err <= TOL_FFT, (wl, c, err)


@pytest.mark.parametrize("wl", WINDOWS)
def test_per_channel_masks_reproduce_the_center(wl):
    """Fed the float64 masks of the center extraction's composition (tests/center_oracle.py) on noise -- no silent bins --, the per-channel
    form reproduces oracle_center's center."""
    import zafx
    from center_oracle import oracle_center
    from oracle import zaf_oracle as orc
    w, h = zafx.hamming(wl), wl // 2
    n = 9 * h + 3
    x = clip(81, n)
    s = [orc.stft(x[:, c].astype(np.float64), w, h) for c in (0, 1)]
    a, b = np.abs(s[0][:h + 1]), np.abs(s[1][:h + 1])
    assert a.min() > 0 and b.min() > 0
    m = np.stack([np.where(b < a, b / a, 1.0), np.where(a < b, a / b, 1.0)])
    y = run_plan(x[None], m[None], wl)[0]
    check(y, oracle_center(x, w), x, f"W={wl} the center's masks handed in")


# ------------------------------------------------------------------------------------------------------------------ 4. the same bits anywhere
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("wl", WINDOWS)
def test_a_clip_has_the_same_bits_anywhere(wl, channels):
    """The clip of 60 blocks + 5 sample frames (several tiles: the carry is handed on) alone -- a batch too small for the device, so it is cut
    into segments --, as the first, a middle and the last clip of batches of 2, 3 and 5, and in a ragged batch beside clips of 5 and 20 H."""
    import zafx
    from maskfilter_stereo_probe import probe_case, ragged_of
    w = zafx.hamming(wl)
    x, m = probe_case(wl, channels)
    alone = run_plan(x[2:3], m[2:3], wl)[0]
    check(alone, oracle_maskfilter_stereo(x[2], w, m[2]), x[2], f"W={wl} mask_channels={channels} the 60-block clip")
    for order in ([2, 0], [0, 2], [2, 1, 0], [1, 2, 0], [0, 1, 2], [2, 0, 1, 3, 0], [0, 1, 2, 3, 1], [3, 1, 0, 0, 2]):
        out = run_plan(x[order], m[order], wl)
        assert np.array_equal(bits(out[order.index(2)]), bits(alone)), (wl, order)
    clips, masks = ragged_of(x, m, wl)
    ys = zafx.maskfilter_stereo_ragged(clips, w, masks)
    assert np.array_equal(bits(ys[1]), bits(alone)), (wl, "ragged")


@pytest.mark.parametrize("channels", [1, 2])
def test_whole_clips_give_the_bits_of_segments(channels):
    """In a batch of as many clips as the device has workgroup slots the clips stay whole; alone the clip is cut."""
    from maskfilter_stereo_probe import probe_case
    wl = 256
    x, m = probe_case(wl, channels)
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
    from maskfilter_stereo_probe import WINDOWS as PROBE_WINDOWS, probe_case
    path = str(tmp_path / "probe.npz")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maskfilter_stereo_probe.py"), path], env=dict(os.environ, ZAFX_COMPUTE_UNITS=str(units)),
                         capture_output=True, timeout=240)
    assert res.returncode == 0 and b"probe ok" in res.stdout, res.stderr.decode()[-2000:]
    got = np.load(path)
    for wl in PROBE_WINDOWS:
        assert int(got[f"units{wl}"]) == units and plan_of(wl).compute_units > units
        for ch in (1, 2):
            x, m = probe_case(wl, ch)
            here = run_plan(x[2:3], m[2:3], wl)[0]
            for name in ("alone", "batch", "ragged"):
                assert np.array_equal(bits(got[f"{name}{wl}_{ch}"]), bits(here)), (wl, ch, name)


# ------------------------------------------------------------------------------------------------------------------ 5. rest
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("wl", WINDOWS)
def test_rest(wl, channels):
    h = wl // 2
    for n in (1, 3 * h + 7, 20 * h + 5):
        x = np.stack([clip(10 + k, n) for k in range(3)])
        m = np.stack([make_stereo_masks("unit", wl, n, channels, seed=k) for k in range(3)])
        both, only = run_plan(x, m, wl, rest=True), run_plan(x, m, wl)
        assert both.shape == (3, 2, n, 2)
        assert np.array_equal(bits(both[:, 0]), bits(only)), (wl, n)
        assert np.array_equal(bits(both[:, 1]), bits(x - both[:, 0])), (wl, n)


@pytest.mark.parametrize("wl", WINDOWS)
def test_fixed_values(wl):
    """A mask of zeros gives exact zeros (and the rest the input's bits); silence on both channels gives zeros under any finite mask."""
    h = wl // 2
    n = 9 * h + 3
    x = np.stack([clip(20 + k, n) for k in range(2)])
    t = mask_frames(n, wl)
    for channels in (1, 2):
        shape = (2, h + 1, t) if channels == 1 else (2, 2, h + 1, t)
        out = run_plan(x, np.zeros(shape, np.float32), wl, rest=True)
        assert not out[:, 0].any() and np.array_equal(bits(out[:, 1]), bits(x))
        wide = np.stack([make_stereo_masks("signed_wide", wl, n, channels, seed=k) for k in range(2)])
        assert not run_plan(np.zeros_like(x), wide, wl, rest=True).any()


# ------------------------------------------------------------------------------------------------------------------ 6. containment
def blocks_mask(n, h, blocks):
    """The sample frames of a clip of n that output blocks `blocks` cover."""
    hit = np.zeros(n, bool)
    for b in blocks:
        if b >= 0:
            hit[min(b * h, n):min((b + 1) * h, n)] = True
    return hit


def run_ragged_simple(clips, masks, wl):
    import zafx
    return zafx.maskfilter_stereo_ragged(clips, zafx.hamming(wl), masks)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("wl", [256, 2048])
def test_containment(wl, channels, ragged):
    """Clip 1 of three.  A NaN sample in ONE channel, in block b, may make only blocks b - 1 .. b + 1 non-finite, of either channel; a NaN
    and a +inf mask value at frames j may make only blocks j - 1 and j non-finite; every other output element -- the other clips whole --
    keeps the clean run's bits.  Finite arithmetic on NaN data."""
    h = wl // 2
    n = 20 * h + 9
    x = np.stack([clip(30 + k, n) for k in range(3)])
    m = np.stack([make_stereo_masks("unit", wl, n, channels, seed=30 + k) for k in range(3)])

    def run(xs, ms):
        if ragged:
            return np.stack(run_ragged_simple(list(xs), list(ms), wl))
        return run_plan(xs, ms, wl)
    clean = run(x, m)
    assert np.isfinite(clean).all()
    s, b = 5 * h + 17, 5                     # sample frame s lies in block 5: frames 5 and 6
    tn, ti = 13, 17                          # the NaN mask value in frame 13, the +inf one in frame 17
    xp, mp = x.copy(), m.copy()
    xp[1, s, 1] = np.nan                     # the right channel only
    mp[(1, h // 3, tn) if channels == 1 else (1, 0, h // 3, tn)] = np.nan   # (with a mask per channel: the left channel's only)
    mp[(1, h // 5, ti) if channels == 1 else (1, 1, h // 5, ti)] = np.inf   # (... the right channel's only)
    got = run(xp, mp)
    for c in (0, 2):
        assert np.array_equal(bits(got[c]), bits(clean[c])), (wl, c)
    may = blocks_mask(n, h, [b - 1, b, b + 1, tn - 1, tn, ti - 1, ti])
    assert not np.isfinite(got[1][may]).all() and np.isfinite(got[1][~may]).all()
    assert np.array_equal(bits(got[1][~may]), bits(clean[1][~may])) and 0 < may.sum() < n
    # the NaN of one channel is seen in the other: the packing's cross-channel consequence, stated in the header
    print(f"W={wl} mask_channels={channels} ragged={ragged}: non-finite L {int((~np.isfinite(got[1][:, 0])).sum())}, R {int((~np.isfinite(got[1][:, 1])).sum())} of {n}")


# ------------------------------------------------------------------------------------------------------------------ 7, 8. ragged, arena
def ragged_lengths(wl):
    h = wl // 2
    return [0, 1, h, 3 * h + 7, 60 * h + 5, 20 * h]


def batch_of(wl, lengths, channels, seed=0):
    return [clip(seed + i, n) for i, n in enumerate(lengths)], [make_stereo_masks("unit", wl, n, channels, seed=seed + i) for i, n in enumerate(lengths)]


def place(sizes, gap, base):
    """-> (offsets, total): blocks of `sizes` elements, `gap` elements between them, the first at element `base`, `gap` + 1 behind the last."""
    offs, at = [], base
    for s in sizes:
        offs.append(at)
        at += s + gap
    return np.array(offs, np.int64), at + 1


def run_ragged(plan, clips, masks, channels, gap=0, byte_bases=(0, 0, 0)):
    """One zafx_execute_masked_stereo_ragged: sample frames, masks and output blocks each inside an arena -- NaN words around the clips and the
    masks, SENTINEL words in the output --, `gap` elements between neighbours (sample frames; float32 words for the masks), the three arrays
    `byte_bases` bytes into their allocations.  -> (the per-clip results (blocks, N_i, 2), after checking every other output word kept SENTINEL)."""
    import zafx
    blocks = 2 if plan.kind == zafx.MASKFILTER_REST else 1
    lengths = np.array([len(c) for c in clips], np.int64)
    flat = [tf_clip(m).ravel() for m in masks]
    in_offs, in_frames = place(lengths.tolist(), gap, 0)
    mask_offs, mask_words = place([len(f) for f in flat], gap, 0)
    out_offs, out_frames = place((blocks * lengths).tolist(), gap, 0)
    pad = [b // 4 for b in byte_bases]
    assert all(b % 4 == 0 for b in byte_bases)
    h_in, h_mask = np.full(pad[0] + 2 * in_frames, FILL, np.uint32), np.full(pad[1] + mask_words, FILL, np.uint32)
    for c, o in zip(clips, in_offs.tolist()):
        h_in[pad[0] + 2 * o:pad[0] + 2 * (o + len(c))] = bits(c).ravel()
    for f, o in zip(flat, mask_offs.tolist()):
        h_mask[pad[1] + o:pad[1] + o + len(f)] = f.view(np.uint32)
    h_out = np.full(pad[2] + 2 * out_frames, SENTINEL, np.uint32)
    bufs = [zafx.DeviceBuffer.from_host(a) for a in (h_in, h_mask, h_out)]
    views = [View(bufs[0], byte_bases[0], 2 * in_frames), View(bufs[1], byte_bases[1], mask_words), View(bufs[2], byte_bases[2], 2 * out_frames)]
    try:
        plan.execute_masked_stereo_ragged(views[0], in_offs, lengths, views[1], mask_offs, views[2], out_offs, channels)
        plan.sync()
        if len(lengths):
            assert plan.last_kernel == "k_maskfilter_stereo_ragged" and plan.kernel_name == "k_maskfilter"
        words = bufs[2].download()
    finally:
        for b in bufs:
            b.free()
    kept = np.ones(len(words), bool)
    res = []
    for o, n in zip((2 * out_offs + pad[2]).tolist(), lengths.tolist()):
        kept[o:o + 2 * blocks * n] = False
        res.append(words[o:o + 2 * blocks * n].view(np.float32).reshape(blocks, n, 2))
    assert (words[kept] == SENTINEL).all(), "written outside the clips' blocks"
    return res


_ALONE = {}


def alone(wl, rest, x, m, key):
    key = (wl, rest) + tuple(key)
    if key not in _ALONE:
        _ALONE[key] = run_plan(x[None], m[None], wl, rest=rest)[0].reshape(2 if rest else 1, len(x), 2)
    return _ALONE[key]


def assert_equal_alone(res, clips, masks, wl, rest, channels, seed, what=""):
    for i, (r, x, m) in enumerate(zip(res, clips, masks)):
        if not len(x):
            assert r.size == 0
            continue
        assert np.array_equal(bits(r), bits(alone(wl, rest, x, m, (channels, seed, i)))), (what, wl, rest, channels, i, len(x))


@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("wl", WINDOWS)
def test_ragged_bitwise_against_the_clip_alone(monkeypatch, wl, channels, rest):
    clips, masks = batch_of(wl, ragged_lengths(wl), channels)
    plan = plan_of(wl, rest)
    for per_slot in (None, "1"):
        if per_slot:
            monkeypatch.setenv("ZAFX_CENTER_UNITS_PER_SLOT", per_slot)
        else:
            monkeypatch.delenv("ZAFX_CENTER_UNITS_PER_SLOT", raising=False)
        assert_equal_alone(run_ragged(plan, clips, masks, channels), clips, masks, wl, rest, channels, 0, what=f"units per slot {per_slot}")


def test_ragged_empty_batches_write_nothing():
    plan = plan_of(512, True)
    for channels in (1, 2):
        assert run_ragged(plan, [], [], channels) == []
        clips, masks = batch_of(512, [0, 0, 0], channels)
        assert all(r.size == 0 for r in run_ragged(plan, clips, masks, channels))


@pytest.mark.parametrize("channels", [1, 2])
def test_the_layout_agrees_with_the_packed_masks(channels):
    import zafx
    for wl in WINDOWS:
        h = wl // 2
        lengths = np.array(ragged_lengths(wl), np.int64)
        _, masks = batch_of(wl, lengths.tolist(), channels)
        packed, offs, mc = zafx.pack_ragged_stereo_masks(masks, lengths, wl)
        for rest in (False, True):
            mask_offs, out_offs = plan_of(wl, rest).stereo_ragged_layout(lengths, channels)
            assert mc == channels and mask_offs.tolist() == offs.tolist() and len(packed) == mask_offs[-1], (wl, rest)
            assert mask_offs.tolist() == (channels * plan_of(wl, rest).mask_ragged_layout(lengths)).tolist()
            assert out_offs.tolist() == np.concatenate(([0], np.cumsum((2 if rest else 1) * lengths))).tolist()
        for m, o, n in zip(masks, offs.tolist(), lengths.tolist()):
            t = mask_frames(n, wl)
            assert np.array_equal(packed[o:o + channels * t * (h + 1)], tf_clip(m).ravel())


@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("wl", [2048, 256])
def test_ragged_arena(wl, channels, rest):
    """Clips, masks and output blocks back to back and with gaps, NaN between the clips and between the masks, the arrays 4 bytes off the
    8-byte grid: nothing outside the blocks is written, and no clip sees its neighbour's samples or masks."""
    clips, masks = batch_of(wl, ragged_lengths(wl), channels)
    plan = plan_of(wl, rest)
    for gap, bases in ((0, (4, 4, 4)), (37, (20, 12, 36))):
        assert all(b % 8 == 4 for b in bases)
        res = run_ragged(plan, clips, masks, channels, gap=gap, byte_bases=bases)
        for r in res:
            assert np.isfinite(r).all()
        assert_equal_alone(res, clips, masks, wl, rest, channels, 0, what=f"gap {gap}")


@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
def test_arena_equal_length(channels, rest):
    """zafx_execute_masked_stereo on slices of larger buffers: the three arrays 4 bytes off the 8-byte grid, NaN around the inputs; nothing but
    the output is written."""
    import zafx
    guard = 64 * 1024
    for wl, n, deltas in ((2048, 9 * 1024 + 1, (4, 132, 20)), (256, 16 * 128 - 1, (132, 4, 68))):
        plan = plan_of(wl, rest)
        x = np.stack([clip(40 + k, n) for k in range(3)])
        m = np.stack([make_stereo_masks("unit", wl, n, channels, seed=40 + k) for k in range(3)])
        laid = tf_batch(m)
        n_out = int(np.prod(plan.stereo_out_shape(3, n)))
        arenas, views = [], []
        for data, words, delta, fill in ((bits(x), x.size, deltas[0], FILL), (laid.view(np.uint32), laid.size, deltas[1], FILL), (None, n_out, deltas[2], SENTINEL)):
            assert delta % 8 == 4
            host = np.full((2 * guard + delta) // 4 + words, fill, np.uint32)
            lo = (guard + delta) // 4
            if data is not None:
                host[lo:lo + words] = data.ravel()
            buf = zafx.DeviceBuffer.from_host(host)
            arenas.append((buf, host, lo, words))
            views.append(View(buf, guard + delta, words))
        try:
            plan.execute_masked_stereo(views[0], views[1], views[2], 3, n, channels)
            plan.sync()
            buf, host, lo, words = arenas[2]
            got = buf.download()
        finally:
            for a in arenas:
                a[0].free()
        assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + words:], host[lo + words:]), "written outside the output"
        out = got[lo:lo + words].view(np.float32).reshape(plan.stereo_out_shape(3, n))
        assert np.isfinite(out).all() and np.array_equal(bits(out), bits(run_plan(x, m, wl, rest=rest))), (wl, rest)


# ------------------------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_leave_the_output_untouched():
    import zafx
    from zafx import _lib
    lib = _lib.load()
    wl, h = 512, 256
    w = zafx.hamming(wl)
    lengths = np.array([3000, 0, 700], np.int64)
    clips, masks = batch_of(wl, lengths.tolist(), 2, seed=50)
    plan, ft_plan, stft = plan_of(wl, True), plan_of(wl, True, layout="FT"), zafx.stft_plan(w, h)
    x = np.concatenate(clips)
    in_offs = np.array([0, 3000, 3000], np.int64)
    mask_offs, out_total = plan.stereo_ragged_layout(lengths, 2)
    out_offs = 2 * in_offs
    assert out_total.tolist() == [0, 6000, 6000, 7400]
    sentinel = np.full((2 * len(x), 2), -12345.5, np.float32)
    d_in, d_out = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(sentinel)
    packed, offs, _ = zafx.pack_ragged_stereo_masks(masks, lengths, wl)
    assert offs.tolist() == mask_offs.tolist()
    d_mask = zafx.DeviceBuffer.from_host(packed)
    first = mask_frames(3000, wl) * 2 * (h + 1)   # the float32 words of clip 0's masks
    p64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731

    def ragged(pl, a_in=d_in.ptr, a_inoff=in_offs, a_len=lengths, a_mask=d_mask.ptr, a_moff=mask_offs, a_out=d_out.ptr, a_ooff=out_offs, n=3, mc=2):
        rc = lib.zafx_execute_masked_stereo_ragged(pl, a_in, None if a_inoff is None else p64(a_inoff), None if a_len is None else p64(a_len), a_mask,
                                                   None if a_moff is None else p64(a_moff), a_out, None if a_ooff is None else p64(a_ooff), n, mc)
        return rc, (lib.zafx_last_error() or b"").decode()

    def equal(pl, a_in=d_in.ptr, a_mask=d_mask.ptr, a_out=d_out.ptr, b=1, n=3000, mc=2):
        return lib.zafx_execute_masked_stereo(pl, a_in, a_mask, a_out, b, n, mc), (lib.zafx_last_error() or b"").decode()

    def neg(a, i):
        b = a.copy()
        b[i] = -1
        return b

    big1, big2 = lengths.copy(), lengths.copy()
    big1[2], big2[2] = 1 << 28, 1 << 27
    cases = [
        (dict(pl=None), "null plan"),
        (dict(a_in=None), "null device pointer"), (dict(a_mask=None), "null device pointer"), (dict(a_out=None), "null device pointer"),
        (dict(a_inoff=None), "null argument"), (dict(a_len=None), "null argument"), (dict(a_moff=None), "null argument"), (dict(a_ooff=None), "null argument"),
        (dict(n=-1), "negative number of clips"),
        (dict(a_len=neg(lengths, 1)), "of clip 1"), (dict(a_inoff=neg(in_offs, 2)), "of clip 2"), (dict(a_moff=neg(mask_offs, 0)), "of clip 0"),
        (dict(a_ooff=neg(out_offs, 2)), "of clip 2"),
        (dict(a_len=big2), "2^27 sample frames or more (not supported): clip 2"),   # by `lengths` alone: the buffers are those of the small batch
        (dict(a_len=big1, mc=1), "2^28 sample frames or more (not supported): clip 2"),
        (dict(mc=0), "mask_channels"), (dict(mc=3), "mask_channels"), (dict(mc=3, n=0), "mask_channels"),
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
                     (dict(n=1 << 27), "2^27"), (dict(n=1 << 27, b=0), "2^27"), (dict(n=1 << 28, mc=1), "2^28"), (dict(mc=0), "mask_channels"),
                     (dict(mc=3, b=0), "mask_channels"), (dict(pl=ft_plan.handle), "ZAFX_LAYOUT_TF"),
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
    one_mask = View(d_mask, 0, first)
    with pytest.raises(zafx.ZafxError, match="ZAFX_LAYOUT_TF"):
        ft_plan.execute_masked_stereo(d_in, one_mask, d_out, 1, 3000, 2)
    with pytest.raises(zafx.ZafxError, match="ZAFX_LAYOUT_TF"):
        ft_plan.execute_masked_stereo_ragged(d_in, in_offs, lengths, d_mask, mask_offs, d_out, out_offs, 2)
    with pytest.raises(zafx.ZafxError, match="MASKFILTER"):
        stft.execute_masked_stereo(d_in, one_mask, d_out, 1, 3000, 2)
    with pytest.raises(zafx.ZafxError, match="mask_channels"):
        plan.execute_masked_stereo(d_in, one_mask, d_out, 1, 3000, 3)
    with pytest.raises(ValueError, match="float32"):
        plan.execute_masked_stereo(d_in, View(d_mask, 0, first // 2, np.complex64), d_out, 1, 3000, 2)
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_stereo(d_in, d_mask, d_out, 1, 3000, 2)   # the masks of three clips for one
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_stereo(d_in, one_mask, d_out, 1, 3000, 1)   # two masks where one is asked for
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_stereo_ragged(d_in, in_offs, lengths, View(d_mask, 0, int(mask_offs[-1]) - 5), mask_offs, d_out, out_offs, 2)
    with pytest.raises(ValueError, match="d_out"):
        plan.execute_masked_stereo_ragged(d_in, in_offs, lengths, d_mask, mask_offs, View(d_out, 0, sentinel.size - 1), out_offs, 2)
    with pytest.raises(ValueError, match="d_in"):
        plan.execute_masked_stereo_ragged(View(d_in, 0, x.size - 1), in_offs, lengths, d_mask, mask_offs, d_out, out_offs, 2)
    with pytest.raises(ValueError, match="one entry per clip"):
        plan.execute_masked_stereo_ragged(d_in, in_offs[:2], lengths, d_mask, mask_offs, d_out, out_offs, 2)
    with pytest.raises(zafx.ZafxError, match="zafx_execute_masked"):
        plan.execute(d_in, d_out, 1, 3000)
    for p in (plan, ft_plan, stft):
        p.sync()
    assert np.array_equal(bits(d_out.download()), bits(sentinel))
    # the same arguments unharmed are accepted
    rc, msg = ragged(plan.handle)
    assert rc == 0, msg
    plan.sync()
    assert plan.last_kernel == "k_maskfilter_stereo_ragged"
    rc, msg = equal(plan.handle)
    assert rc == 0, msg
    plan.sync()
    assert plan.last_kernel == "k_maskfilter_stereo"
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
        for channels in (1, 2):
            clips, masks = batch_of(wl, [3 * h + 7, 0, 30 * h], channels, seed=70)
            p = zafx.Plan(kind, window_length=wl, step_length=h, layout="TF")
            p.set_window(zafx.hamming(wl))
            res = run_ragged(p, clips, masks, channels)
            assert all(np.isfinite(r).all() for r in res)
            plans.append(p)
    assert live() > before
    for p in plans:
        p.destroy()
    assert live() == before
