"""Ragged batches of the mask filter on the GPU (k_maskfilter's RAGGED form; zafx_execute_masked_ragged, zafx_plan_mask_ragged_layout): every
clip bit for bit what zafx_execute_masked gives it alone -- at every window, with and without the rest, in every mask layout, cut into
units, dealt over fewer workgroups than units, on one compute unit, permuted, inside NaN-filled arenas --, parity with the reference's
composition (tests/golden/maskfilter.npz) within the project's TOL_FFT = 1e-5 on mask_error, the mask layout shared with a ragged |X| STFT,
two calls in flight on one plan, the refusals and the Python functions.

H = W/2 is a block; F (maskfilter_tile_transforms) packed transforms make a tile; the cutter cuts a clip of more than 4 F - 3 block pairs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from maskfilter_oracle import TOL_FFT, golden_cases, make_mask, mask_error, mask_frames

pytestmark = pytest.mark.gpu

WINDOWS = (256, 512, 1024, 2048)
LAYOUTS = (("FT", 0), ("FT", 32), ("TF", 0))   # (layout, row_align)
FILL = 0x7FC5A5A5   # a quiet NaN no kernel computes (tests/test_gpu_maskfilter.py)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clip(seed, n):
    return np.random.default_rng([404, seed, n]).standard_normal(n).astype(np.float32)


def lengths_of(h):
    """About 12 clips: 0, 1, around one and two blocks, an odd (7) and an even (8) block count, an odd frame count (8 blocks: 9 frames), 14, 60 and
    almost 61 blocks."""
    return [0, 1, h - 1, h, h + 1, 2 * h, 2 * h + 1, 7 * h - 2, 7 * h + 5, 14 * h, 60 * h, 61 * h - 3, 0]


def batch_of(wl, lengths, seed=0):
    return [clip(seed + i, n) for i, n in enumerate(lengths)], [make_mask("unit", wl, n, seed=seed + i) for i, n in enumerate(lengths)]


def laid(plan, m, n, pad=np.nan):
    """One clip's mask (W/2 + 1, T) as the plan reads it, flat: rows at the plan's pitch with `pad` in the padding, or (T, W/2 + 1)."""
    import zafx
    if plan.layout == zafx.LAYOUT_TF:
        return np.ascontiguousarray(m.T, np.float32).ravel()
    out = np.full((m.shape[0], plan.row_pitch(n)), pad, np.float32)
    out[:, :m.shape[1]] = m
    return out.ravel()


class View:
    """`count` float32 at word `first` of a DeviceBuffer of 32-bit words (nothing to free)."""

    def __init__(self, buf, first, count):
        self.ptr, self.dtype, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + 4 * first), np.dtype(np.float32), 4 * count, (count,)


def place(sizes, gap, base):
    """-> (offsets, words): blocks of `sizes` words, `gap` words between them, the first at word `base`, `gap` words behind the last."""
    offs, at = [], base
    for s in sizes:
        offs.append(at)
        at += s + gap
    return np.array(offs, np.int64), at + 1


_ALONE = {}


def alone(wl, rest, layout, row_align, x, m, key=None):
    """zafx_execute_masked on one clip and its mask alone: the (2, N) or (N,) result.  `key`: the clip's name in the cache of this module."""
    import zafx
    key = key and (wl, rest, layout, row_align) + tuple(key)
    if key in _ALONE:
        return _ALONE[key]
    n = len(x)
    plan = zafx.maskfilter_plan(zafx.hamming(wl), rest=rest, layout=layout, row_align=row_align)
    d_in, d_mask = zafx.DeviceBuffer.from_host(x[None]), zafx.DeviceBuffer.from_host(laid(plan, m, n).reshape(plan.mask_shape(1, n)))
    d_out = zafx.DeviceBuffer(plan.out_shape(1, n), np.float32)
    try:
        plan.execute_masked(d_in, d_mask, d_out, 1, n)
        plan.sync()
        assert plan.last_kernel == "k_maskfilter"
        res = d_out.download()[0]
    finally:
        for b in (d_in, d_mask, d_out):
            b.free()
    if key:
        _ALONE[key] = res
    return res


def run_ragged(plan, clips, masks, gap=0, bases=(0, 0, 0), sync=True):
    """One zafx_execute_masked_ragged over the clips, every array inside an arena of FILL words: `gap` words between the clips, between the masks
    and between the output blocks, the three arrays at words `bases`.  -> (the output arena's words, out_offsets, lengths, the buffers)."""
    import zafx
    blocks = 2 if plan.kind == zafx.MASKFILTER_REST else 1
    lengths = np.array([len(c) for c in clips], np.int64)
    flat = [laid(plan, m, len(c)) for c, m in zip(clips, masks)]
    in_offs, in_words = place(lengths.tolist(), gap, bases[0])
    mask_offs, mask_words = place([len(f) for f in flat], gap, bases[1])
    out_offs, out_words = place((blocks * lengths).tolist(), gap, bases[2])
    h_in, h_mask = np.full(in_words, FILL, np.uint32), np.full(mask_words, FILL, np.uint32)
    for c, o in zip(clips, in_offs.tolist()):
        h_in[o:o + len(c)] = bits(c)
    for f, o in zip(flat, mask_offs.tolist()):
        h_mask[o:o + len(f)] = bits(f)
    bufs = [zafx.DeviceBuffer.from_host(h_in), zafx.DeviceBuffer.from_host(h_mask), zafx.DeviceBuffer.from_host(np.full(out_words, FILL, np.uint32))]
    views = [View(b, 0, b.shape[0]) for b in bufs]
    plan.execute_masked_ragged(views[0], in_offs, lengths, views[1], mask_offs, views[2], out_offs)
    if not sync:
        return None, out_offs, lengths, bufs
    try:
        plan.sync()
        assert plan.last_kernel == "k_maskfilter_ragged" and plan.kernel_name == "k_maskfilter"
        return bufs[2].download(), out_offs, lengths, None
    finally:
        for b in bufs:
            b.free()


def results(words, out_offs, lengths, blocks):
    """The per-clip results of an output arena, (blocks, N_i) float32 each, after checking that every word outside them kept the fill."""
    kept = np.ones(len(words), bool)
    res = []
    for o, n in zip(out_offs.tolist(), lengths.tolist()):
        kept[o:o + blocks * n] = False
        res.append(words[o:o + blocks * n].view(np.float32).reshape(blocks, n))
    assert (words[kept] == FILL).all(), "written outside the clips"
    return res


def plan_of(wl, rest, layout="FT", row_align=0):
    import zafx
    return zafx.maskfilter_plan(zafx.hamming(wl), rest=rest, layout=layout, row_align=row_align)


def assert_equal_alone(res, clips, masks, wl, rest, layout, row_align, keys=None, what=""):
    for i, (r, x, m) in enumerate(zip(res, clips, masks)):
        if not len(x):
            assert r.size == 0
            continue
        ref = alone(wl, rest, layout, row_align, x, m, keys and keys[i]).reshape(r.shape)
        assert np.array_equal(bits(r), bits(ref)), (what, wl, rest, layout, row_align, i, len(x))


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("wl", WINDOWS)
def test_bitwise_against_the_clip_alone(wl, rest):
    lengths = lengths_of(wl // 2)
    clips, masks = batch_of(wl, lengths)
    for layout, row_align in LAYOUTS:
        plan = plan_of(wl, rest, layout, row_align)
        words, out_offs, lens, _ = run_ragged(plan, clips, masks)
        res = results(words, out_offs, lens, 2 if rest else 1)
        assert_equal_alone(res, clips, masks, wl, rest, layout, row_align, keys=[(0, i) for i in range(len(clips))])


# ------------------------------------------------------------------------------------------------------------------ 2
def test_cut_clips_and_more_units_than_workgroups():
    from maskfilter_ragged_probe import probe_batch
    for which, layouts in (("cut", LAYOUTS), ("short", LAYOUTS[:1])):
        wl, clips, masks = probe_batch(which)
        for layout, row_align in layouts:
            words, out_offs, lens, _ = run_ragged(plan_of(wl, True, layout, row_align), clips, masks)
            assert_equal_alone(results(words, out_offs, lens, 2), clips, masks, wl, True, layout, row_align, what=which)


def test_more_units_than_workgroups_at_one_workgroup_per_compute_unit():
    """600 clips of 1 - 6 blocks at W = 2048 / FT, where one workgroup fits a compute unit: the rounds of the deal run forwards and backwards."""
    wl = 2048
    g = np.random.default_rng(601)
    lengths = (g.integers(0, 6, 600) * 1024 + g.integers(1, 1025, 600)).tolist()
    clips, masks = batch_of(wl, lengths, seed=1000)
    plan = plan_of(wl, False)
    assert plan.compute_units < 600
    words, out_offs, lens, _ = run_ragged(plan, clips, masks)
    assert_equal_alone(results(words, out_offs, lens, 1), clips, masks, wl, False, "FT", 0)


@pytest.mark.timeout(300)
def test_one_compute_unit_gives_the_same_bits(tmp_path):
    """The cut clips and the 600 short ones in a fresh child process with ZAFX_COMPUTE_UNITS=1: other cuts, every unit on a few workgroups."""
    import zafx
    from maskfilter_ragged_probe import BATCHES, probe_batch
    path = str(tmp_path / "probe.npz")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maskfilter_ragged_probe.py"), path], env=dict(os.environ, ZAFX_COMPUTE_UNITS="1"),
                         capture_output=True, timeout=240)
    assert res.returncode == 0 and b"probe ok" in res.stdout, res.stderr.decode()[-2000:]
    got = np.load(path)
    for which in BATCHES:
        wl, clips, masks = probe_batch(which)
        w = zafx.hamming(wl)
        assert int(got[f"units_{which}"]) == 1 and zafx.maskfilter_plan(w, rest=True).compute_units > 1
        here = np.concatenate([np.concatenate(pair) for pair in zafx.maskfilter_ragged(clips, w, masks, rest=True)])
        assert np.array_equal(bits(got[which]), bits(here)), which


# ------------------------------------------------------------------------------------------------------------------ 3
def test_oracle_parity():
    """The cases of tests/golden/maskfilter.npz, one ragged batch per window (the stored clip between two others): y within TOL_FFT of the stored
    one, the rest exactly x - y of the written y."""
    for wl, n, x, m, ref in golden_cases():
        h = wl // 2
        clips, masks = batch_of(wl, [3 * h + 1, 0, 17 * h], seed=50)
        clips.insert(1, x), masks.insert(1, m)
        for layout, row_align in LAYOUTS:
            for rest in (False, True):
                words, out_offs, lens, _ = run_ragged(plan_of(wl, rest, layout, row_align), clips, masks)
                res = results(words, out_offs, lens, 2 if rest else 1)
                err = mask_error(res[1][0], ref, x)
                print(f"W={wl} N={n} {layout}/{row_align} rest={rest}: {err:.3e} of the level")
                assert np.isfinite(res[1]).all() and err <= TOL_FFT, (wl, layout, row_align, rest, err)
                if rest:
                    for r, c in zip(res, clips):
                        assert np.array_equal(bits(r[1]), bits(c - r[0])), (wl, layout, row_align)


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("layout, row_align", LAYOUTS)
def test_writes_nothing_but_the_clips(layout, row_align, rest):
    """Clips, masks and output blocks with gaps between them, inside arenas of NaN words; the masks start 4 bytes behind a 128-byte line and carry NaN
    in their pad columns.  Every output word outside the clips keeps the fill; the results are finite and those of the compact run."""
    for wl in (2048, 256):
        clips, masks = batch_of(wl, lengths_of(wl // 2))
        plan = plan_of(wl, rest, layout, row_align)
        blocks = 2 if rest else 1
        compact = results(*run_ragged(plan, clips, masks)[:3], blocks)
        words, out_offs, lens, _ = run_ragged(plan, clips, masks, gap=37, bases=(35, 32 * 3 + 1, 33))
        spread = results(words, out_offs, lens, blocks)
        for a, b in zip(spread, compact):
            assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b)), (wl, layout, row_align)


# ------------------------------------------------------------------------------------------------------------------ 5
def test_permutation():
    wl = 512
    clips, masks = batch_of(wl, lengths_of(wl // 2), seed=7)
    perm = np.random.default_rng(8).permutation(len(clips)).tolist()
    for layout, row_align in LAYOUTS:
        plan = plan_of(wl, True, layout, row_align)
        straight = results(*run_ragged(plan, clips, masks)[:3], 2)
        permuted = results(*run_ragged(plan, [clips[i] for i in perm], [masks[i] for i in perm])[:3], 2)
        for k, i in enumerate(perm):
            assert np.array_equal(bits(permuted[k]), bits(straight[i])), (layout, k, i)


# ------------------------------------------------------------------------------------------------------------------ 5b
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
    """A NaN sample and a NaN mask value in one clip of a ragged batch, in every mask layout, with the rest: every other clip has the bits of its
    run alone and of the clean batch; inside that clip only the samples of the frames that hold the NaN sample or mask value, and of the frames
    paired with them, may be non-finite -- every other sample has the bits of the clean run."""
    h = wl // 2
    n = 20 * h + 9
    lengths = [7 * h + 3, 0, n, 1, 20 * h + 9]
    clips, masks = batch_of(wl, lengths, seed=80)
    s, (k, t), at = 5 * h + 17, (h // 3, 13), 2   # sample s lies in frames 5 and 6; the mask value in frame 13
    bad_clips, bad_masks = [c.copy() for c in clips], [m.copy() for m in masks]
    bad_clips[at][s] = np.nan
    bad_masks[at][k, t] = np.nan
    may = touched(n, h, [s // h, s // h + 1, t])
    assert 0 < may.sum() < n
    for layout, row_align in LAYOUTS:
        plan = plan_of(wl, True, layout, row_align)
        clean = results(*run_ragged(plan, clips, masks)[:3], 2)
        got = results(*run_ragged(plan, bad_clips, bad_masks)[:3], 2)
        others = [i for i in range(len(clips)) if i != at]
        assert_equal_alone([got[i] for i in others], [clips[i] for i in others], [masks[i] for i in others], wl, True, layout, row_align, what="containment")
        for i in others:
            assert np.array_equal(bits(got[i]), bits(clean[i])), (wl, layout, row_align, i)
        for j in range(2):
            assert not np.isfinite(got[at][j][may]).all() and np.isfinite(got[at][j][~may]).all(), (wl, layout, row_align, j)
            assert np.array_equal(bits(got[at][j][~may]), bits(clean[at][j][~may])), (wl, layout, row_align, j)


# ------------------------------------------------------------------------------------------------------------------ 6
def test_back_to_back_calls_each_see_their_own_table():
    wl = 1024
    h = wl // 2
    a = batch_of(wl, [5 * h + 3, 1, 40 * h, 2 * h], seed=20)
    b = batch_of(wl, [70 * h - 1, 0, 3 * h, h + 1, 9 * h, 2], seed=30)
    plan = plan_of(wl, True)
    first = run_ragged(plan, *a, sync=False)
    second = run_ragged(plan, *b, sync=False)
    try:
        plan.sync()
        assert plan.last_kernel == "k_maskfilter_ragged"
        got = [results(r[3][2].download(), r[1], r[2], 2) for r in (first, second)]
    finally:
        for r in (first, second):
            for buf in r[3]:
                buf.free()
    for res, (clips, masks) in zip(got, (a, b)):
        assert_equal_alone(res, clips, masks, wl, True, "FT", 0)


# ------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("layout, row_align", LAYOUTS)
def test_mask_layout_is_that_of_a_ragged_magnitude_stft(layout, row_align):
    import zafx
    for wl in WINDOWS:
        w, h = zafx.hamming(wl), wl // 2
        lengths = np.array(lengths_of(h), np.int64)
        plan = plan_of(wl, False, layout, row_align)
        spec = zafx.stft_plan(w, h, layout=layout, onesided="magnitude", row_align=row_align)
        offs, frames, pitch = spec.ragged_layout(lengths)
        assert plan.mask_ragged_layout(lengths).tolist() == offs.tolist(), (wl, layout, row_align)
        assert [plan.mask_dims(n) for n in lengths.tolist()] == [(h + 1, t) for t in frames.tolist()]
        assert [plan.row_pitch(n) for n in lengths.tolist()] == pitch.tolist()


def test_ones_masks_in_the_buffer_of_a_ragged_stft_give_back_the_clips():
    """A ragged |X| STFT writes its spectra into a buffer; ones put where its |X| lie (NaN in the pad columns) are the masks of the ragged mask
    filter at the same offsets: the filter returns the clips (Hamming at H = W/2 is COLA)."""
    import zafx
    wl, layout, row_align = 2048, "FT", 32
    w, h = zafx.hamming(wl), wl // 2
    lengths = [n for n in lengths_of(h)]
    clips = [clip(90 + i, n) for i, n in enumerate(lengths)]
    spec = zafx.stft_plan(w, h, layout=layout, onesided="magnitude", row_align=row_align)
    x, in_offs, lens = zafx.pack_ragged(clips)
    offs, frames, pitch = spec.ragged_layout(lens)
    plan = plan_of(wl, False, layout, row_align)
    d_in, d_spec = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer((int(offs[-1]),), np.float32)
    d_out = zafx.DeviceBuffer.from_host(np.full(len(x), FILL, np.uint32))
    try:
        spec.execute_ragged(d_in, in_offs, lens, d_spec)
        spec.sync()
        mag = d_spec.download()
        for o, t, p in zip(offs[:-1].tolist(), frames.tolist(), pitch.tolist()):
            block = mag[o:o + (h + 1) * p].reshape(h + 1, p)
            assert np.isfinite(block[:, :t]).all()
            block[:, :t] = 1.0
            block[:, t:] = np.nan
        d_spec.upload(mag)
        plan.execute_masked_ragged(d_in, in_offs, lens, d_spec, offs, View(d_out, 0, len(x)), in_offs)
        plan.sync()
        got = d_out.download()
    finally:
        for b in (d_in, d_spec, d_out):
            b.free()
    for c, o in zip(clips, in_offs.tolist()):
        y = got[o:o + len(c)].view(np.float32)
        err = mask_error(y, c, c)
        print(f"identity N={len(c)}: {err:.3e} of the level")
        assert np.isfinite(y).all() and err <= TOL_FFT, (len(c), err)


# ------------------------------------------------------------------------------------------------------------------ 8
def test_refusals_leave_the_output_untouched():
    import zafx
    from zafx import _lib
    wl, h = 512, 256
    w = zafx.hamming(wl)
    lengths = np.array([3000, 0, 700], np.int64)
    clips, masks = batch_of(wl, lengths.tolist(), seed=40)
    plan = plan_of(wl, True)
    x = np.concatenate(clips)
    in_offs = np.array([0, 3000, 3000], np.int64)
    mask_offs = plan.mask_ragged_layout(lengths)
    out_offs = 2 * in_offs
    sentinel = np.full(2 * len(x), -12345.5, np.float32)
    d_in, d_out = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(sentinel)
    d_mask = zafx.DeviceBuffer.from_host(np.concatenate([laid(plan, m, len(c)) for c, m in zip(clips, masks)]))
    lib = _lib.load()
    p64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731

    def call(pl, a_in=d_in.ptr, a_inoff=in_offs, a_len=lengths, a_mask=d_mask.ptr, a_moff=mask_offs, a_out=d_out.ptr, a_ooff=out_offs, n=3):
        rc = lib.zafx_execute_masked_ragged(pl, a_in, None if a_inoff is None else p64(a_inoff), None if a_len is None else p64(a_len), a_mask,
                                            None if a_moff is None else p64(a_moff), a_out, None if a_ooff is None else p64(a_ooff), n)
        return rc, (lib.zafx_last_error() or b"").decode()

    def neg(a, i):
        b = a.copy()
        b[i] = -1
        return b

    big = lengths.copy()
    big[2] = 1 << 28
    cases = [
        (dict(pl=None), "null plan"),
        (dict(a_in=None), "null device pointer"), (dict(a_mask=None), "null device pointer"), (dict(a_out=None), "null device pointer"),
        (dict(a_inoff=None), "null argument"), (dict(a_len=None), "null argument"), (dict(a_moff=None), "null argument"), (dict(a_ooff=None), "null argument"),
        (dict(n=-1), "negative number of clips"),
        (dict(a_len=neg(lengths, 1)), "of clip 1"), (dict(a_inoff=neg(in_offs, 2)), "of clip 2"), (dict(a_moff=neg(mask_offs, 0)), "of clip 0"),
        (dict(a_ooff=neg(out_offs, 2)), "of clip 2"),
        (dict(a_len=big), "clip 2 has 2^28 samples"),
    ]
    for kw, text in cases:
        kw.setdefault("pl", plan.handle)
        rc, msg = call(**kw)
        assert rc != 0 and text in msg, (kw.keys(), rc, msg)
        if "of clip" in text:
            assert "negative" in msg
    # another kind
    stft = zafx.stft_plan(w, h)
    rc, msg = call(stft.handle)
    assert rc != 0 and "ZAFX_MASKFILTER" in msg, msg
    offs = (ctypes.c_int64 * 4)()
    assert lib.zafx_plan_mask_ragged_layout(stft.handle, p64(lengths), 3, offs) != 0 and b"ZAFX_MASKFILTER" in lib.zafx_last_error()
    assert lib.zafx_plan_mask_ragged_layout(plan.handle, p64(neg(lengths, 1)), 3, offs) != 0 and b"clip 1" in lib.zafx_last_error()
    # a window that is not set, and one whose COLA sum is zero
    bare = zafx.Plan(zafx.MASKFILTER_REST, window_length=wl, step_length=h)
    rc, msg = call(bare.handle)
    assert rc != 0 and "window constant not set" in msg, msg
    wz = np.array(w, np.float64)
    wz[h] = -wz[0]
    bare.set_window(wz)
    rc, msg = call(bare.handle)
    assert rc != 0 and "is zero" in msg, msg
    bare.destroy()
    # zafx_execute_ragged and zafx_plan_ragged_layout on a mask-filter plan: today's message
    rc = lib.zafx_execute_ragged(plan.handle, d_in.ptr, p64(in_offs), p64(lengths), d_out.ptr, 3)
    msg = lib.zafx_last_error().decode()
    assert rc != 0 and msg == "zafx_execute_ragged: mask filter plans (ZAFX_MASKFILTER / ZAFX_MASKFILTER_REST) take a mask: call zafx_execute_masked", msg
    with pytest.raises(zafx.ZafxError, match="call zafx_execute_masked"):
        plan.ragged_layout(lengths)
    # through the Python layer: buffers too small
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_ragged(d_in, in_offs, lengths, View(d_mask, 0, int(mask_offs[-1]) - 5), mask_offs, d_out, out_offs)
    with pytest.raises(ValueError, match="d_out"):
        plan.execute_masked_ragged(d_in, in_offs, lengths, d_mask, mask_offs, View(d_out, 0, len(sentinel) - 1), out_offs)
    with pytest.raises(ValueError, match="one entry per clip"):
        plan.execute_masked_ragged(d_in, in_offs[:2], lengths, d_mask, mask_offs, d_out, out_offs)
    plan.sync(), stft.sync()
    assert np.array_equal(bits(d_out.download()), bits(sentinel))
    # ... and the same arguments unharmed are accepted
    rc, msg = call(plan.handle)
    assert rc == 0, msg
    plan.sync()
    assert plan.last_kernel == "k_maskfilter_ragged"
    for buf in (d_in, d_mask, d_out):
        buf.free()


# ------------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("layout", ["FT", "TF"])
def test_python_api(layout):
    import zafx
    wl = 1024
    w, h = zafx.hamming(wl), wl // 2
    lengths = [4 * h + 7, 1, 0, 33 * h, h]
    clips, masks = batch_of(wl, lengths, seed=60)
    given = masks if layout == "FT" else [m.T for m in masks]
    ys = zafx.maskfilter_ragged([c.astype(np.float64) for c in clips], w, given, layout=layout)
    pairs = zafx.maskfilter_ragged(clips, w, given, step_length=h, rest=True, layout=layout)
    assert len(ys) == len(pairs) == len(clips)
    for y, (yr, rr), c, m in zip(ys, pairs, clips, given):
        assert y.dtype == yr.dtype == rr.dtype == np.float32 and y.shape == yr.shape == rr.shape == c.shape
        assert yr.base is not None and yr.base is rr.base
        if not len(c):
            continue
        ref = zafx.maskfilter_batch(c[None], w, m[None], layout=layout)
        ref_y, ref_r = zafx.maskfilter_batch(c[None], w, m[None], rest=True, layout=layout)
        assert np.array_equal(bits(y), bits(ref[0])) and np.array_equal(bits(yr), bits(ref_y[0])) and np.array_equal(bits(rr), bits(ref_r[0]))
    with pytest.raises(ValueError, match="mask 3 must have shape .* for clip 3"):
        zafx.maskfilter_ragged(clips, w, given[:3] + [given[0]] + given[4:], layout=layout)
