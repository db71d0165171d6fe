"""Ragged mask filter stems on the GPU (k_maskfilter_stems' RAGGED form; zafx_execute_masked_stems_ragged, zafx_plan_stems_ragged_layout): clips
of different lengths with S masks each in one launch.  Every clip's block is held BIT FOR BIT to Plan.execute_masked_stems on that clip and
its S masks alone (B = 1, a "TF" plan) -- at the pair and tile edges of every window, for S = 1, 2, 3 and 8, with and without the rest, cut
into units, dealt over fewer workgroups than units, on one compute unit, permuted, with the masks in another order, inside NaN-filled arenas
off the 8-byte and the 128-byte grid --, the rest to the float32 subtraction chain of the downloaded stems, and at W = 256 and 2048 every stem
to the float64 oracle; then several calls and kinds on one plan, the refusals and the host functions.

Bounds: bit identity; against the oracle max|y - ref| <= 1e-5 max(max|ref|, max|x|) per stem (TOL_FFT at mask_error's level, the bound of
tests/test_gpu_maskfilter_stems.py).  H = W/2 is a block; F (maskfilter_tile_transforms) packed transforms make a tile; the cutter cuts a clip
of more than 4 F - 3 block pairs."""
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
KERNEL = "k_maskfilter_stems_ragged"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def clip(seed, n):
    return np.random.default_rng([405, seed, n]).standard_normal(n).astype(np.float32)


def edge_lengths(wl):
    """The pair and tile edges, a clip of length 0 among them."""
    import zafx
    h, f = wl // 2, zafx.maskfilter_tile_transforms(wl)
    return [1, h, 0, 2 * h + 1, 2 * f * h - 1, 2 * f * h, 2 * f * h + 1, 4 * f * h + 3]


def tf(m):
    """Masks (..., W/2 + 1, T) -> (..., T, W/2 + 1), contiguous float32."""
    return np.ascontiguousarray(np.swapaxes(m, -1, -2), np.float32)


def batch_of(wl, lengths, n_stems=8, seed=0):
    """-> (clips, masks): clip i (N_i,), its masks (n_stems, T_i, W/2 + 1) "unit" with a seed per (clip, stem)."""
    clips = [clip(seed + i, n) for i, n in enumerate(lengths)]
    masks = [tf(np.stack([make_mask("unit", wl, n, seed=10 * (seed + i) + s) for s in range(n_stems)])) for i, n in enumerate(lengths)]
    return clips, masks


def chain(x, y):
    """((x - y_0) - y_1) - ... in float32, left to right; x (N,), y (S, N)."""
    r = np.asarray(x, np.float32).copy()
    for s in range(len(y)):
        r = r - y[s]
    assert r.dtype == np.float32
    return r


class View:
    """`count` float32 at word `first` of a DeviceBuffer of 32-bit words (nothing to free)."""

    def __init__(self, buf, first, count):
        self.ptr, self.dtype, self.nbytes, self.shape = ctypes.c_void_p(buf.ptr.value + 4 * first), np.dtype(np.float32), 4 * count, (count,)


def place(sizes, gap, base, order=None):
    """-> (offsets, words): blocks of `sizes` words laid in `order` (default: as given), `gap` words between them, the first at word `base`."""
    offs, at = [0] * len(sizes), base
    for i in (range(len(sizes)) if order is None else order):
        offs[i] = at
        at += sizes[i] + gap
    return np.array(offs, np.int64), at + 1


def plan_of(wl, rest):
    import zafx
    return zafx.maskfilter_plan(zafx.hamming(wl), rest=rest, layout="TF")


def fresh_plan(wl, rest):
    """A plan nothing has run on (maskfilter_plan's are cached); the caller destroys it."""
    import zafx
    p = zafx.Plan(zafx.MASKFILTER_REST if rest else zafx.MASKFILTER, window_length=wl, step_length=wl // 2, layout="TF")
    p.set_window(zafx.hamming(wl))
    return p


_ALONE = {}


def alone(wl, rest, x, m, key=None):
    """Plan.execute_masked_stems with B = 1 on one clip and its S masks alone: (S [+ 1], N).  `key`: the clip's name in this module's cache."""
    import zafx
    key = key and (wl, rest, m.shape[0]) + tuple(key)
    if key in _ALONE:
        return _ALONE[key]
    n, s = len(x), m.shape[0]
    plan = plan_of(wl, rest)
    d_in, d_mask = zafx.DeviceBuffer.from_host(x[None]), zafx.DeviceBuffer.from_host(m[None])
    d_out = zafx.DeviceBuffer(plan.stems_out_shape(1, n, s), np.float32)
    try:
        plan.execute_masked_stems(d_in, d_mask, d_out, 1, n, s)
        plan.sync()
        assert plan.last_kernel == "k_maskfilter_stems"
        res = d_out.download()[0]
    finally:
        for b in (d_in, d_mask, d_out):
            b.free()
    if key:
        _ALONE[key] = res
    return res


def run_ragged(plan, clips, masks, gap=0, bases=(0, 0, 0), sync=True, mask_order=None):
    """One zafx_execute_masked_stems_ragged over the clips, every array inside an arena of FILL words: `gap` words between the clips, between the
    clips' masks and between the output blocks, the three arrays at words `bases`; the masks laid in `mask_order`.  masks[i]: (S, T_i, W/2 + 1).
    -> (the output arena's words, out_offsets, lengths, the buffers)."""
    import zafx
    n_stems = masks[0].shape[0]
    blocks = n_stems + (1 if plan.kind == zafx.MASKFILTER_REST else 0)
    lengths = np.array([len(c) for c in clips], np.int64)
    in_offs, in_words = place(lengths.tolist(), gap, bases[0])
    mask_offs, mask_words = place([m.size for m in masks], gap, bases[1], mask_order)
    out_offs, out_words = place((blocks * lengths).tolist(), gap, bases[2])
    h_in, h_mask = np.full(in_words, FILL, np.uint32), np.full(mask_words, FILL, np.uint32)
    for c, o in zip(clips, in_offs.tolist()):
        h_in[o:o + len(c)] = bits(c)
    for m, o in zip(masks, mask_offs.tolist()):
        h_mask[o:o + m.size] = bits(m).ravel()
    bufs = [zafx.DeviceBuffer.from_host(h_in), zafx.DeviceBuffer.from_host(h_mask), zafx.DeviceBuffer.from_host(np.full(out_words, FILL, np.uint32))]
    views = [View(b, 0, b.shape[0]) for b in bufs]
    plan.execute_masked_stems_ragged(views[0], in_offs, lengths, views[1], mask_offs, views[2], out_offs, n_stems)
    if not sync:
        return None, out_offs, lengths, bufs
    try:
        plan.sync()
        assert plan.last_kernel == KERNEL and plan.kernel_name == "k_maskfilter"
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
    assert (words[kept] == FILL).all(), "written outside the clips' blocks"
    return res


def assert_equal_alone(res, clips, masks, wl, rest, keys=None, what=""):
    n_stems = masks[0].shape[0]
    for i, (r, x, m) in enumerate(zip(res, clips, masks)):
        assert r.shape == (n_stems + int(rest), len(x))
        if not len(x):
            continue
        ref = alone(wl, rest, x, m, keys and keys[i])
        assert np.array_equal(bits(r), bits(ref)), (what, wl, rest, n_stems, i, len(x))
        if rest:
            assert np.array_equal(bits(r[n_stems]), bits(chain(x, r[:n_stems]))), (what, wl, n_stems, i, "rest")


@pytest.fixture(scope="module")
def edges():
    """Per W: (clips, masks with 8 stems) at the edge lengths; S stems are a clip's first S masks."""
    return {wl: batch_of(wl, edge_lengths(wl)) for wl in WINDOWS}


_ORACLE = {}


def oracle(wl, i, s, x, m):
    """The float64 reference of clip i, stem s of the edge batch (m: (T, W/2 + 1)), computed once."""
    import zafx
    if (wl, i, s) not in _ORACLE:
        _ORACLE[wl, i, s] = oracle_maskfilter(x, zafx.hamming(wl), m.T)
    return _ORACLE[wl, i, s]


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("wl", WINDOWS)
def test_pair_and_tile_edges_bit_for_bit(edges, wl, rest):
    clips, masks8 = edges[wl]
    for s in STEMS:
        masks = [np.ascontiguousarray(m[:s]) for m in masks8]
        words, out_offs, lens, _ = run_ragged(plan_of(wl, rest), clips, masks)
        res = results(words, out_offs, lens, s + int(rest))
        assert_equal_alone(res, clips, masks, wl, rest, keys=[(0, i) for i in range(len(clips))])
        if s == 3 and wl in (256, 2048):
            worst = 0.0
            for i, (r, x, m) in enumerate(zip(res, clips, masks)):
                for j in range(s):
                    err = mask_error(r[j], oracle(wl, i, j, x, m[j]), x)
                    worst = max(worst, err)
                    assert err <= TOL_FFT, (wl, rest, i, j, err)
            print(f"W={wl} rest={rest}: worst error against the oracle {worst:.3e} of the level")


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("rest", [False, True])
def test_cut_clips(rest):
    """60, almost 61 and almost 200 blocks at W = 2048: the cutter cuts all three."""
    from maskfilter_stems_ragged_probe import probe_batch
    wl, clips, masks = probe_batch("cut", 3)
    words, out_offs, lens, _ = run_ragged(plan_of(wl, rest), clips, masks)
    assert_equal_alone(results(words, out_offs, lens, 3 + int(rest)), clips, masks, wl, rest, what="cut")


# ------------------------------------------------------------------------------------------------------------------ 3
def test_more_units_than_workgroups():
    """600 clips of 1 - 6 blocks at W = 256, two stems: the rounds of the deal run forwards and backwards.  Against the same clips through the
    equal-length execute_masked_stems, one launch per length."""
    import zafx
    from maskfilter_stems_ragged_probe import probe_batch
    wl, clips, masks = probe_batch("short", 2)
    plan = plan_of(wl, True)
    words, out_offs, lens, _ = run_ragged(plan, clips, masks)
    res = results(words, out_offs, lens, 3)
    groups = {}
    for i, c in enumerate(clips):
        groups.setdefault(len(c), []).append(i)
    for n, idx in groups.items():
        x, m = np.stack([clips[i] for i in idx]), np.stack([masks[i] for i in idx])
        d_in, d_mask = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(m)
        d_out = zafx.DeviceBuffer(plan.stems_out_shape(len(idx), n, 2), np.float32)
        try:
            plan.execute_masked_stems(d_in, d_mask, d_out, len(idx), n, 2)
            plan.sync()
            assert plan.last_kernel == "k_maskfilter_stems"
            ref = d_out.download()
        finally:
            for b in (d_in, d_mask, d_out):
                b.free()
        for k, i in enumerate(idx):
            assert np.array_equal(bits(res[i]), bits(ref[k])), (n, i)


def test_more_units_than_workgroups_at_one_workgroup_per_compute_unit():
    """600 clips of 1 - 6 blocks at W = 2048, where one workgroup fits a compute unit, two stems: every workgroup walks several rounds of the deal."""
    wl = 2048
    g = np.random.default_rng(601)
    lengths = (g.integers(0, 6, 600) * 1024 + g.integers(1, 1025, 600)).tolist()
    clips, masks = batch_of(wl, lengths, n_stems=2, seed=1000)
    plan = plan_of(wl, False)
    assert plan.compute_units < 600
    words, out_offs, lens, _ = run_ragged(plan, clips, masks)
    assert_equal_alone(results(words, out_offs, lens, 2), clips, masks, wl, False)


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.timeout(300)
def test_one_compute_unit_gives_the_same_bits(tmp_path):
    """The cut clips and the 600 short ones in a fresh child process with ZAFX_COMPUTE_UNITS=1: other slots, other cuts, every unit on a few workgroups."""
    from maskfilter_stems_ragged_probe import BATCHES, run_batch
    path = str(tmp_path / "probe.npz")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "maskfilter_stems_ragged_probe.py"), path, "1"],
                         env=dict(os.environ, ZAFX_COMPUTE_UNITS="1"), capture_output=True, timeout=240)
    assert res.returncode == 0 and b"probe ok" in res.stdout, res.stderr.decode()[-2000:]
    got = np.load(path)
    for which, n_stems in BATCHES:
        here, cus = run_batch(which, n_stems)
        assert int(got[f"units_{which}"]) == 1 and cus > 1
        assert np.array_equal(bits(got[which]), bits(here)), which


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("rest", [False, True])
def test_writes_nothing_but_the_clips_blocks(edges, rest):
    """Clips, masks and output blocks with gaps between them, inside arenas of NaN words whose bases are 4 bytes off the 8-byte and the 128-byte
    grid.  Every output word outside the blocks keeps the fill; the results are finite and those of the compact run."""
    for wl in (2048, 256):
        clips, masks = edges[wl][0], [np.ascontiguousarray(m[:3]) for m in edges[wl][1]]
        plan = plan_of(wl, rest)
        blocks = 3 + int(rest)
        compact = results(*run_ragged(plan, clips, masks)[:3], blocks)
        words, out_offs, lens, _ = run_ragged(plan, clips, masks, gap=37, bases=(35, 32 * 3 + 1, 33))
        spread = results(words, out_offs, lens, blocks)
        for a, b in zip(spread, compact):
            assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b)), (wl, rest)


# ------------------------------------------------------------------------------------------------------------------ 6
def test_place_in_the_batch(edges):
    wl = 512
    clips, masks = edges[wl][0], [np.ascontiguousarray(m[:3]) for m in edges[wl][1]]
    plan = plan_of(wl, True)
    straight = results(*run_ragged(plan, clips, masks)[:3], 4)
    perm = np.random.default_rng(8).permutation(len(clips)).tolist()
    permuted = results(*run_ragged(plan, [clips[i] for i in perm], [masks[i] for i in perm])[:3], 4)
    for k, i in enumerate(perm):
        assert np.array_equal(bits(permuted[k]), bits(straight[i])), ("permuted", k, i)
    # the masks in reverse order, mask_offsets to match
    turned = results(*run_ragged(plan, clips, masks, mask_order=list(range(len(clips)))[::-1])[:3], 4)
    for i, (a, b) in enumerate(zip(turned, straight)):
        assert np.array_equal(bits(a), bits(b)), ("masks reversed", i)
    # a NaN sample in one clip stays there: the clips lie back to back
    k = 4
    sick = [c.copy() for c in clips]
    sick[k][len(sick[k]) // 2] = np.nan
    got = results(*run_ragged(plan, sick, masks)[:3], 4)
    assert np.isnan(got[k]).any()
    for i, (a, b) in enumerate(zip(got, straight)):
        if i != k:
            assert np.array_equal(bits(a), bits(b)), ("beside a NaN", i)


# ------------------------------------------------------------------------------------------------------------------ 7
def test_back_to_back_calls_each_see_their_own_table():
    wl = 1024
    h = wl // 2
    a = batch_of(wl, [5 * h + 3, 1, 40 * h, 2 * h], n_stems=2, seed=20)
    b = batch_of(wl, [70 * h - 1, 0, 3 * h, h + 1, 9 * h, 2], n_stems=3, seed=30)
    plan = plan_of(wl, True)
    first = run_ragged(plan, *a, sync=False)
    second = run_ragged(plan, *b, sync=False)
    try:
        plan.sync()
        assert plan.last_kernel == KERNEL
        got = [results(r[3][2].download(), r[1], r[2], s + 1) for r, s in ((first, 2), (second, 3))]
    finally:
        for r in (first, second):
            for buf in r[3]:
                buf.free()
    for res, (clips, masks) in zip(got, (a, b)):
        assert_equal_alone(res, clips, masks, wl, True)


def test_other_kinds_on_the_same_plan_are_not_affected():
    """After a ragged stems call the equal-length stems, the ragged one-mask kind and the one-mask kind on the same plan give a fresh plan's bits."""
    import zafx
    wl = 512
    h = wl // 2
    lengths = [9 * h + 5, 0, h, 37 * h - 1]
    clips, masks = batch_of(wl, lengths, n_stems=3, seed=70)

    def others(plan):
        out = []
        n = lengths[0]
        d_in, d_mask = zafx.DeviceBuffer.from_host(clips[0][None]), zafx.DeviceBuffer.from_host(masks[0][None])
        d_out = zafx.DeviceBuffer(plan.stems_out_shape(1, n, 3), np.float32)
        d_one = zafx.DeviceBuffer(plan.out_shape(1, n), np.float32)
        lens = np.array(lengths, np.int64)
        in_offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        mask_offs = plan.mask_ragged_layout(lens)
        d_x = zafx.DeviceBuffer.from_host(np.concatenate(clips))
        d_m = zafx.DeviceBuffer.from_host(np.concatenate([m[0].ravel() for m in masks]))
        d_r = zafx.DeviceBuffer((2 * int(lens.sum()),), np.float32)
        try:
            plan.execute_masked_stems(d_in, d_mask, d_out, 1, n, 3)
            plan.sync()
            assert plan.last_kernel == "k_maskfilter_stems"
            out.append(d_out.download())
            plan.execute_masked_ragged(d_x, in_offs, lens, d_m, mask_offs, d_r, 2 * in_offs)
            plan.sync()
            assert plan.last_kernel == "k_maskfilter_ragged"
            out.append(d_r.download())
            plan.execute_masked(d_in, View(d_mask, 0, masks[0][0].size), d_one, 1, n)
            plan.sync()
            assert plan.last_kernel == "k_maskfilter"
            out.append(d_one.download())
        finally:
            for b in (d_in, d_mask, d_out, d_one, d_x, d_m, d_r):
                b.free()
        return out

    used, fresh = fresh_plan(wl, True), fresh_plan(wl, True)
    try:
        words, out_offs, lens, _ = run_ragged(used, clips, masks)
        assert_equal_alone(results(words, out_offs, lens, 4), clips, masks, wl, True)
        for a, b in zip(others(used), others(fresh)):
            assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b))
    finally:
        used.destroy(), fresh.destroy()


# ------------------------------------------------------------------------------------------------------------------ 8
def test_refusals_leave_the_output_untouched():
    import zafx
    from zafx import _lib
    wl, h = 512, 256
    w = zafx.hamming(wl)
    lengths = np.array([3000, 0, 700], np.int64)
    clips, masks = batch_of(wl, lengths.tolist(), n_stems=2, seed=40)
    plan = plan_of(wl, True)
    x = np.concatenate(clips)
    in_offs = np.array([0, 3000, 3000], np.int64)
    mask_offs, out_offs = plan.stems_ragged_layout(lengths, 2)
    assert out_offs.tolist() == [0, 9000, 9000, 11100]
    sentinel = np.full(int(out_offs[-1]), -12345.5, np.float32)
    d_in, d_out = zafx.DeviceBuffer.from_host(x), zafx.DeviceBuffer.from_host(sentinel)
    d_mask = zafx.DeviceBuffer.from_host(np.concatenate([m.ravel() for m in masks]))
    assert d_mask.shape[0] == mask_offs[-1]
    lib = _lib.load()
    p64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))   # noqa: E731

    def call(pl, a_in=d_in.ptr, a_inoff=in_offs, a_len=lengths, a_mask=d_mask.ptr, a_moff=mask_offs, a_out=d_out.ptr, a_ooff=out_offs, n=3, stems=2):
        rc = lib.zafx_execute_masked_stems_ragged(pl, a_in, None if a_inoff is None else p64(a_inoff), None if a_len is None else p64(a_len), a_mask,
                                                  None if a_moff is None else p64(a_moff), a_out, None if a_ooff is None else p64(a_ooff), n, stems)
        return rc, (lib.zafx_last_error() or b"").decode()

    def neg(a, i):
        b = a.copy()
        b[i] = -1
        return b

    big = lengths.copy()
    big[2] = 1 << 28   # in `lengths` only: refused before anything is read
    cases = [
        (dict(pl=None), "null plan"),
        (dict(a_in=None), "null device pointer"), (dict(a_mask=None), "null device pointer"), (dict(a_out=None), "null device pointer"),
        (dict(a_inoff=None), "null argument"), (dict(a_len=None), "null argument"), (dict(a_moff=None), "null argument"), (dict(a_ooff=None), "null argument"),
        (dict(n=-1), "negative number of clips"),
        (dict(a_len=neg(lengths, 1)), "of clip 1"), (dict(a_inoff=neg(in_offs, 2)), "of clip 2"), (dict(a_moff=neg(mask_offs, 0)), "of clip 0"),
        (dict(a_ooff=neg(out_offs, 2)), "of clip 2"),
        (dict(a_len=big), "2^28"),
        (dict(stems=0), "n_stems"), (dict(stems=9), "n_stems"), (dict(stems=0, n=0), "n_stems"),
    ]
    for kw, text in cases:
        kw.setdefault("pl", plan.handle)
        rc, msg = call(**kw)
        assert rc != 0 and text in msg, (kw.keys(), rc, msg)
        if "of clip" in text:
            assert "negative" in msg
        if text == "2^28":
            assert "clip 2" in msg
        if text == "n_stems":
            assert "1 .. 8" in msg
    # an FT plan: the message names the layout to use
    ft = zafx.maskfilter_plan(w, rest=True, layout="FT")
    rc, msg = call(ft.handle)
    assert rc != 0 and "ZAFX_LAYOUT_TF" in msg, msg
    offs = (ctypes.c_int64 * 4)()
    offs2 = (ctypes.c_int64 * 4)()
    assert lib.zafx_plan_stems_ragged_layout(ft.handle, p64(lengths), 3, 2, offs, offs2) != 0 and b"ZAFX_LAYOUT_TF" in lib.zafx_last_error()
    # another kind
    stft = zafx.stft_plan(w, h)
    rc, msg = call(stft.handle)
    assert rc != 0 and "ZAFX_MASKFILTER" in msg, msg
    assert lib.zafx_plan_stems_ragged_layout(stft.handle, p64(lengths), 3, 2, offs, offs2) != 0 and b"ZAFX_MASKFILTER" in lib.zafx_last_error()
    assert lib.zafx_plan_stems_ragged_layout(plan.handle, p64(neg(lengths, 1)), 3, 2, offs, offs2) != 0 and b"clip 1" in lib.zafx_last_error()
    assert lib.zafx_plan_stems_ragged_layout(plan.handle, p64(lengths), 3, 9, offs, offs2) != 0 and b"n_stems" in lib.zafx_last_error()
    # through the Python layer: buffers too small, arrays of the wrong length, masks of the wrong shape, S differing between clips
    with pytest.raises(ValueError, match="d_mask"):
        plan.execute_masked_stems_ragged(d_in, in_offs, lengths, View(d_mask, 0, int(mask_offs[-1]) - 5), mask_offs, d_out, out_offs, 2)
    with pytest.raises(ValueError, match="d_out"):
        plan.execute_masked_stems_ragged(d_in, in_offs, lengths, d_mask, mask_offs, View(d_out, 0, len(sentinel) - 1), out_offs, 2)
    with pytest.raises(ValueError, match="one entry per clip"):
        plan.execute_masked_stems_ragged(d_in, in_offs[:2], lengths, d_mask, mask_offs, d_out, out_offs, 2)
    with pytest.raises(ValueError, match="mask 2 must have shape .* for clip 2"):
        zafx.maskfilter_stems_ragged(clips, w, [masks[0], masks[1], masks[2][:, 1:]], layout="TF")
    with pytest.raises(ValueError, match="mask 2 has 1 stems"):
        zafx.maskfilter_stems_ragged(clips, w, [masks[0], masks[1], masks[2][:1]], layout="TF")
    plan.sync(), stft.sync(), ft.sync()
    assert np.array_equal(bits(d_out.download()), bits(sentinel))
    # ... the same arguments unharmed are accepted, and an empty batch is fine
    rc, msg = call(plan.handle, n=0)
    assert rc == 0, msg
    rc, msg = call(plan.handle)
    assert rc == 0, msg
    plan.sync()
    assert plan.last_kernel == KERNEL
    got = d_out.download()
    for i, (x_i, m_i) in enumerate(zip(clips, masks)):
        if len(x_i):
            assert np.array_equal(bits(got[out_offs[i]:out_offs[i + 1]]), bits(alone(wl, True, x_i, m_i).ravel())), i
    for buf in (d_in, d_mask, d_out):
        buf.free()


# ------------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("layout", ["FT", "TF"])
def test_host_functions(layout, rest):
    import zafx
    wl = 1024
    w, h = zafx.hamming(wl), wl // 2
    lengths = [4 * h + 7, 1, 0, 33 * h, h]
    clips = [clip(60 + i, n) for i, n in enumerate(lengths)]
    masks = [np.stack([make_mask("unit", wl, n, seed=600 + 10 * i + s) for s in range(3)]) for i, n in enumerate(lengths)]   # (S, W/2 + 1, T)
    given = masks if layout == "FT" else [tf(m) for m in masks]
    out = zafx.maskfilter_stems_ragged([c.astype(np.float64) for c in clips], w, given, step_length=h, rest=rest, layout=layout)
    assert len(out) == len(clips)
    for o, c, m in zip(out, clips, given):
        stems, rr = o if rest else (o, None)
        assert stems.dtype == np.float32 and stems.shape == (3, len(c)) and stems.base is not None
        if rest:
            assert rr.dtype == np.float32 and rr.shape == c.shape
        if not len(c):
            continue
        ref = zafx.maskfilter_stems_batch(c[None], w, m[None], rest=rest, layout=layout)
        ref_stems, ref_rest = (ref[0][0], ref[1][0]) if rest else (ref[0], None)
        assert np.array_equal(bits(stems), bits(ref_stems))
        if rest:
            assert np.array_equal(bits(rr), bits(ref_rest)) and np.array_equal(bits(rr), bits(chain(c, stems)))


def test_layout_is_stems_times_the_one_mask_layout():
    for wl in WINDOWS:
        lengths = np.array(edge_lengths(wl), np.int64)
        for rest in (False, True):
            plan = plan_of(wl, rest)
            one = plan.mask_ragged_layout(lengths)
            for s in STEMS:
                mask_offs, out_offs = plan.stems_ragged_layout(lengths, s)
                assert mask_offs.tolist() == (s * one).tolist(), (wl, s)
                assert out_offs.tolist() == np.concatenate([[0], np.cumsum((s + int(rest)) * lengths)]).tolist(), (wl, s, rest)
    assert one[3] - one[2] == wl // 2 + 1   # a clip of length 0: one frame


# ------------------------------------------------------------------------------------------------------------------ 10
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
    """Three stems and the rest over a ragged batch.  A NaN sample in one clip and a NaN in the mask of its stem 0: every other clip has the bits
    of its run alone and of the clean batch; inside that clip only the samples of the frames that hold the NaN sample or mask value, and of
    the frames paired with them, may be non-finite, in any stem or the rest.  Then a NaN, and +inf, in the mask of stem 1 alone -- the stems
    share one forward transform --: stems 0 and 2 keep the clean bits everywhere, stem 1 and the rest are non-finite only in the samples of
    that frame and of its partner."""
    h = wl // 2
    n = 20 * h + 9
    clips, masks = batch_of(wl, [7 * h + 3, 0, n, 1, n], n_stems=3, seed=80)
    plan = plan_of(wl, True)
    at, s, (k, t) = 2, 5 * h + 17, (h // 3, 13)   # sample s lies in frames 5 and 6; the mask value in frame 13
    others = [i for i in range(len(clips)) if i != at]
    clean = results(*run_ragged(plan, clips, masks)[:3], 4)

    def rerun(sample, stem, value):
        bad_clips, bad_masks = [c.copy() for c in clips], [m.copy() for m in masks]
        if sample:
            bad_clips[at][s] = np.nan
        bad_masks[at][stem, t, k] = value
        got = results(*run_ragged(plan, bad_clips, bad_masks)[:3], 4)
        for i in others:
            assert np.array_equal(bits(got[i]), bits(clean[i])), (wl, stem, i)
        return got

    got = rerun(True, 0, np.nan)
    assert_equal_alone([got[i] for i in others], [clips[i] for i in others], [masks[i] for i in others], wl, True, what="containment")
    may = touched(n, h, [s // h, s // h + 1, t])
    assert 0 < may.sum() < n
    for j in range(4):
        assert not np.isfinite(got[at][j][may]).all() and np.isfinite(got[at][j][~may]).all(), (wl, j)
        assert np.array_equal(bits(got[at][j][~may]), bits(clean[at][j][~may])), (wl, j)
    may = touched(n, h, [t])
    for value in (np.nan, np.inf):
        got = rerun(False, 1, value)
        for j in (0, 2):
            assert np.array_equal(bits(got[at][j]), bits(clean[at][j])), (wl, value, "stem", j)
        for j in (1, 3):
            assert not np.isfinite(got[at][j][may]).all() and np.isfinite(got[at][j][~may]).all(), (wl, value, j)
            assert np.array_equal(bits(got[at][j][~may]), bits(clean[at][j][~may])), (wl, value, j)
