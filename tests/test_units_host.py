"""The exact tables of the ragged launches (no GPU): the cutter's rule and the deal (zafx_units.hpp), restated here in a few lines of Python, held
record for record against what the two host programs print -- center_units_emu for k_center's units, tile_units_emu for k_imdct's and
k_istft_ft16's units and their tables in launch order.  test_center_ragged_host.py, test_imdct_ragged_host.py and test_istft_ragged_host.py hold
the invariants of a cut; this pins the cut itself, so a change to the shared cutter cannot re-balance one kernel's launch unnoticed."""
import numpy as np

from test_center_ragged_host import cutter as center_cutter, length_lists   # noqa: F401  (center_cutter: a fixture)
from test_imdct_ragged_host import PER_SLOT, TILE, cutter as imdct_cutter, random_batches   # noqa: F401  (imdct_cutter: a fixture)
from test_istft_ragged_host import PER_SLOT as ISTFT_PER_SLOT, TILE as ISTFT_TILE, cutter as istft_cutter, random_batches as istft_random_batches   # noqa: F401  (istft_cutter: a fixture)

CENTER_PER_SLOT = 12   # kCenterUnitsPerSlot


def cut(counts, floor, slots, per_slot):
    """-> (S, [(clip, a, b)]): the rule of zafx_units.hpp for clips of counts[i] pieces."""
    seg = max(floor, -(-sum(counts) // (max(1, slots) * per_slot)))
    segs = []
    for clip, n in enumerate(counts):
        if n <= 0:
            continue
        k = -(-n // seg)
        q, r = divmod(n, k)
        a = 0
        for j in range(k):           # r segments of q + 1 pieces, then k - r of q
            segs.append((clip, a, a + q + (j < r)))
            a += q + (j < r)
    return seg, sorted(segs, key=lambda s: s[1] - s[2])   # (stable) descending size; ties: clip order, then a


def deal(units, grid, hole):
    """The table in launch order: rounds of `grid` units, forwards and backwards in turn; a short backward round is padded in front."""
    table = []
    for r in range(-(-len(units) // grid) if grid > 0 else 0):
        row = units[r * grid:(r + 1) * grid]
        table += [hole] * (grid - len(row)) + row[::-1] if r & 1 else row
    return table


def center_batches():
    for wl, f in [(256, 8), (1024, 8), (2048, 4), (512, 4)]:
        h = wl // 2
        for slots in (1, 256, 1024):
            for what, lengths in length_lists(h).items():
                yield what, lengths, wl, f, slots
        floor = 4 * f - 3
        yield "only empty clips", [0] * 7, wl, f, 4
        yield "one clip of exactly S blocks, at the floor", [floor * h], wl, f, 1
        yield "one clip of S + 1 blocks, at the floor", [floor * h + 1], wl, f, 1
        yield "clips of S - 1, S and S + 1 blocks, above the floor", [h * n for n in [39, 40, 41] + [40] * 9], wl, f, 1   # 480 blocks on 12 units: S = 40
    yield "the measured batch", np.random.default_rng(0).integers(5 * 44100, 15 * 44100 + 1, 1024).tolist(), 2048, 4, 256


def test_center_units_are_exactly_the_rule(center_cutter):
    for what, lengths, wl, f, slots in center_batches():
        h = wl // 2
        seg, segs = cut([-(-n // h) for n in lengths], 4 * f - 3, slots, CENTER_PER_SLOT)
        got_seg, got = center_cutter(lengths, wl, f, slots)
        assert got_seg == seg, what
        assert got == [(clip, a, b, lengths[clip]) for clip, a, b in segs], what


def imdct_batches():
    yield from random_batches()
    yield "the measured batch", (-(-np.random.default_rng(0).integers(5 * 44100, 15 * 44100 + 1, 1024) // 1024) + 1).tolist(), 256
    yield "only empty clips", [0, 1, 0, 1, 1], 8
    yield "one clip of exactly S tiles, at the floor", [3 * TILE], 1
    yield "one clip of S + 1 tiles, at the floor", [3 * TILE + 1], 1
    yield "clips of S - 1, S and S + 1 tiles, above the floor", [TILE * n for n in (9, 10, 11, 10)], 1   # 40 tiles on 4 units: S = 10
    yield "a backward last round with a single unit", [2] * 5, 4
    yield "a forward last round with a single unit", [2] * 9, 4


def test_imdct_units_and_table_are_exactly_the_rule(imdct_cutter):
    for what, frames, slots in imdct_batches():
        counts = [0 if t <= 1 else -(-t // TILE) for t in frames]
        seg, segs = cut(counts, 3, slots, PER_SLOT)
        units = [(clip, a, b, counts[clip], frames[clip]) for clip, a, b in segs]
        grid = min(slots, len(units))
        got_seg, got_grid, got_units, got_table = imdct_cutter(frames, slots)
        assert (got_seg, got_grid) == (seg, grid), what
        assert got_units == units, what
        assert got_table == deal(units, grid, (-1, 0, 0, 0, 0)), what


def istft_batches():
    """(what, frames, slots, W, H); the random batches with the windows and hops test_istft_ragged_host.py gives them."""
    for k, (what, frames, slots) in enumerate(istft_random_batches()):
        yield (what, frames, slots) + [(2048, 1024), (512, 128), (1024, 768), (256, 129)][k % 4]
    yield "only empty clips", [0, 1, 0, 1, 1], 8, 2048, 1024
    yield "one clip of exactly S tiles, at the floor", [3 * ISTFT_TILE], 1, 2048, 1024
    yield "one clip of S tiles + 1 frame, at the floor", [3 * ISTFT_TILE + 1], 1, 2048, 1024
    yield "a backward last round with a single unit", [2] * 5, 4, 512, 256     # (hop W / 2: a spectrum of 2 frames still has output)
    yield "a forward last round with a single unit", [2] * 9, 4, 512, 256
    yield "frames but no output: no unit", [3] * 6, 4, 512, 128               # 3 H - (W - H) = 0


def test_istft_units_and_table_are_exactly_the_rule(istft_cutter):
    for what, frames, slots, w, h in istft_batches():
        out = [max(t * h - (w - h), 0) for t in frames]
        counts = [0 if t * h - (w - h) <= 0 else -(-t // ISTFT_TILE) for t in frames]
        seg, segs = cut(counts, 3, slots, ISTFT_PER_SLOT)
        units = [(clip, a, b, counts[clip], frames[clip], out[clip], -(-frames[clip] // 16) * 16) for clip, a, b in segs]
        grid = min(slots, len(units))
        got_seg, got_grid, got_lens, got_units, got_table = istft_cutter(frames, slots, w, h)
        assert (got_seg, got_grid) == (seg, grid), what
        assert got_lens == out, what
        assert got_units == units, what
        assert got_table == deal(units, grid, (-1, 0, 0, 0, 0, 0, 0)), what
        if what.startswith("frames but no output"):
            assert frames and min(frames) > 0 and got_units == [] and got_table == [], what
        if "last round" in what:
            assert len(units) % grid == 1 and (len(units) // grid) % 2 == ("backward" in what), what


def test_the_added_batches_reach_the_edges_they_are_named_for():
    """(the rule alone, against cuts written out by hand)"""
    assert cut([3], 3, 1, PER_SLOT) == (3, [(0, 0, 3)])
    assert cut([4], 3, 1, PER_SLOT) == (3, [(0, 0, 2), (0, 2, 4)])
    assert cut([9, 10, 11, 10], 3, 1, PER_SLOT) == (10, [(1, 0, 10), (3, 0, 10), (0, 0, 9), (2, 0, 6), (2, 6, 11)])
    assert cut([39, 40, 41] + [40] * 9, 29, 1, CENTER_PER_SLOT)[0] == 40
    units = cut([1] * 5, 3, 4, PER_SLOT)[1]
    assert deal(units, 4, None) == units[:4] + [None] * 3 + units[4:]
    assert deal(cut([1] * 9, 3, 4, PER_SLOT)[1], 4, None)[8:] == [(8, 0, 1)]
