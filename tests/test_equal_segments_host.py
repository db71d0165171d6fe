"""center_equal_segments and maskfilter_equal_segments (zafx_units.hpp; no GPU): the cut of an equal-length batch's clips into segments for
k_center, k_maskfilter and k_maskfilter_stems.  The functions as g++ compiles them (tests/host_emu/equal_segments_emu.cpp) against the invariants
the kernels rely on and against a table of the values the launchers computed when each carried the rule itself."""
import os
import subprocess

import pytest

from conftest import ROOT

TILES = (8, 4)   # F = center_tile_frames = maskfilter_tile_transforms at W = 256 and W = 2048
SLOTS = (1, 4, 1024)
SRC = os.path.join(ROOT, "tests", "host_emu", "equal_segments_emu.cpp")
INC = os.path.join(ROOT, "zaf-python_amd", "csrc")


def blocks(f):
    return (1, 2, 4 * f - 3, 4 * f - 2, 4 * f - 1, 60, 861)


def clips(slots):
    return sorted({c for c in (1, 3, slots - 1, slots) if c >= 1})


# {(F, slots, n_clips): the (seg_blocks, segs) of n_blocks in blocks(F)}, from the formulas as run_center and run_maskfilter held them,
# compiled on their own
CENTER = {
    (8, 1, 1): ((1, 1), (2, 1), (29, 1), (30, 1), (31, 1), (60, 1), (861, 1),),
    (8, 1, 3): ((1, 1), (2, 1), (29, 1), (30, 1), (31, 1), (60, 1), (861, 1),),
    (8, 4, 1): ((1, 1), (2, 1), (29, 1), (15, 2), (16, 2), (15, 4), (108, 8),),
    (8, 4, 3): ((1, 1), (2, 1), (29, 1), (15, 2), (16, 2), (20, 3), (287, 3),),
    (8, 4, 4): ((1, 1), (2, 1), (29, 1), (30, 1), (31, 1), (60, 1), (861, 1),),
    (8, 1024, 1): ((1, 1), (2, 1), (29, 1), (15, 2), (16, 2), (15, 4), (16, 54),),
    (8, 1024, 3): ((1, 1), (2, 1), (29, 1), (15, 2), (16, 2), (15, 4), (16, 54),),
    (8, 1024, 1023): ((1, 1), (2, 1), (29, 1), (15, 2), (16, 2), (20, 3), (287, 3),),
    (8, 1024, 1024): ((1, 1), (2, 1), (29, 1), (30, 1), (31, 1), (60, 1), (861, 1),),
    (4, 1, 1): ((1, 1), (2, 1), (13, 1), (14, 1), (15, 1), (60, 1), (861, 1),),
    (4, 1, 3): ((1, 1), (2, 1), (13, 1), (14, 1), (15, 1), (60, 1), (861, 1),),
    (4, 4, 1): ((1, 1), (2, 1), (13, 1), (7, 2), (8, 2), (8, 8), (108, 8),),
    (4, 4, 3): ((1, 1), (2, 1), (13, 1), (7, 2), (8, 2), (20, 3), (287, 3),),
    (4, 4, 4): ((1, 1), (2, 1), (13, 1), (14, 1), (15, 1), (60, 1), (861, 1),),
    (4, 1024, 1): ((1, 1), (2, 1), (13, 1), (7, 2), (8, 2), (8, 8), (7, 123),),
    (4, 1024, 3): ((1, 1), (2, 1), (13, 1), (7, 2), (8, 2), (8, 8), (7, 123),),
    (4, 1024, 1023): ((1, 1), (2, 1), (13, 1), (7, 2), (8, 2), (20, 3), (287, 3),),
    (4, 1024, 1024): ((1, 1), (2, 1), (13, 1), (14, 1), (15, 1), (60, 1), (861, 1),),
}
MASKFILTER = {
    (8, 1, 1): ((2, 1), (2, 1), (30, 1), (30, 1), (32, 1), (60, 1), (862, 1),),
    (8, 1, 3): ((2, 1), (2, 1), (30, 1), (30, 1), (32, 1), (60, 1), (862, 1),),
    (8, 4, 1): ((2, 1), (2, 1), (30, 1), (30, 1), (30, 2), (30, 2), (110, 8),),
    (8, 4, 3): ((2, 1), (2, 1), (30, 1), (30, 1), (30, 2), (30, 2), (302, 3),),
    (8, 4, 4): ((2, 1), (2, 1), (30, 1), (30, 1), (32, 1), (60, 1), (862, 1),),
    (8, 1024, 1): ((2, 1), (2, 1), (30, 1), (30, 1), (30, 2), (30, 2), (30, 29),),
    (8, 1024, 3): ((2, 1), (2, 1), (30, 1), (30, 1), (30, 2), (30, 2), (30, 29),),
    (8, 1024, 1023): ((2, 1), (2, 1), (30, 1), (30, 1), (30, 2), (30, 2), (302, 3),),
    (8, 1024, 1024): ((2, 1), (2, 1), (30, 1), (30, 1), (32, 1), (60, 1), (862, 1),),
    (4, 1, 1): ((2, 1), (2, 1), (14, 1), (14, 1), (16, 1), (60, 1), (862, 1),),
    (4, 1, 3): ((2, 1), (2, 1), (14, 1), (14, 1), (16, 1), (60, 1), (862, 1),),
    (4, 4, 1): ((2, 1), (2, 1), (14, 1), (14, 1), (14, 2), (14, 5), (110, 8),),
    (4, 4, 3): ((2, 1), (2, 1), (14, 1), (14, 1), (14, 2), (22, 3), (294, 3),),
    (4, 4, 4): ((2, 1), (2, 1), (14, 1), (14, 1), (16, 1), (60, 1), (862, 1),),
    (4, 1024, 1): ((2, 1), (2, 1), (14, 1), (14, 1), (14, 2), (14, 5), (14, 62),),
    (4, 1024, 3): ((2, 1), (2, 1), (14, 1), (14, 1), (14, 2), (14, 5), (14, 62),),
    (4, 1024, 1023): ((2, 1), (2, 1), (14, 1), (14, 1), (14, 2), (22, 3), (294, 3),),
    (4, 1024, 1024): ((2, 1), (2, 1), (14, 1), (14, 1), (16, 1), (60, 1), (862, 1),),
}


def _cut(exe):
    """{(rule, F, slots, n_clips, n_blocks): (seg_blocks, segs)} over the table's cases, as the program `exe` gives them."""
    out = {}
    for rule in ("center", "maskfilter"):
        for f in TILES:
            for slots in SLOTS:
                cases = [(c, b) for c in clips(slots) for b in blocks(f)]
                res = subprocess.run([str(exe), rule, str(f), str(slots)] + [str(v) for case in cases for v in case], capture_output=True, text=True)
                assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
                rows = [tuple(int(v) for v in ln.split()) for ln in res.stdout.splitlines()]
                assert len(rows) == len(cases)
                out.update({(rule, f, slots, c, b): row for (c, b), row in zip(cases, rows)})
    return out


@pytest.fixture(scope="module")
def cut(tmp_path_factory):
    exe = tmp_path_factory.mktemp("equal_segments") / "equal_segments_emu"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", INC, SRC, "-o", str(exe)], check=True)
    return _cut(exe)


def test_the_table(cut):
    for rule, want in (("center", CENTER), ("maskfilter", MASKFILTER)):
        assert sorted(want) == [(f, s, c) for f in sorted(TILES) for s in SLOTS for c in clips(s)]
        for (f, slots, c), row in want.items():
            assert tuple(cut[(rule, f, slots, c, b)] for b in blocks(f)) == row, (rule, f, slots, c)


def test_no_empty_last_segment(cut):
    for (rule, f, slots, c, b), (seg_blocks, segs) in cut.items():
        assert seg_blocks >= 1 and segs == -(-b // seg_blocks), (rule, f, slots, c, b, seg_blocks, segs)


def test_whole_clips_when_the_clips_fill_the_slots(cut):
    seen = 0
    for (rule, f, slots, c, b), (seg_blocks, segs) in cut.items():
        if c >= slots:
            assert segs == 1, (rule, f, slots, c, b, seg_blocks, segs)
            seen += 1
    assert seen


def test_maskfilter_segments_are_even_and_a_cut_clip_fills_whole_tiles(cut):
    """A segment starts on a transform of its own (seg_blocks even); a cut clip's segments are 2 F m - 2 blocks, m >= 2: with the halo m full tiles."""
    n_cut = 0
    for (rule, f, slots, c, b), (seg_blocks, segs) in cut.items():
        if rule != "maskfilter":
            continue
        assert seg_blocks % 2 == 0, (f, slots, c, b, seg_blocks)
        if segs > 1:
            m, r = divmod(seg_blocks + 2, 2 * f)
            assert r == 0 and m >= 2, (f, slots, c, b, seg_blocks, segs)
            n_cut += 1
    assert n_cut


def test_center_segments_keep_two_tiles(cut):
    """The segment length of a cut clip is never below 2 F - 1 blocks, and a clip below 2 (2 F - 1) is one segment.  (The length is the rule's
    seg_blocks: a clip's last segment is what the others leave, never empty -- test_no_empty_last_segment -- but as short as 13 of 15 blocks
    for 861 blocks in 54 segments at F = 8, which the table holds as the launcher always cut it.)"""
    n_cut = 0
    for (rule, f, slots, c, b), (seg_blocks, segs) in cut.items():
        if rule != "center":
            continue
        if segs > 1:
            assert seg_blocks >= 2 * f - 1 and b >= 2 * (2 * f - 1), (f, slots, c, b, seg_blocks, segs)
            n_cut += 1
        else:
            assert seg_blocks == b
    assert n_cut


def test_under_the_sanitizers(tmp_path_factory, cut):
    """The same stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, run as such: a clean exit and the same values."""
    exe = tmp_path_factory.mktemp("equal_segments_san") / "equal_segments_emu_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC, SRC,
                    "-o", str(exe)], check=True)
    assert _cut(exe) == cut
