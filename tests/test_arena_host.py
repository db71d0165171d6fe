"""tests/arena.py checked on the CPU: the checker accepts a correct result and rejects each planted defect.

The executor is the oracle writing into a NumPy arena where a kernel would write into a device one; this is the proof that the
cases of tests/test_gpu_arena.py can fail."""
import numpy as np
import pytest

import arena
from conftest import relerr, synth_clip
from oracle import zaf_oracle as orc

W, HOP, N = 64, 32, 400      # T = 14 frames
TOL = 1e-5


def kinds():
    """(name, input dtype, output dtype, pitch or None, transform of one clip -> the compact float64 result)."""
    ham, kbd = orc.hamming_periodic(W), orc.kbd_window(W)
    return {
        "stft_c64_padded": (np.float32, np.complex64, 16, lambda x: orc.stft(x, ham, HOP)),
        "mdct_f32_padded": (np.float32, np.float32, 32, lambda x: orc.mdct(x, kbd)),
        "stft_c128": (np.float64, np.complex128, None, lambda x: orc.stft(x, ham, HOP)),
        "samples_f64": (np.float64, np.float64, None, lambda x: np.cumsum(x)[:-1]),   # a 1-D output of odd length
    }


class Fake:
    """One 'kernel': reads the clips out of the input arena, writes the oracle's results into the output arena."""

    def __init__(self, kind, delta_in, delta_out, defect=None):
        self.in_dtype, self.out_dtype, self.pitch, self.fn = kinds()[kind]
        self.in_dtype, self.out_dtype = np.dtype(self.in_dtype), np.dtype(self.out_dtype)
        self.delta_in, self.delta_out, self.defect = delta_in, delta_out, defect
        self.x = np.stack([synth_clip(3, c, N) for c in range(3)]).astype(self.in_dtype)
        ref = [self.fn(c.astype(np.float64)) for c in self.x]
        self.frames = ref[0].shape[-1]
        pitch = self.pitch or self.frames
        self.shape = (3,) + ref[0].shape[:-1] + (pitch,)
        self.blocks = arena.uniform_blocks(self.shape, self.frames, ref)
        out_bytes = int(np.prod(self.shape)) * self.out_dtype.itemsize
        self.guard = arena.guard_bytes(self.x[0].nbytes, out_bytes // 3)
        self.s_in = arena.Span(self.x.nbytes, self.guard, delta_in)
        self.s_out = arena.Span(out_bytes, self.guard, delta_out)

    def run(self, x):
        a_in = arena.place(self.s_in, arena.poison_word(self.in_dtype), x)
        out = arena.filled(self.s_out, arena.fill_word(self.out_dtype))
        isz, osz = self.in_dtype.itemsize, self.out_dtype.itemsize
        per = int(np.prod(self.shape[1:]))
        poisoned = bool(np.isnan(x[1]).any())
        for c in range(3):
            lo = self.s_in.lo + c * N * isz
            n_read = N + 1 if (self.defect == "reads_outside" and c == 2) else N
            clip = a_in[lo:lo + n_read * isz].copy().view(self.in_dtype).astype(np.float64)
            if n_read > N:
                clip = clip[:N] + 0.0 * clip[N]          # "masked" by a multiplication with zero
            with np.errstate(invalid="ignore"):
                res = np.asarray(self.fn(clip)).astype(self.out_dtype)
            if self.defect == "leak" and c == 0 and poisoned:
                flat = res.reshape(-1).view(arena.fill_word(self.out_dtype)[0])
                flat[5] ^= 1                             # one bit of clip 0 follows clip 1
            block = np.frombuffer(out[self.s_out.lo + c * per * osz:self.s_out.lo + (c + 1) * per * osz].tobytes(), dtype=self.out_dtype).reshape(self.shape[1:]).copy()
            block[..., :self.frames] = res
            if self.defect == "unwritten" and c == 1:
                fw = arena.fill_word(self.out_dtype)
                block[..., self.frames - 1:self.frames] = np.array([fw[1]] * (osz // fw[0].itemsize), dtype=fw[0]).view(self.out_dtype)[0]
            if self.defect == "padding" and c == 2:
                block[..., -1, self.frames] = 0
            out[self.s_out.lo + c * per * osz:self.s_out.lo + (c + 1) * per * osz] = np.frombuffer(block.tobytes(), dtype=np.uint8)
        word = 4
        if self.defect == "front":
            out[self.s_out.lo - word:self.s_out.lo] = 0
        if self.defect == "back":
            out[self.s_out.hi:self.s_out.hi + word] = 0
        return out

    def check(self):
        """What run_case does around a launch, on the fake's arenas."""
        clean = arena.check_arena(self.run(self.x), self.s_out, self.out_dtype, self.blocks, TOL, relerr)
        other = arena.check_arena(self.run(arena.poisoned_copy(self.x)), self.s_out, self.out_dtype, self.blocks, TOL, relerr, skip=(1,))
        arena.check_neighbours(clean, other, self.blocks, self.out_dtype)
        return clean


@pytest.mark.parametrize("kind", sorted(kinds()))
@pytest.mark.parametrize("delta_in,delta_out", [(0, 0), (4, 4), (128, 8), (16, 128), (64, 64), (8, 4)])
def test_checker_accepts_the_oracle(kind, delta_in, delta_out):
    f = Fake(kind, delta_in, delta_out)
    got = f.check()
    assert len(got) == 3 and got[0].shape == f.shape[1:]
    assert f.guard % 256 == 0 and f.guard >= 64 * 1024 and f.guard >= f.s_out.nbytes // 3


@pytest.mark.parametrize("kind", sorted(kinds()))
@pytest.mark.parametrize("defect,message", [("front", r"\(a\) written in front of the array: byte -"),
                                            ("back", r"\(a\) written behind the array: byte 0 past the end"),
                                            ("unwritten", r"\(b\) clip 1: \d+ elements never written"),
                                            ("reads_outside", r"\(c\) clip 2: \d+ values not finite"),
                                            ("leak", r"clip 0 depends on clip 1: 1 words differ")])
def test_checker_rejects_each_defect(kind, defect, message):
    with pytest.raises(AssertionError, match=message):
        Fake(kind, 4, 8, defect).check()


@pytest.mark.parametrize("kind", ["stft_c64_padded", "mdct_f32_padded"])
def test_checker_rejects_a_written_padding_element(kind):
    with pytest.raises(AssertionError, match=r"\(b\) clip 2: 1 row-padding elements written, the first at index \[\d+, 14\]"):
        Fake(kind, 16, 4, "padding").check()


def test_checker_rejects_a_wrong_value():
    """(c) is the oracle's bound, not only finiteness: one frame scaled by 1 + 1e-4."""
    f = Fake("stft_c64_padded", 8, 8)
    out = f.run(f.x)
    good = arena.extract(out, f.s_out, f.out_dtype, f.blocks)
    bad = good[0].copy()
    bad[:, 3] *= np.float32(1.0001)
    out[f.s_out.lo:f.s_out.lo + bad.nbytes] = np.frombuffer(bad.tobytes(), dtype=np.uint8)
    with pytest.raises(AssertionError, match=r"\(c\) clip 0: .* off the oracle"):
        arena.check_arena(out, f.s_out, f.out_dtype, f.blocks, TOL, relerr)


def test_fills_and_guards():
    assert arena.guard_bytes(1, 2) == 64 * 1024 and arena.guard_bytes(70000, 100) == 70144 and arena.guard_bytes(100, 1 << 20) == 1 << 20
    for delta in (0, 4, 8, 12):
        s = arena.Span(64, arena.MIN_GUARD, delta)
        a = arena.filled(s, arena.fill_word(np.complex128))
        assert a.shape == (s.total,) and (a[s.lo:s.hi].copy().view(np.uint64) == arena.FILL64).all()   # in phase with element 0 at any offset
        assert np.isnan(a[s.lo:s.hi].copy().view(np.float64)).all()
    p = arena.filled(arena.Span(8, arena.MIN_GUARD, 2), arena.poison_word(np.int16))
    assert (p[arena.MIN_GUARD + 2:arena.MIN_GUARD + 10].copy().view(np.int16) == -32768).all()
    assert np.isnan(arena.filled(arena.Span(8, arena.MIN_GUARD, 4), arena.poison_word(np.complex64))[arena.MIN_GUARD + 4:][:8].copy().view(np.float32)).all()
    with pytest.raises(ValueError):
        arena.Span(8, 1000, 0)


# ------------------------------------------------------------------------------------------------ gap blocks
def gapped(delta_out=4):
    """Three 1-D clips of 50, 1 and 33 float32 samples at caller-chosen places -- gaps of 1 and 3 elements between them and a tail of 2 --, as
    the ragged center and IMDCT entry points write them: the blocks, the span and a clean arena with the oracle's numbers in the clips."""
    ref = [np.cumsum(synth_clip(5, c, n).astype(np.float64)) for c, n in enumerate((50, 1, 33))]
    blocks = [arena.Block(0, (50,), 50, ref[0]), arena.gap_block(50, 1), arena.Block(51, (1,), 1, ref[1]), arena.gap_block(52, 3),
              arena.Block(55, (33,), 33, ref[2]), arena.gap_block(88, 2)]
    span = arena.Span(90 * 4, arena.guard_bytes(200, 200), delta_out)
    out = arena.filled(span, arena.fill_word(np.float32))
    for b in blocks:
        if not arena.is_gap(b):
            out[span.lo + 4 * b.offset:span.lo + 4 * (b.offset + b.frames)] = np.frombuffer(b.ref.astype(np.float32).tobytes(), dtype=np.uint8)
    return blocks, span, out


def test_gap_blocks_accept_a_clean_arena():
    blocks, span, out = gapped()
    got = arena.check_arena(out, span, np.float32, blocks, TOL, relerr)
    assert [g.shape for g in got] == [(50,), (1,), (1,), (3,), (33,), (2,)]
    other = arena.check_arena(out, span, np.float32, blocks, TOL, relerr, skip=(2,))
    arena.check_neighbours(got, other, blocks, np.float32, middle=2)


@pytest.mark.parametrize("at,message", [(50, r"\(a\) written into the gap in front of block 2: 1 words changed, the first at element 50 of the array"),
                                        (54, r"\(a\) written into the gap in front of block 4: 1 words changed, the first at element 54"),
                                        (89, r"\(a\) written into the gap in front of block 6: 1 words changed, the first at element 89"),
                                        (-1, r"\(a\) written in front of the array: byte -4"),
                                        (90, r"\(a\) written behind the array: byte 0 past the end")])
def test_gap_blocks_report_a_write(at, message):
    """One float32 zero written into a gap, in front of the array and behind it: each is reported where it is."""
    blocks, span, out = gapped()
    out[span.lo + 4 * at:span.lo + 4 * at + 4] = 0
    with pytest.raises(AssertionError, match=message):
        arena.check_arena(out, span, np.float32, blocks, TOL, relerr)


def test_gap_blocks_still_find_an_unwritten_element_and_a_leak():
    blocks, span, out = gapped()
    clean = arena.check_arena(out, span, np.float32, blocks, TOL, relerr)
    bad = out.copy()
    bad[span.lo + 4 * 60:span.lo + 4 * 61] = np.frombuffer(np.array([arena.FILL32], np.uint32).tobytes(), dtype=np.uint8)
    with pytest.raises(AssertionError, match=r"\(b\) clip 4: 1 elements never written, the first at index \[5\]"):
        arena.check_arena(bad, span, np.float32, blocks, TOL, relerr)
    leak = out.copy()
    leak[span.lo + 4 * 70] ^= 1
    other = arena.check_arena(leak, span, np.float32, blocks, TOL, relerr, skip=(2,))
    with pytest.raises(AssertionError, match=r"clip 4 depends on clip 2: 1 words differ"):
        arena.check_neighbours(clean, other, blocks, np.float32, middle=2)
