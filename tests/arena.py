"""Device arrays carved out of a larger allocation: the harness of tests/test_gpu_arena.py (checked on the CPU by tests/test_arena_host.py).

The C-ABI takes any device pointer, and the launchers branch on its address in about sixty places; a fresh allocation always
sits on a 256-byte boundary, so only one outcome of those branches runs on one.  Here the caller's arrays are VIEWS at a byte
offset inside an arena this module owns:

    input arena    guard | delta_in  | input  | guard     filled with quiet NaNs (int16 / int32 PCM: the most negative value)
    output arena   guard | delta_out | output | guard     filled with a NaN of one fixed payload (FILL32 / FILL64)

`guard` (guard_bytes) is a multiple of 256 bytes, at least 64 KiB and at least one clip's input or output block: a stray access
of up to a whole clip stays inside memory the test owns.  That is a condition of the harness, not a tuning value.

The checking half is plain NumPy on the downloaded bytes (check_arena, check_neighbours); the running half (run_in_arena) takes
the zafx module as an argument, so this file imports nothing from the GPU side and no test of it needs one:

    (a) every byte outside [guard + delta_out, guard + delta_out + out_bytes) is bit-identical to the fill,
    (b) no element inside the array still carries the fill -- except the row padding of a row_align plan, all of which must,
    (c) the values are finite and within `tol` (normwise per clip, conftest.relerr) of the float64 oracle,
    and, in a second pass at the same addresses with the middle clip poisoned (NaN), every other clip is bit-identical.

Entry points that put every clip's result where the caller says (zafx_execute_center_ragged, zafx_execute_imdct_ragged) leave room between the
blocks: a GAP is a Block of `frames` = 0 (gap_block), every element of which must still carry the fill -- reported as (a), a write outside the
clips.  Blocks and gaps together tile the array.

NaN payloads do not survive `==`: everything is compared as integers."""
import ctypes
from collections import namedtuple

import numpy as np

FILL32 = 0x7FC5A5A5            # a quiet float32 NaN no kernel computes
FILL64 = 0x7FF8A5A5A5A5A5A5    # its float64 analogue
MIN_GUARD = 64 * 1024

# One clip's part of the output array: `offset` elements into the array, `shape` (rows, pitch) or (samples,), the first `frames` elements of
# the last axis are the clip's (the rest is row padding), `ref` the oracle's compact result (shape[:-1] + (frames,)).
Block = namedtuple("Block", "offset shape frames ref")


def gap_block(offset, elems):
    """`elems` elements at `offset` that belong to no clip: nothing may be written there."""
    return Block(int(offset), (int(elems),), 0, None)


def is_gap(block):
    return block.frames == 0 and block.ref is None


def guard_bytes(*clip_bytes):
    """The guard for clips of these input / output sizes: >= 64 KiB, >= each of them, a multiple of 256."""
    g = max((MIN_GUARD,) + tuple(int(b) for b in clip_bytes))
    return -(-g // 256) * 256


def fill_word(dtype):
    """(unsigned integer dtype, value) of the OUTPUT arena's fill for arrays of `dtype` (complex: seen through their real view)."""
    dtype = np.dtype(dtype)
    real = dtype.itemsize // 2 if dtype.kind == "c" else dtype.itemsize
    if dtype.kind not in "fc" or real not in (4, 8):
        raise ValueError(f"no output fill for {dtype}")
    return (np.dtype(np.uint32), FILL32) if real == 4 else (np.dtype(np.uint64), FILL64)


def poison_word(dtype):
    """(unsigned integer dtype, value) of the INPUT arena's fill: a quiet NaN; the most negative value of an integer PCM type."""
    dtype = np.dtype(dtype)
    if dtype.kind == "i":
        return np.dtype(f"u{dtype.itemsize}"), 1 << (8 * dtype.itemsize - 1)
    real = dtype.itemsize // 2 if dtype.kind == "c" else dtype.itemsize
    return (np.dtype(np.uint32), 0x7FC00000) if real == 4 else (np.dtype(np.uint64), 0x7FF8000000000000)


def poison_value(dtype):
    """What a poisoned clip holds: NaN (complex: both parts), the most negative value of an integer type."""
    dtype = np.dtype(dtype)
    return np.iinfo(dtype).min if dtype.kind == "i" else np.nan


class Span:
    """Where an array of `nbytes` lies in its arena: [lo, hi) of `total` bytes."""

    def __init__(self, nbytes, guard, delta):
        if guard % 256 or guard < MIN_GUARD or delta < 0:
            raise ValueError("the guard is a multiple of 256 bytes of at least 64 KiB")
        self.nbytes, self.guard, self.delta = int(nbytes), int(guard), int(delta)
        self.lo = self.guard + self.delta
        self.hi = self.lo + self.nbytes
        self.total = self.hi + self.guard


def filled(span, word):
    """The arena's bytes before anything ran: `word` repeated, in phase with the array's first element."""
    wdtype, value = word
    wb = np.frombuffer(np.array([value], dtype=wdtype).tobytes(), dtype=np.uint8)
    ws = len(wb)
    start = (-span.lo) % ws
    return np.tile(wb, span.total // ws + 2)[start:start + span.total].copy()


def place(span, word, array):
    """The input arena: the fill with `array`'s bytes at [lo, hi)."""
    a = np.ascontiguousarray(array)
    if a.nbytes != span.nbytes:
        raise ValueError("array and span differ in size")
    arena = filled(span, word)
    arena[span.lo:span.hi] = np.frombuffer(a.tobytes(), dtype=np.uint8)
    return arena


def uniform_blocks(shape, frames, ref):
    """Blocks of a batch whose clips are all alike: `shape` = (clips,) + one clip's shape, ref[c] the oracle's result of clip c."""
    per = int(np.prod(shape[1:], dtype=np.int64))
    frames = shape[-1] if frames is None else int(frames)
    return [Block(c * per, tuple(shape[1:]), frames, np.asarray(ref[c])) for c in range(shape[0])]


def _first(mask):
    return int(np.flatnonzero(mask)[0])


def extract(arena, span, dtype, blocks):
    """The clips' results as the kernel left them: a list of arrays of the blocks' shapes (padding included)."""
    dtype = np.dtype(dtype)
    flat = arena[span.lo:span.hi].copy().view(dtype)
    return [flat[b.offset:b.offset + int(np.prod(b.shape, dtype=np.int64))].reshape(b.shape) for b in blocks]


def check_arena(arena, span, dtype, blocks, tol, relerr, skip=()):
    """Assertions (a), (b), (c) of the module docstring on the downloaded output arena (uint8, span.total bytes).  Clips listed in `skip`
    (the poisoned one of the second pass) are exempt from (c); -> the clips' results (extract)."""
    dtype = np.dtype(dtype)
    word = fill_word(dtype)
    wdtype, value = word
    arena = np.asarray(arena, dtype=np.uint8)
    assert arena.shape == (span.total,), (arena.shape, span.total)
    assert sum(int(np.prod(b.shape, dtype=np.int64)) for b in blocks) * dtype.itemsize == span.nbytes, "the blocks must tile the array"
    # (a) nothing outside the array
    clean = filled(span, word)
    front = arena[:span.lo] != clean[:span.lo]
    assert not front.any(), f"(a) written in front of the array: byte {_first(front) - span.lo} (relative to element 0), {int(front.sum())} bytes changed"
    back = arena[span.hi:] != clean[span.hi:]
    assert not back.any(), f"(a) written behind the array: byte {_first(back)} past the end, {int(back.sum())} bytes changed"
    got = extract(arena, span, dtype, blocks)
    words = dtype.itemsize // wdtype.itemsize   # (2 for complex)
    for c, (b, g) in enumerate(zip(blocks, got)):
        if is_gap(b):
            # (a) for the room between two clips: every WORD still the fill (complex: both parts)
            hit = np.ascontiguousarray(g).view(wdtype) != value
            assert not hit.any(), f"(a) written into the gap in front of block {c + 1}: {int(hit.sum())} words changed, the first at element {b.offset + _first(hit) // words} of the array"
            continue
        carries = (np.ascontiguousarray(g).view(wdtype).reshape(g.shape + (words,)) == value).any(axis=-1)
        inside, padding = carries[..., :b.frames], carries[..., b.frames:]
        # (b) every element written, no padding element written
        assert not inside.any(), f"(b) clip {c}: {int(inside.sum())} elements never written, the first at index {np.argwhere(inside)[0].tolist()} of {g.shape}"
        if not padding.all():
            at = np.argwhere(~padding)[0]
            at[-1] += b.frames
            raise AssertionError(f"(b) clip {c}: {int((~padding).sum())} row-padding elements written, the first at index {at.tolist()} of {g.shape}")
        if c in skip:
            continue
        # (c) finite, and the oracle's numbers
        val = g[..., :b.frames]
        bad = ~np.isfinite(val)
        assert not bad.any(), f"(c) clip {c}: {int(bad.sum())} values not finite, the first at index {np.argwhere(bad)[0].tolist()} of {val.shape}"
        assert val.shape == b.ref.shape, (c, val.shape, b.ref.shape)
        err = relerr(val, b.ref)
        assert err <= tol, f"(c) clip {c}: {err:.3e} off the oracle, bound {tol:.1e}"
    return got


def check_neighbours(clean, poisoned, blocks, dtype, middle=1):
    """The poisoned-neighbour pass: every clip but `middle` bit-identical to the clean pass (the clips' elements; padding is (b)'s)."""
    wdtype = fill_word(dtype)[0]
    for c, (b, a, p) in enumerate(zip(blocks, clean, poisoned)):
        if c == middle or is_gap(b):
            continue
        a = np.ascontiguousarray(a[..., :b.frames]).view(wdtype)
        p = np.ascontiguousarray(p[..., :b.frames]).view(wdtype)
        diff = a != p
        assert not diff.any(), f"clip {c} depends on clip {middle}: {int(diff.sum())} words differ once that clip is poisoned, the first at index {np.argwhere(diff)[0].tolist()}"


# --------------------------------------------------------------------------------------------- the running half (needs the zafx module)
def run_in_arena(zafx, x, out_dtype, out_elems, guard, delta_in, delta_out, launch):
    """Upload `x` into an input arena at `delta_in`, carve an output array of `out_elems` x `out_dtype` at `delta_out`, call
    launch(d_in, d_out) -- which enqueues AND syncs --, download the whole output arena: -> (bytes, span).  The views' pointers are
    cleared before they die (views, not allocations: nothing to free)."""
    x = np.ascontiguousarray(x)
    out_dtype = np.dtype(out_dtype)
    s_in = Span(x.nbytes, guard, delta_in)
    s_out = Span(int(out_elems) * out_dtype.itemsize, guard, delta_out)
    if delta_in % min(x.dtype.itemsize, 4) or delta_out % 4:
        raise ValueError("offsets are multiples of 4 bytes (2 for int16 input)")
    a_in = zafx.DeviceBuffer.from_host(place(s_in, poison_word(x.dtype), x))
    a_out = zafx.DeviceBuffer.from_host(filled(s_out, fill_word(out_dtype)))
    v_in = zafx.DeviceBuffer(x.shape, x.dtype, _ptr_from_pool=ctypes.c_void_p(a_in.ptr.value + s_in.lo))
    v_out = zafx.DeviceBuffer((int(out_elems),), out_dtype, _ptr_from_pool=ctypes.c_void_p(a_out.ptr.value + s_out.lo))
    try:
        launch(v_in, v_out)
        arena = a_out.download()
    finally:
        v_in.ptr = ctypes.c_void_p()
        v_out.ptr = ctypes.c_void_p()
        a_in.free()
        a_out.free()
    return arena, s_out


def poisoned_copy(x, middle=1):
    y = np.array(x, copy=True)
    y[middle] = poison_value(y.dtype)
    return y


def run_case(zafx, x, out_dtype, blocks, guard, deltas, launch, tol, relerr, poisoned=None, exact=None, exact_tol=0.0, middle=1):
    """One array pair at one (delta_in, delta_out): the clean pass with (a), (b), (c), then the poisoned-neighbour pass with (a), (b) and the
    bit comparison of clips 0 and 2.  `poisoned`: the input of the second pass (default: clip 1 of `x` all NaN).  `exact` (integer PCM):
    the same call's result on a plain allocation -- the clean pass must equal it bit for bit (exact_tol 0: the same kernel form ran there) or
    within exact_tol normwise (another form of the kernel: same frames, other rounding order).  `middle`: the poisoned clip's index in `blocks`
    (gaps count); None: no second pass (a case without a neighbour to poison)."""
    out_elems = sum(int(np.prod(b.shape, dtype=np.int64)) for b in blocks)
    arena, span = run_in_arena(zafx, x, out_dtype, out_elems, guard, deltas[0], deltas[1], launch)
    clean = check_arena(arena, span, out_dtype, blocks, tol, relerr)
    if exact is not None:
        wdtype = fill_word(out_dtype)[0]
        want = np.ascontiguousarray(exact).reshape(-1).view(wdtype)
        have = arena[span.lo:span.hi].copy().view(wdtype)
        if exact_tol:
            err = relerr(arena[span.lo:span.hi].copy().view(out_dtype), np.ascontiguousarray(exact).reshape(-1))
            assert err <= exact_tol, f"{err:.3e} off the same call on a plain allocation, bound {exact_tol:.1e}"
        else:
            assert np.array_equal(have, want), "differs bitwise from the same call on a plain allocation"
    if middle is None:
        return clean
    arena2, span2 = run_in_arena(zafx, poisoned_copy(x) if poisoned is None else poisoned, out_dtype, out_elems, guard, deltas[0], deltas[1], launch)
    other = check_arena(arena2, span2, out_dtype, blocks, tol, relerr, skip=(middle,))
    check_neighbours(clean, other, blocks, out_dtype, middle)
    return clean
