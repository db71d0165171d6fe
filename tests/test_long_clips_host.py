"""tests/long_clips.py without a GPU: what makes tests/test_gpu_long_clips.py trustworthy.

  * periodic_reference equals the plain oracle on the whole clip, to 1e-12, for every kind, at W = 64 and 256 with q = 7 over 40 - 60 frames,
    at lengths that end on a hop, one sample behind, one sample in front of one and in the middle of one;
  * the checker finds what was done to a doctored array, at its index: a frame off by 1e-3, an element left at the fill, a padding element
    written, a result shifted by one frame, two frames 2^k apart swapped, and (the mutation of the ISTFT bound) a frame whose rows
    beyond a wrapped 32-bit byte offset came from 2^31 bytes further down;
  * every BOUNDS record brackets its condition."""
import ctypes

import numpy as np
import pytest

import arena
import long_clips as lc
from oracle import zaf_oracle as orc

FS = 8000


def _prm(kind, wl):
    w = orc.hamming_periodic(wl)
    if kind in ("mdct", "imdct"):
        return dict(w=orc.kbd_window(wl)), wl // 2
    if kind in ("cqt", "chroma"):
        ck = orc.cqtkernel(FS, 4, 500, 2000)   # (8 bins, 256-point frames)
        return dict(fs=FS, tr=FS // (wl // 4), ck=ck, octave=4), wl // 4
    if kind == "center":
        return dict(w=w), wl // 2
    hop = wl // 2 if kind in ("stft", "istft", "mel", "mel_mfcc") else wl // 4 if kind in ("stft_one_sided", "istft_one_sided", "mfcc") else wl
    prm = dict(w=w, hop=hop)
    if kind in ("mel", "mfcc", "mel_mfcc"):
        prm.update(fb=orc.melfilterbank(FS, wl, 12), ncoef=5)
    return prm, hop


@pytest.mark.parametrize("ends", ["on_a_hop", "one_behind", "one_in_front", "mid_hop"])
@pytest.mark.parametrize("wl", [64, 256])
@pytest.mark.parametrize("kind", lc.KINDS)
def test_periodic_reference_is_the_plain_oracle(kind, wl, ends):
    prm, step = _prm(kind, wl)
    p = lc.period_block(step, channels=2 if kind == "center" else 1).astype(np.float64)
    n = 47 * step + {"on_a_hop": 0, "one_behind": 1, "one_in_front": step - 1, "mid_hop": step // 2 + 3}[ends]
    ref = lc.periodic_reference(kind, p, n, **prm)
    want = lc.plain_oracle(kind, lc.periodic_clip(p, n), **prm)
    assert 40 <= ref.frames <= 60 and ref.last - ref.first >= 3 * lc.Q, (ref.frames, ref.first, ref.last)   # (the pieces are in use, not the fallback)
    assert ref.small.shape[1] < ref.frames // 2
    got = ref(0, ref.frames)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # lazily, any range of frames and rows
    assert np.array_equal(ref(11, 29, 1, 4), got[1:4, 11:29])
    if kind in lc.INVERSE or kind == "center":
        assert np.array_equal(ref.hops(5, 9), got[:, 5:9].T)
        if kind == "imdct":
            expected = step * (lc.frames_of("mdct", n, **prm) - 1) - 1    # zaf.py:1182
        elif kind == "center":
            expected = n
        else:
            expected = lc.frames_of("stft", n, **prm) * step - (wl - step)   # zaf.py:236-238
        assert ref.n_out == expected, (kind, ref.n_out, expected)


def test_the_sides_are_what_the_center_leaves():
    w = orc.hamming_periodic(256)
    p = lc.period_block(128, channels=2).astype(np.float64)
    n = 47 * 128 + 67
    center, sides = lc.periodic_reference("center", p, n, w=w), lc.periodic_reference("center", p, n, w=w, sides=True)
    x = lc.periodic_clip(p, n)
    hops = np.pad(x, ((0, 48 * 128 - n), (0, 0))).reshape(48, 256).T
    assert sides.frames == center.frames == 48 and sides.last > sides.first
    assert np.abs(sides(0, 48) - (hops - center(0, 48))).max() <= 1e-12 * np.abs(hops).max()


def test_a_short_clip_takes_the_plain_oracle():
    prm, step = _prm("stft", 64)
    p = lc.period_block(step).astype(np.float64)
    ref = lc.periodic_reference("stft", p, 5 * step + 3, **prm)
    assert ref.last == ref.first == 0
    assert np.array_equal(ref(0, ref.frames), orc.stft(lc.periodic_clip(p, 5 * step + 3), prm["w"], step))


# ------------------------------------------------------------------------------------------------------------ the checker on doctored arrays
W, HOP, N = 256, 128, 128 * 300 + 17
ALIGN = 16


@pytest.fixture(scope="module")
def spectrum():
    """A float32 `device result` of 302 frames at a pitch of 304: the oracle's values rounded, the padding at the fill."""
    p = lc.period_block(HOP)
    ref = lc.periodic_reference("stft", p, N, w=orc.hamming_periodic(W), hop=HOP)
    pitch = -(-ref.frames // ALIGN) * ALIGN
    out = np.empty((ref.rows, pitch), np.complex64)
    out.view(np.uint32)[:] = arena.FILL32
    out[:, :ref.frames] = ref(0, ref.frames)
    return ref, out


def _check(ref, out):
    return lc.check_frames(out, ref, lc.TOL_FFT, lc.floor_of("stft", ref), chunk_rows=37)


def test_the_clean_array_passes(spectrum):
    ref, out = spectrum
    assert _check(ref, out) < 0.1   # (rounding to float32: 6e-8 of a bound of 1e-5)


def test_one_frame_off_by_1e_3(spectrum):
    ref, out = spectrum
    bad = out.copy()
    bad[:, 171] *= np.float32(1.001)
    with pytest.raises(lc.LongClipFailure) as e:
        _check(ref, bad)
    assert (e.value.what, e.value.frame) == ("bound", 171)
    # ONE element of that frame, its loudest bin
    bad = out.copy()
    row = int(np.abs(out[:, 171]).argmax())
    bad[row, 171] *= np.float32(1.001)
    with pytest.raises(lc.LongClipFailure) as e:
        _check(ref, bad)
    assert (e.value.what, e.value.frame) == ("bound", 171) and "1 frames" in str(e.value)


def test_one_element_left_at_the_fill(spectrum):
    ref, out = spectrum
    bad = out.copy()
    bad.view(np.uint32).reshape(ref.rows, -1, 2)[77, 259, 1] = arena.FILL32   # (the imaginary part alone)
    with pytest.raises(lc.LongClipFailure) as e:
        _check(ref, bad)
    assert (e.value.what, e.value.frame, e.value.row) == ("fill", 259, 77)


def test_one_value_not_finite(spectrum):
    ref, out = spectrum
    for value in (np.nan, np.inf, complex(0, -np.inf)):
        bad = out.copy()
        bad[201, 17] = value
        with pytest.raises(lc.LongClipFailure) as e:
            _check(ref, bad)
        assert (e.value.what, e.value.frame, e.value.row) == ("finite", 17, 201)


def test_one_padding_element_written(spectrum):
    ref, out = spectrum
    bad = out.copy()
    bad[130, ref.frames + 1] = 0
    with pytest.raises(lc.LongClipFailure) as e:
        _check(ref, bad)
    assert (e.value.what, e.value.frame, e.value.row) == ("padding", ref.frames + 1, 130)


def test_a_result_shifted_by_one_frame(spectrum):
    ref, out = spectrum
    bad = out.copy()
    bad[:, 1:ref.frames] = out[:, :ref.frames - 1]
    with pytest.raises(lc.LongClipFailure) as e:
        _check(ref, bad)
    assert (e.value.what, e.value.frame) == ("bound", 1)   # (frame 0 is in its place)


@pytest.mark.parametrize("k", [0, 3, 6, 8])
def test_two_frames_swapped(spectrum, k):
    """No power of two is a multiple of q = 7: frames t and t + 2^k never share a reference column."""
    ref, out = spectrum
    t = 33
    bad = out.copy()
    bad[:, [t, t + (1 << k)]] = out[:, [t + (1 << k), t]]
    with pytest.raises(lc.LongClipFailure) as e:
        _check(ref, bad)
    assert (e.value.what, e.value.frame) == ("bound", t)
    assert "2 frames" in str(e.value)


def test_rows_never_compared(spectrum):
    ref, out = spectrum
    ck = lc.FrameChecker(ref, lc.TOL_FFT, lc.floor_of("stft", ref))
    ck.add(0, out[:200])
    with pytest.raises(lc.LongClipFailure) as e:
        ck.finish()
    assert (e.value.what, e.value.row) == ("coverage", 200)


def test_the_hop_checker_on_doctored_samples():
    p = lc.period_block(HOP)
    ref = lc.periodic_reference("istft", p, N, w=orc.hamming_periodic(W), hop=HOP)
    y = ref.hops(0, ref.frames).reshape(-1)[:ref.n_out].astype(np.float32)
    floor = lc.floor_of("istft", ref)
    assert ref.n_out % HOP == 0 and lc.check_hops(y, ref, lc.TOL_FFT, floor) < 0.1
    bad = y.copy()
    bad[HOP * 123 + 5] += np.float32(1e-3)
    with pytest.raises(lc.LongClipFailure) as e:
        lc.check_hops(bad, ref, lc.TOL_FFT, floor)
    assert (e.value.what, e.value.frame) == ("bound", 123)
    bad = y.copy()
    bad.view(np.uint32)[HOP * 250 + 127] = arena.FILL32
    with pytest.raises(lc.LongClipFailure) as e:
        lc.check_hops(bad, ref, lc.TOL_FFT, floor)
    assert (e.value.what, e.value.frame, e.value.row) == ("fill", 250, 127)
    bad = np.roll(y, HOP)
    with pytest.raises(lc.LongClipFailure) as e:
        lc.check_hops(bad, ref, lc.TOL_FFT, floor)
    assert (e.value.what, e.value.frame) == ("bound", 0)
    with pytest.raises(lc.LongClipFailure) as e:
        lc.check_hops(y[:-HOP], ref, lc.TOL_FFT, floor)
    assert e.value.what == "coverage"
    # an IMDCT result ends one sample short of a hop: the short last hop is compared, not skipped
    kbd = orc.kbd_window(W)
    ref = lc.periodic_reference("imdct", p, N, w=kbd)
    y = ref.hops(0, ref.frames).reshape(-1)[:ref.n_out].astype(np.float32)
    assert ref.n_out % HOP == HOP - 1 and lc.check_hops(y, ref, lc.TOL_FFT, lc.floor_of("imdct", ref)) < 0.1
    bad = y.copy()
    bad[-1] += np.float32(1e-2)
    with pytest.raises(lc.LongClipFailure) as e:
        lc.check_hops(bad, ref, lc.TOL_FFT, lc.floor_of("imdct", ref))
    assert (e.value.what, e.value.frame) == ("bound", ref.frames - 1)


def test_the_loosened_istft_bound_would_be_seen():
    """The mutation check of DESIGN 4.  run_istft admits k_istft_ft16 while W pitch 8 < 2^31; the kernel reads element (row, t) of the clip's
    spectrum at the 32-bit byte offset row pitch 8 + 8 t (v_up / v_down + the sweep's row offset + t_bytes, all `int`).  With the condition
    loosened to <= 2^31 + 4096 * 8 a compact spectrum of 131074 frames is admitted; its row 2047 passes 2^31 - 1 at frame 126978 and the signed
    offset wraps: that row is read from somewhere else, or as zero, from that frame on.  The loosened build never runs; here the same thing is
    done to a small spectrum -- W = 256, pitch 32, a limit twelve elements short of the array -- and the hop checker must refuse the samples at
    the first hop the first wrapped frame reaches (frame t lands in hops t - 1 and t at hop W / 2)."""
    rows, frames = 2048, 131074
    assert rows * frames * 8 <= (1 << 31) + 4096 * 8 < rows * (frames + 1) * 8                      # the loosened condition admits exactly this much
    assert ((1 << 31) - (rows - 1) * frames * 8 + 7) // 8 == 126978 and (rows - 2) * frames * 8 + 8 * frames < 1 << 31   # row 2047 alone, from frame 126978
    p = lc.period_block(HOP)
    w = orc.hamming_periodic(W)
    n = HOP * 31   # T = 32 frames
    spec = orc.stft(lc.periodic_clip(p, n).astype(np.float64), w, HOP)
    pitch = 32
    limit = W * pitch * 8 - 8 * 12
    assert spec.shape == (W, pitch) and (W - 1) * pitch * 8 + 8 * (pitch - 1) >= limit > (W - 1) * pitch * 8   # (only the last row wraps)
    first_wrapped = (limit - (W - 1) * pitch * 8) // 8
    assert first_wrapped == 20
    hurt = spec.copy()
    hurt[W - 1, first_wrapped:] = 0
    ref = lc.periodic_reference("istft", p, n, w=w, hop=HOP)
    y = orc.istft(hurt, w, HOP).astype(np.float32)
    with pytest.raises(lc.LongClipFailure) as e:
        lc.check_hops(y, ref, lc.TOL_FFT, lc.floor_of("istft", ref))
    # frame t lands in the hops t - 1 and t of the output (W = 2 H)
    assert (e.value.what, e.value.frame) == ("bound", first_wrapped - 1)


# ------------------------------------------------------------------------------------------------------------ the bounds table
@pytest.mark.parametrize("name", lc.BOUND_NAMES)
def test_a_bound_brackets_its_condition(name):
    b = lc.bound(name)
    cond, on_route = b["cond"], b["on_route"]
    assert b["n_below"] < b["n_above"]
    assert on_route(b["n_below"]) and on_route(b["n_above"])
    assert cond(b["n_below"]) and not cond(b["n_above"])
    between = [n for n in range(b["n_below"] + 1, b["n_above"]) if on_route(n)]
    assert not between, between[:3]
    # on the route the condition changes once: it holds well below and fails well above
    below = [n for n in range(b["n_below"] - 70000, b["n_below"]) if on_route(n)]
    above = [n for n in range(b["n_above"], b["n_above"] + 70000) if on_route(n)]
    assert below and above and all(cond(n) for n in below) and not any(cond(n) for n in above)
    assert b["above"] == "refused" or b["above"].startswith("k_")
    assert ":" in b["source"] and b["kernel_below"].startswith("k_") and b["kind"] in lc.KINDS


def test_the_bounds_are_where_the_issue_puts_them():
    assert (lc.bound("stft_magnitude_2048")["n_below"], lc.bound("stft_magnitude_2048")["n_above"]) == ((1 << 29) - 1, 1 << 29)
    b = lc.bound("stft_one_sided_2048_carry")
    assert lc.frames_of("stft", b["n_below"], w=np.zeros(2048), hop=2048) == (1 << 18) - 1 and lc.frames_of("stft", b["n_above"], w=np.zeros(2048), hop=2048) == (1 << 18) + 1
    b = lc.bound("istft_2048")   # 131072 frames: 51 minutes at 44.1 kHz
    assert lc.frames_of("stft", b["n_below"], w=np.zeros(2048), hop=1024) == 131071 and lc.frames_of("stft", b["n_above"], w=np.zeros(2048), hop=1024) == 131072
    b = lc.bound("istft_one_sided_2048_padded")
    assert lc.frames_of("stft", b["n_below"], w=np.zeros(2048), hop=1024) == 131056 and lc.frames_of("stft", b["n_above"], w=np.zeros(2048), hop=1024) == 131057
    assert (lc.bound("mdct_2048")["n_below"], lc.bound("mdct_2048")["n_above"]) == ((1 << 28) - 4, 1 << 28)
    assert (lc.bound("mel_2048")["n_below"], lc.bound("mel_2048")["n_above"]) == ((1 << 29) - 2, 1 << 29)
    assert (lc.bound("cqt")["n_below"], lc.bound("center_2048")["n_above"]) == ((1 << 29) - 1, 1 << 28)


# ------------------------------------------------------------------------------------------------------------ the running half on host memory
class HostBuffer:
    """DeviceBuffer's interface (the part long_clips uses) over host memory: the running half without a GPU."""
    live = {}

    def __init__(self, shape, dtype, device=0, _ptr_from_pool=None):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        if _ptr_from_pool is not None:
            self.ptr = _ptr_from_pool
            return
        mem = np.zeros(max(self.nbytes, 1), np.uint8)
        self.ptr = ctypes.c_void_p(mem.ctypes.data)
        HostBuffer.live[self.ptr.value] = mem

    @classmethod
    def from_host(cls, array, device=0):
        array = np.ascontiguousarray(array)
        buf = cls(array.shape, array.dtype)
        ctypes.memmove(buf.ptr.value, array.ctypes.data, array.nbytes)
        return buf

    def copy_from(self, other, nbytes=None, dst_offset=0, src_offset=0):
        nbytes = other.nbytes if nbytes is None else nbytes
        assert 0 <= dst_offset and dst_offset + nbytes <= self.nbytes and 0 <= src_offset and src_offset + nbytes <= other.nbytes
        assert self.ptr.value != other.ptr.value or dst_offset >= src_offset + nbytes or src_offset >= dst_offset + nbytes, "overlapping copy"
        ctypes.memmove(self.ptr.value + dst_offset, other.ptr.value + src_offset, nbytes)
        return self

    def download(self, first=0, count=None):
        count = self.shape[0] - first if count is None else count
        assert first >= 0 and count >= 0 and first + count <= self.shape[0]
        out = np.empty((count,) + self.shape[1:], self.dtype)
        row = self.nbytes // max(self.shape[0], 1)
        ctypes.memmove(out.ctypes.data, self.ptr.value + first * row, out.nbytes)
        return out

    def free(self):
        if self.ptr.value:
            del HostBuffer.live[self.ptr.value]
            self.ptr = ctypes.c_void_p()


class HostZafx:
    DeviceBuffer = HostBuffer


@pytest.fixture
def small_blocks(monkeypatch):
    monkeypatch.setattr(lc, "BLOCK_BYTES", 4096)   # (so that the doubling copies run at these sizes)
    yield
    assert not HostBuffer.live, "a buffer was not freed"


@pytest.mark.parametrize("n", [1, 895, 896, 897, 100003])
@pytest.mark.parametrize("dtype,channels", [(np.float32, 1), (np.int16, 1), (np.float32, 2)])
def test_device_clip_is_the_periodic_clip(small_blocks, dtype, channels, n):
    p = lc.period_block(128, dtype=dtype, channels=channels)
    d = lc.device_clip(HostZafx, p, n)
    assert d.shape == (n,) + p.shape[1:] and d.dtype == p.dtype
    assert np.array_equal(d.download(), lc.periodic_clip(p, n))
    d.free()


def test_device_ragged_lays_the_clips_on_slots(small_blocks):
    p = lc.period_block(128)
    a, c = np.arange(5, dtype=np.float32), np.arange(70, dtype=np.float32) + 100
    d, offsets, lengths = lc.device_ragged(HostZafx, [a, (p, 5000), c])
    assert offsets.tolist() == [0, 32, 32 + 5024] and lengths.tolist() == [5, 5000, 70] and d.shape == (32 + 5024 + 96,)
    want = np.zeros(d.shape, np.float32)
    want[:5], want[32:5032], want[5056:5126] = a, lc.periodic_clip(p, 5000), c
    assert np.array_equal(d.download(), want)
    assert np.array_equal(lc.download_block(HostZafx, d, (10, 7), 5056), c.reshape(10, 7))
    with pytest.raises(ValueError):
        lc.download_block(HostZafx, d, (97,), 5056)
    d.free()
    s = lc.period_block(128, channels=2)
    d, offsets, lengths = lc.device_ragged(HostZafx, [s[:3], (s, 1000)])
    assert d.shape == (32 + 1024, 2) and np.array_equal(d.download()[32:1032], lc.periodic_clip(s, 1000)) and not d.download()[3:32].any()
    d.free()


def test_the_walkers_compare_every_element(small_blocks, spectrum):
    ref, out = spectrum
    rows, pitch = out.shape
    d = lc.device_filled(HostZafx, (1, rows, pitch), np.complex64)
    lc.assert_untouched(HostZafx, d, chunk_bytes=1 << 12)
    assert (d.download().view(np.uint32) == arena.FILL32).all()
    with pytest.raises(lc.LongClipFailure) as e:
        lc.walk_frames(HostZafx, d, rows, pitch, ref, lc.TOL_FFT, lc.floor_of("stft", ref), chunk_bytes=1 << 14)
    assert (e.value.what, e.value.frame, e.value.row) == ("fill", 0, 0)
    ctypes.memmove(d.ptr.value, out.ctypes.data, out.nbytes)
    with pytest.raises(lc.LongClipFailure) as e:
        lc.assert_untouched(HostZafx, d, chunk_bytes=1 << 12)
    assert (e.value.what, e.value.row) == ("untouched", 0)
    assert lc.walk_frames(HostZafx, d, rows, pitch, ref, lc.TOL_FFT, lc.floor_of("stft", ref), chunk_bytes=1 << 14) < 0.1
    # rows that share a bound: the lower half alone
    half = lc.PeriodicRef(ref.small[:100], ref.idx, ref.first, ref.last, ref.q)
    assert lc.walk_frames(HostZafx, d, rows, pitch, half, lc.TOL_FFT, lc.floor_of("stft", half), chunk_bytes=1 << 14, part=(0, 100)) < 0.1
    bad = out.copy()
    bad[255, 300] += 1
    ctypes.memmove(d.ptr.value, bad.ctypes.data, bad.nbytes)
    with pytest.raises(lc.LongClipFailure) as e:
        lc.walk_frames(HostZafx, d, rows, pitch, ref, lc.TOL_FFT, lc.floor_of("stft", ref), chunk_bytes=1 << 14)
    assert (e.value.what, e.value.frame) == ("bound", 300)
    d.free()
    # samples
    hops = lc.periodic_reference("imdct", lc.period_block(HOP), N, w=orc.kbd_window(W))
    y = hops.hops(0, hops.frames).reshape(-1)[:hops.n_out].astype(np.float32)
    d = lc.device_filled(HostZafx, (1, hops.n_out), np.float32)
    ctypes.memmove(d.ptr.value, y.ctypes.data, y.nbytes)
    assert lc.walk_hops(HostZafx, d, hops.n_out, hops, lc.TOL_FFT, lc.floor_of("imdct", hops), chunk_bytes=1 << 12) < 0.1
    y[-1] += 1
    ctypes.memmove(d.ptr.value, y.ctypes.data, y.nbytes)
    with pytest.raises(lc.LongClipFailure) as e:
        lc.walk_hops(HostZafx, d, hops.n_out, hops, lc.TOL_FFT, lc.floor_of("imdct", hops), chunk_bytes=1 << 12)
    assert (e.value.what, e.value.frame) == ("bound", hops.frames - 1)
    d.free()
