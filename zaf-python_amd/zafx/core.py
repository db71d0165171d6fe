"""Plans, device buffers and the batched / drop-in transform functions.

Layering: Python host code -> ctypes -> libzafx.so (C-ABI, include/zafx.h)
-> hand-written HIP kernels.  No PyTorch, no CPU fallback.
"""
import collections
import ctypes
import threading
import weakref

import numpy as np

from . import _lib
from . import constants
from ._lib import ZafxError

_LAYOUTS = {"FT": _lib.LAYOUT_FT, "TF": _lib.LAYOUT_TF, _lib.LAYOUT_FT: _lib.LAYOUT_FT, _lib.LAYOUT_TF: _lib.LAYOUT_TF}


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _i64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _as_int64(values, name):
    a = np.asarray(values)
    if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"{name} must be a 1-D sequence of integers")
    return np.ascontiguousarray(a, dtype=np.int64)


def _as_lengths(values, name="lengths"):
    a = _as_int64(values, name)
    if a.size and int(a.min()) < 0:
        raise ValueError(f"{name} must not be negative")
    return a


# ======================================================================================
# device memory
# ======================================================================================
class _Pinned:
    """Owner of one page-locked host allocation (zafx_host_alloc); freed when the last array view dies."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        _lib.check(_lib.load().zafx_host_alloc(ctypes.byref(p), int(nbytes)), "zafx_host_alloc")
        self.ptr, self.nbytes = p, int(nbytes)

    def __del__(self):
        try:
            if self.ptr and self.ptr.value:
                _lib.load().zafx_host_free(self.ptr)
                self.ptr = ctypes.c_void_p()
        except Exception:
            pass


def pinned_empty(shape, dtype):
    """np.empty in page-locked host memory: transfers at the PCIe rate (~56 GB/s) instead of ~25 GB/s pageable."""
    dtype = np.dtype(dtype)
    shape = tuple(int(s) for s in np.atleast_1d(shape))
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    if nbytes == 0:
        return np.empty(shape, dtype)
    owner = _Pinned(nbytes)
    raw = (ctypes.c_uint8 * nbytes).from_address(owner.ptr.value)
    arr = np.frombuffer(raw, dtype=dtype).reshape(shape)
    _PINNED_OWNERS[id(raw)] = owner   # keep the allocation alive as long as `raw` (the array's base) lives
    weakref.finalize(raw, _PINNED_OWNERS.pop, id(raw), None)
    return arr


_PINNED_OWNERS = {}


class DeviceBuffer:
    """A typed, shaped allocation in one GPU's HBM (owned by this object)."""

    def __init__(self, shape, dtype, device=0, _ptr_from_pool=None):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.device = int(device)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        if _ptr_from_pool is not None:
            self.ptr = _ptr_from_pool
            return
        p = ctypes.c_void_p()
        rc = _lib.load().zafx_alloc(self.device, ctypes.byref(p), self.nbytes)
        if rc == _lib.ERROR_OUT_OF_MEMORY and DeviceBuffer._pool_bytes[0] > 0:
            # out of device memory with allocations parked in the pool: give back those of THIS device, retry once
            # (any other error -- a bad device index, say -- leaves the pool alone)
            DeviceBuffer.drain_pool(self.device)
            rc = _lib.load().zafx_alloc(self.device, ctypes.byref(p), self.nbytes)
        _lib.check(rc, "zafx_alloc")
        self.ptr = p

    # Allocation pool of the host-buffer entry points: a drop-in call on one 10 s clip spends more time in
    # hipMalloc / hipFree (which synchronises the device) than in its kernel, so run_host recycles allocations
    # of the exact size it needs (repeated calls have repeated sizes), up to _POOL_CAP bytes per process.
    _pool, _pool_bytes, _pool_lock = {}, [0], threading.Lock()
    _POOL_CAP = 4 << 30

    @classmethod
    def pooled(cls, shape, dtype, device=0):
        probe_bytes = int(np.prod([int(s) for s in np.atleast_1d(shape)], dtype=np.int64)) * np.dtype(dtype).itemsize
        with cls._pool_lock:
            key = (int(device), probe_bytes)
            free = cls._pool.get(key)
            ptr = free.pop() if free else None
            if ptr is not None:
                cls._pool_bytes[0] -= probe_bytes
            if free is not None and not free:
                del cls._pool[key]   # (an empty size class must not sit at the head of the eviction order, see release)
        return cls(shape, dtype, device, _ptr_from_pool=ptr) if ptr is not None else cls(shape, dtype, device)

    def release(self):
        """Return the allocation to the pool.  The pool is bounded (_POOL_CAP bytes): the oldest parked allocations are
        freed to make room, so a workload of ever-changing clip lengths cannot pin device memory with sizes it never reuses."""
        if getattr(self, "ptr", None) is None or not self.ptr.value:
            return
        if self.nbytes == 0 or self.nbytes > self._POOL_CAP:
            self.free()
            return
        evicted = []
        with self._pool_lock:
            while self._pool_bytes[0] + self.nbytes > self._POOL_CAP and self._pool:
                key = next(iter(self._pool))            # dicts keep insertion order: the size class parked first
                ptrs = self._pool[key]
                if not ptrs:                            # (never left behind by pooled(); kept as a guard)
                    del self._pool[key]
                    continue
                evicted.append((key[0], ptrs.pop(0)))
                self._pool_bytes[0] -= key[1]
                if not ptrs:
                    del self._pool[key]
            self._pool.setdefault((self.device, self.nbytes), []).append(self.ptr)
            self._pool_bytes[0] += self.nbytes
        self.ptr = ctypes.c_void_p()
        for device, ptr in evicted:
            _lib.load().zafx_free(device, ptr)

    @classmethod
    def drain_pool(cls, device=None):
        """Free the parked allocations (of one device, or of all)."""
        with cls._pool_lock:
            items = {k: v for k, v in cls._pool.items() if device is None or k[0] == int(device)}
            for k, ptrs in items.items():
                del cls._pool[k]
                cls._pool_bytes[0] -= k[1] * len(ptrs)
        for (dev, _), ptrs in items.items():
            for p in ptrs:
                _lib.load().zafx_free(dev, p)

    @classmethod
    def from_host(cls, array, device=0):
        array = np.ascontiguousarray(array)
        buf = cls(array.shape, array.dtype, device)
        buf.upload(array)
        return buf

    def upload(self, array):
        array = np.ascontiguousarray(array, dtype=self.dtype)
        if array.nbytes != self.nbytes:
            raise ValueError("upload size mismatch")
        if self.nbytes:
            _lib.check(_lib.load().zafx_h2d(self.device, self.ptr, _ptr(array), self.nbytes), "zafx_h2d")
        return self

    def download(self, first=0, count=None, out=None):
        """Copy to host; `first`/`count` select a range along axis 0.  `out`: destination array (e.g. from
        pinned_empty, reused across calls -- pinning costs ~0.2 ms/MB, so it only pays for a buffer that lives on)."""
        count = self.shape[0] - first if count is None else count
        if first < 0 or count < 0 or first + count > self.shape[0]:
            raise ValueError("download range out of bounds")
        shape = (count,) + self.shape[1:]
        if out is None:
            out = np.empty(shape, dtype=self.dtype)
        elif out.shape != shape or out.dtype != self.dtype or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous array of the downloaded shape and dtype")
        if out.nbytes:
            row = self.nbytes // max(self.shape[0], 1)
            src = ctypes.c_void_p(self.ptr.value + first * row)
            _lib.check(_lib.load().zafx_d2h(self.device, _ptr(out), src, out.nbytes), "zafx_d2h")
        return out

    def fill_zero(self):
        if self.nbytes:
            _lib.check(_lib.load().zafx_memset(self.device, self.ptr, 0, self.nbytes), "zafx_memset")
        return self

    def copy_from(self, other, nbytes=None, dst_offset=0, src_offset=0):
        """Device-to-device copy of `nbytes` (default: all of `other`); returns when the copy is done (zafx_d2d), so a plan launched next
        sees the bytes and cannot have its result overwritten by them."""
        nbytes = other.nbytes if nbytes is None else nbytes
        dst = ctypes.c_void_p(self.ptr.value + dst_offset)
        src = ctypes.c_void_p(other.ptr.value + src_offset)
        _lib.check(_lib.load().zafx_d2d(self.device, dst, src, nbytes), "zafx_d2d")
        return self

    @classmethod
    def placed(cls, shape, dtype, probe, candidates=4, device=0, init=None):
        """The fastest of `candidates` allocations of this shape: -> (buffer, [probe times]).

        Where a large allocation lands in physical memory changes the rate of the kernels that walk it with a row stride (the
        (W, T) spectra of the reference layout): the same STFT runs in 1.50 ms into one 7 GB allocation and in 1.70 ms into
        another made by the same process (profiles/r02_notes.md).  The address is not the caller's to choose, so a long-lived
        buffer is picked by trial: all candidates are allocated (held at once -- freed ones would come straight back), `init(buffer)`
        fills each if the probe reads it, `probe(buffer)` returns a time, the best one stays, the others are freed."""
        bufs = [cls(shape, dtype, device) for _ in range(max(int(candidates), 1))]
        times = []
        for k, b in enumerate(bufs):
            if init is not None:
                init(b)
            if k == 0 and len(bufs) > 1:
                probe(b)   # (not counted: the first probe also carries the clock ramp)
            times.append(float(probe(b)))
        best = min(range(len(bufs)), key=times.__getitem__)
        for i, b in enumerate(bufs):
            if i != best:
                b.free()
        return bufs[best], times

    @classmethod
    def placed_for(cls, plan, d_in, n_clips, n_in, candidates=4, reps=8):
        """The output buffer of `plan` for (n_clips, n_in) as the fastest of `candidates` allocations, picked by the library itself
        (zafx_alloc_placed: every candidate timed with the plan's own kernel on `d_in`): -> (buffer, [ms per launch of each candidate]).
        The C-ABI twin of `placed` -- what a caller without this Python layer uses."""
        shape, dtype = plan.out_shape(n_clips, n_in), plan.out_dtype
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        p = ctypes.c_void_p()
        times = (ctypes.c_float * int(candidates))()
        _lib.check(_lib.load().zafx_alloc_placed(plan.handle, ctypes.byref(p), nbytes, d_in.ptr, int(n_clips), int(n_in), int(candidates), int(reps), times),
                   "zafx_alloc_placed")
        return cls(shape, dtype, plan.device, _ptr_from_pool=p), [float(t) for t in times]

    def free(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            _lib.load().zafx_free(self.device, self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ======================================================================================
# plans
# ======================================================================================
# `onesided` of the STFT / ISTFT entry points: False / True, or "magnitude" / "power" (STFT only: |X| or |X|^2 of
# rows 0..W/2 as real arrays -- the spectrogram of the reference's examples, zaf.py:83)
_SPECTRA = {False: _lib.SPECTRUM_TWO_SIDED, True: _lib.SPECTRUM_ONE_SIDED, "magnitude": _lib.SPECTRUM_MAGNITUDE,
            "power": _lib.SPECTRUM_POWER}


def _as_row_align(row_align, layout):
    a = int(row_align or 0)
    if a < 0 or a > 1024 or a & (a - 1):
        raise ValueError("row_align must be 0 or a power of two <= 1024")
    if a > 1 and _LAYOUTS[layout] != _lib.LAYOUT_FT:
        raise ValueError('row_align applies to layout "FT" only')
    return a


def _spectrum_of(onesided):
    try:
        return _SPECTRA[onesided]
    except (KeyError, TypeError):
        raise ValueError('onesided must be False, True, "magnitude" or "power"') from None


def _rows_with_pitch(a, pitch):
    """a: (B, F, T).  When `a` is a view of rows that lie `pitch` elements apart inside one buffer -- clip after clip, as the (B, F, pitch)
    array of a row_align plan does -- return that (B, F, pitch) array over the same memory, else None.  (The padding behind the last
    row must belong to the buffer too: checked against the bounds of the array that owns the memory.)"""
    isz = a.dtype.itemsize
    b, f, t = a.shape
    if t > pitch or a.strides != (f * pitch * isz, pitch * isz, isz) or not a.size:
        return None
    owner = a
    while isinstance(owner.base, np.ndarray):
        owner = owner.base
    try:
        from numpy.lib.array_utils import byte_bounds
    except ImportError:   # NumPy < 2
        byte_bounds = np.byte_bounds
    lo, hi = byte_bounds(owner)
    start = a.__array_interface__["data"][0]
    if start < lo or start + b * f * pitch * isz > hi:
        return None
    return np.lib.stride_tricks.as_strided(a, shape=(b, f, pitch), strides=(f * pitch * isz, pitch * isz, isz), writeable=False)


def _line_elements(dtype):
    """Elements of one 128-byte line."""
    return 128 // np.dtype(dtype).itemsize


class _MaskedForm(collections.namedtuple("_MaskedForm", (
        "suffix mask_dtype tf_only count_name count_range unit_bytes stems_out per_clip_bound units masks shape_call for_what "
        "equal_sizes_need_tf ragged_sizes_need_tf mask_shape out_shape as_masks batch_count ragged_count_first ragged_count batch_words"))):
    """What the four kinds of the mask filter -- real masks, stems, complex masks, interleaved stereo -- differ in on this side of the library
    (zafx_routes.hpp MaskfilterForm and zafx_capi.cpp kMaskedForms hold the other two thirds):
      suffix         of the method, function and entry-point names ("", "_stems", "_complex", "_stereo")
      mask_dtype     of the device's mask array; tf_only: the device reads "TF" masks only ("FT" ones are transposed on the host)
      count_name     the extra argument (None: the kind has none) and count_range, the values the library takes
      unit_bytes     of what a length or a sample offset counts: 4 (samples), 8 (sample frames)
      stems_out      a clip's output is `count` blocks (+ 1 with rest) instead of 1 (+ 1)
      per_clip_bound count -> the clip length from which the range checks step aside and leave the refusal to the library (None: never)
      units, masks, shape_call, for_what: the messages' words
      equal_sizes_need_tf, ragged_sizes_need_tf: the size checks of the Plan methods step aside for a plan in "FT" (kept as they grew:
                     the complex kind both, the stereo kind for ragged batches only, the stems never)
      mask_shape, out_shape: (plan, n_clips, n_in, count) -> the shapes of the equal-length device arrays
      as_masks       the host masks of a *_batch call as an array
      batch_count    the *_batch masks -> count, or the ValueError of masks it cannot be read from
      ragged_count_first / ragged_count: the same for a sequence of masks, asked before / after the masks are looked at one by one
      batch_words    (what a ragged batch of masks is called, what its items are called; the latter a function of the count)."""
    __slots__ = ()

    def mask_blocks(self, count):
        """Masks of T x (W/2 + 1) a clip brings."""
        return count if self.count_name else 1

    def out_blocks(self, count, rest):
        return (count if self.stems_out else 1) + (1 if rest else 0)

    def count_ok(self, count):
        return self.count_name is None or self.count_range[0] <= count <= self.count_range[1]

    def tf_shape(self, count, frames, rows):
        """One clip's masks as the device reads them in "TF"."""
        if self.stems_out:
            return (count, frames, rows)
        return (frames, count, rows) if self.count_name and count == 2 else (frames, rows)

    def ft_axes(self, count):
        """The transposition that takes one clip's "FT" host masks, the reference's order, to tf_shape."""
        if self.stems_out:
            return (0, 2, 1)
        return (2, 0, 1) if self.count_name and count == 2 else (1, 0)

    def host_shape(self, count, frames, rows, ft):
        tf = self.tf_shape(count, frames, rows)
        return tuple(tf[self.ft_axes(count).index(i)] for i in range(len(tf))) if ft else tf


def _stems_of(shape_text):
    def count(n_stems):
        if not 1 <= n_stems <= _lib.MASKFILTER_MAX_STEMS:
            raise ValueError(f"the number of stems, {shape_text}, must be in 1 .. {_lib.MASKFILTER_MAX_STEMS}, got {n_stems}")
        return n_stems
    return count


def _stems_batch_count(m):
    if m.ndim != 4:
        raise ValueError(f"masks must be 4-D, (clips, stems, ...), got shape {m.shape}")
    return _stems_of("masks.shape[1]")(m.shape[1])


def _stereo_mask_channels(ndim, shared_ndim, what):
    """1 for masks of `shared_ndim` dimensions (one mask for both channels), 2 for one more (one per channel); anything else raises."""
    if ndim not in (shared_ndim, shared_ndim + 1):
        raise ValueError(f"{what} must be {shared_ndim}-D (one mask for both channels) or {shared_ndim + 1}-D (one per channel), got {ndim} dimensions")
    return 1 if ndim == shared_ndim else 2


def _stereo_batch_count(m):
    if m.dtype.kind not in "biuf":
        raise ValueError(f"masks must be real numbers, got dtype {m.dtype}")
    return _stereo_mask_channels(m.ndim, 3, "masks")


def _stereo_ragged_count(masks):
    if isinstance(masks, np.ndarray) and masks.dtype != object:
        raise ValueError("a ragged stereo mask batch is a sequence of 2-D or 3-D masks, not one array")
    try:
        masks = list(masks)
    except TypeError:
        raise ValueError("a ragged stereo mask batch is a sequence of 2-D or 3-D masks") from None
    return masks, (_stereo_mask_channels(np.ndim(masks[0]), 2, "mask 0") if masks else 1)


def _as_complex_masks(masks):
    """The masks of the complex mask filter as an array: real or complex numbers (cast to complex64 at the upload); anything else raises."""
    m = np.asarray(masks)
    if m.dtype.kind not in "biufc":
        raise ValueError(f"masks must be real or complex numbers, got dtype {m.dtype}")
    return m


_MASKED_REAL = _MaskedForm(
    "", np.dtype(np.float32), False, None, None, 4, False, None, "samples", "a float32 mask", "mask_shape(n_clips, n_in)", "these clips", False, False,
    lambda p, b, n, c: p.mask_shape(b, n), lambda p, b, n, c: p.out_shape(b, n), np.asarray, None, None, None, ("ragged mask batch", lambda c: "2-D masks"))
_MASKED_STEMS = _MaskedForm(
    "_stems", np.dtype(np.float32), True, "n_stems", (1, _lib.MASKFILTER_MAX_STEMS), 4, True, lambda c: 1 << 28, "samples", "float32 masks",
    "stems_mask_shape(n_clips, n_in, n_stems)", "these clips and stems", False, False,
    lambda p, b, n, c: p.stems_mask_shape(b, n, c), lambda p, b, n, c: p.stems_out_shape(b, n, c), np.asarray, _stems_batch_count, None,
    lambda arrays: _stems_of("masks[0].shape[0]")(arrays[0].shape[0] if arrays else 1), ("ragged stems mask batch", lambda c: "3-D masks, (stems, ...)"))
_MASKED_COMPLEX = _MaskedForm(
    "_complex", np.dtype(np.complex64), True, None, None, 4, False, lambda c: 1 << 27, "samples", "a complex64 mask", "mask_shape(n_clips, n_in)", "these clips",
    True, True, lambda p, b, n, c: p.mask_shape(b, n), lambda p, b, n, c: p.out_shape(b, n), _as_complex_masks, None, None, None,
    ("ragged mask batch", lambda c: "2-D masks"))
_MASKED_STEREO = _MaskedForm(
    "_stereo", np.dtype(np.float32), True, "mask_channels", (1, 2), 8, False, lambda c: 1 << (29 - c), "sample frames", "float32 masks",
    "stereo_mask_shape(n_clips, n_in, mask_channels)", "these clips", False, True,
    lambda p, b, n, c: p.stereo_mask_shape(b, n, c), lambda p, b, n, c: p.stereo_out_shape(b, n), np.asarray, _stereo_batch_count, _stereo_ragged_count, None,
    ("ragged stereo mask batch", lambda c: f"{1 + c}-D masks"))

# the mono PCM form (execute_masked_pcm with one channel): the real kind's shapes, but the device reads "TF" masks only, and clips below 2^28
_MASKED_PCM_MONO = _MASKED_REAL._replace(tf_only=True, per_clip_bound=lambda c: 1 << 28)


def _check_masked_dtypes(form, name, d_in, d_mask, d_out):
    if d_in.dtype != np.float32 or d_mask.dtype != form.mask_dtype or d_out.dtype != np.float32:
        raise ValueError(f"{name} takes float32 {form.units}, {form.masks} and a float32 output buffer")


class Plan:
    """One transform kind bound to one device and one HIP stream (zafx_plan)."""

    _FORWARD = (_lib.STFT, _lib.MDCT, _lib.MEL, _lib.MFCC, _lib.CQT, _lib.CHROMA)   # 2-D (frequency x time) outputs

    def __init__(self, kind, device=0, window_length=0, step_length=0, layout="FT", n_filters=0, n_coefs=0,
                 fft_length=0, n_bins=0, octave_resolution=0, onesided=False, f64=False, row_align=0, transform_type=0, transform_sine=False,
                 with_mel=False):
        self.kind = kind
        self.device = int(device)
        self.layout = _LAYOUTS[layout]
        prm = _lib.ZafxParams()
        prm.struct_size = ctypes.sizeof(_lib.ZafxParams)
        prm.window_length = int(window_length)
        prm.step_length = int(step_length)
        prm.layout = self.layout
        prm.n_filters = int(n_filters)
        prm.n_coefs = int(n_coefs)
        prm.fft_length = int(fft_length)
        prm.n_bins = int(n_bins)
        prm.octave_resolution = int(octave_resolution)
        prm.transform_type = int(transform_type)
        prm.transform_sine = int(bool(transform_sine))
        prm.with_mel = int(bool(with_mel))
        self.spectrum = _spectrum_of(onesided)
        prm.spectrum = self.spectrum
        prm.precision = _lib.PRECISION_F64 if f64 else _lib.PRECISION_F32
        self.f64 = bool(f64)
        self.row_align = _as_row_align(row_align, layout)
        prm.row_align = self.row_align
        self.params = prm
        h = ctypes.c_void_p()
        _lib.check(_lib.load().zafx_plan_create(ctypes.byref(h), self.device, kind, ctypes.byref(prm)), "zafx_plan_create")
        self.handle = h
        self.lock = threading.Lock()

    # ---- constants -----------------------------------------------------------------
    def _set(self, which, array, dtype):
        array = np.ascontiguousarray(array, dtype=dtype)
        _lib.check(_lib.load().zafx_plan_set_constant(self.handle, which, _ptr(array), array.nbytes), "zafx_plan_set_constant")

    def set_window(self, window_function):
        self._set(_lib.CONST_WINDOW, window_function, np.float64 if self.f64 else np.float32)

    def set_mel_filterbank(self, mel_filterbank):
        dense = mel_filterbank.toarray() if hasattr(mel_filterbank, "toarray") else np.asarray(mel_filterbank)
        self._set(_lib.CONST_MEL_FB, dense, np.float64 if self.f64 else np.float32)

    def set_dct(self, dct_rows):
        self._set(_lib.CONST_DCT, dct_rows, np.float64 if self.f64 else np.float32)

    def set_matrix(self, matrix):
        self._set(_lib.CONST_MATRIX, matrix, np.float32)

    def set_cqt_kernel(self, cqt_kernel):
        csr = cqt_kernel.tocsr()
        csr.sort_indices()
        self._set(_lib.CONST_CQT_INDPTR, csr.indptr, np.int32)
        self._set(_lib.CONST_CQT_INDICES, csr.indices, np.int32)
        self._set(_lib.CONST_CQT_VALUES, csr.data, np.complex128 if self.f64 else np.complex64)

    # ---- geometry / execution ----------------------------------------------------------
    def out_dims(self, n_in):
        dims = (ctypes.c_int64 * 2)()
        _lib.check(_lib.load().zafx_plan_out_dims(self.handle, int(n_in), dims), "zafx_plan_out_dims")
        return int(dims[0]), int(dims[1])

    def row_pitch(self, n_in):
        """Elements between consecutive rows of the plan's 2-D array (T rounded up to row_align; T for compact plans)."""
        pitch = ctypes.c_int64()
        _lib.check(_lib.load().zafx_plan_row_pitch(self.handle, int(n_in), ctypes.byref(pitch)), "zafx_plan_row_pitch")
        return int(pitch.value)

    def out_shape(self, n_clips, n_in):
        """Shape of the device array execute() writes; with row_align the last axis of an (F, T) array is the pitch."""
        rows, frames = self.out_dims(n_in)
        if self.kind in self._FORWARD:
            return (n_clips, rows, self.row_pitch(n_in)) if self.layout == _lib.LAYOUT_FT else (n_clips, frames, rows)
        if self.kind == _lib.CENTER:
            return (n_clips, rows, 2)
        if self.kind == _lib.CENTER_SIDES:   # block 0 the center, block 1 the sides
            return (n_clips, 2, rows // 2, 2)
        if self.kind == _lib.MASKFILTER_REST:   # block 0 the filtered clip, block 1 the rest
            return (n_clips, 2, rows // 2)
        return (n_clips, rows)

    def mask_dims(self, n_in):
        """(rows, frames) of one clip's mask under a mask filter plan (zafx_plan_mask_dims): W/2 + 1 and ceil(n_in / H) + 1."""
        dims = (ctypes.c_int64 * 2)()
        _lib.check(_lib.load().zafx_plan_mask_dims(self.handle, int(n_in), dims), "zafx_plan_mask_dims")
        return int(dims[0]), int(dims[1])

    def mask_shape(self, n_clips, n_in):
        """Shape of the float32 device array execute_masked() reads its masks from: (clips, W/2 + 1, row_pitch(n_in)) in "FT" -- the last axis
        is the pitch, the frame count rounded up to row_align -- or (clips, frames, W/2 + 1) in "TF"."""
        rows, frames = self.mask_dims(n_in)
        return (n_clips, rows, self.row_pitch(n_in)) if self.layout == _lib.LAYOUT_FT else (n_clips, frames, rows)

    @property
    def out_dtype(self):
        complex_out = self.kind == _lib.STFT and self.spectrum < _lib.SPECTRUM_MAGNITUDE
        if self.f64:
            return np.dtype(np.complex128) if complex_out else np.dtype(np.float64)
        return np.dtype(np.complex64) if complex_out else np.dtype(np.float32)

    @property
    def in_dtype(self):
        if self.kind == _lib.ISTFT:
            return np.dtype(np.complex128) if self.f64 else np.dtype(np.complex64)
        return np.dtype(np.float64) if self.f64 else np.dtype(np.float32)

    def execute(self, d_in, d_out, n_clips, n_in):
        """Enqueue on the plan's stream (asynchronous); d_in / d_out are DeviceBuffers."""
        _lib.check(_lib.load().zafx_execute(self.handle, d_in.ptr, d_out.ptr, int(n_clips), int(n_in)), "zafx_execute")

    def execute_masked(self, d_in, d_mask, d_out, n_clips, n_in):
        """Enqueue the mask filter on the plan's stream (asynchronous; zafx_execute_masked, mask filter plans only; last_kernel: k_maskfilter):
        d_in (clips, n_in) float32 samples, d_mask float32 of mask_shape(n_clips, n_in), d_out of out_shape(n_clips, n_in).  Buffers of another
        dtype or too small for these clips raise ValueError before anything is enqueued."""
        self._execute_masked(_MASKED_REAL, d_in, d_mask, d_out, n_clips, n_in)

    def _execute_masked(self, form, d_in, d_mask, d_out, n_clips, n_in, count=None):
        """The equal-length entry point of a kind behind _check_masked."""
        n_clips, n_in, tail = int(n_clips), int(n_in), () if count is None else (int(count),)
        self._check_masked(form, d_in, d_mask, d_out, n_clips, n_in, *tail)
        entry = "zafx_execute_masked" + form.suffix
        _lib.check(getattr(_lib.load(), entry)(self.handle, d_in.ptr, d_mask.ptr, d_out.ptr, n_clips, n_in, *tail), entry)

    def _check_masked(self, form, d_in, d_mask, d_out, n_clips, n_in, count=None):
        """The checks of the three buffers of an equal-length call of `form`, before anything is enqueued."""
        name = "execute_masked" + form.suffix
        _check_masked_dtypes(form, name, d_in, d_mask, d_out)
        if n_clips < 0 or n_in < 0:
            raise ValueError("n_clips and n_in must not be negative")
        # (another kind, count or -- where the shapes depend on it -- layout: the library says so)
        if self.kind in (_lib.MASKFILTER, _lib.MASKFILTER_REST) and form.count_ok(count) and not (form.equal_sizes_need_tf and self.layout != _lib.LAYOUT_TF):
            mask_shape, out_shape = form.mask_shape(self, n_clips, n_in, count), form.out_shape(self, n_clips, n_in, count)
            if d_in.nbytes < n_clips * n_in * form.unit_bytes:
                raise ValueError(f"d_in holds fewer than clips x n_in {form.units}")
            if d_mask.nbytes != int(np.prod(mask_shape, dtype=np.int64)) * form.mask_dtype.itemsize:
                raise ValueError(f"d_mask must hold {form.shape_call} = {mask_shape} {form.mask_dtype.name}, got {d_mask.nbytes} bytes")
            if d_out.nbytes < int(np.prod(out_shape, dtype=np.int64)) * 4:
                raise ValueError(f"d_out is smaller than the plan's output for {form.for_what}")

    def stems_mask_shape(self, n_clips, n_in, n_stems):
        """Shape of the float32 device array execute_masked_stems() reads its masks from: (clips, stems, frames, W/2 + 1) compact -- a clip's
        masks back to back, each as a "TF" plan's mask_shape gives it."""
        rows, frames = self.mask_dims(n_in)
        return (int(n_clips), int(n_stems), frames, rows)

    def stems_out_shape(self, n_clips, n_in, n_stems):
        """Shape of execute_masked_stems()'s output: (clips, stems, n_in), or (clips, stems + 1, n_in) under a MASKFILTER_REST plan, whose last
        block of a clip is the rest."""
        return (int(n_clips), int(n_stems) + (1 if self.kind == _lib.MASKFILTER_REST else 0), int(n_in))

    def execute_masked_stems(self, d_in, d_mask, d_out, n_clips, n_in, n_stems):
        """Enqueue the mask filter with n_stems masks per clip on the plan's stream (asynchronous; zafx_execute_masked_stems, mask filter plans of
        layout "TF" only; last_kernel: k_maskfilter_stems): one forward transform per clip, one inverse per stem.  d_in (clips, n_in) float32
        samples, d_mask float32 of stems_mask_shape(n_clips, n_in, n_stems), d_out of stems_out_shape(n_clips, n_in, n_stems).  Stem s of a clip
        has the bits execute_masked gives that clip with mask s alone.  Buffers of another dtype or of the wrong size raise ValueError before
        anything is enqueued."""
        self._execute_masked(_MASKED_STEMS, d_in, d_mask, d_out, n_clips, n_in, n_stems)

    def execute_masked_complex(self, d_in, d_mask, d_out, n_clips, n_in):
        """Enqueue the mask filter under complex masks on the plan's stream (asynchronous; zafx_execute_masked_complex, mask filter plans of
        layout "TF" only; last_kernel: k_maskfilter_complex): y = istft(concat(M, conj(M[-2:0:-1])) * stft(x))[0:n_in].  d_in (clips, n_in)
        float32 samples, d_mask complex64 of mask_shape(n_clips, n_in) = (clips, frames, W/2 + 1), d_out of out_shape(n_clips, n_in).  The
        imaginary parts of mask rows 0 and W/2 have no effect.  Buffers of another dtype or too small for these clips raise ValueError before
        anything is enqueued."""
        self._execute_masked(_MASKED_COMPLEX, d_in, d_mask, d_out, n_clips, n_in)

    def stereo_mask_shape(self, n_clips, n_in, mask_channels):
        """Shape of the float32 device array execute_masked_stereo() reads its masks from, compact: (clips, frames, W/2 + 1) for one mask for
        both channels (mask_channels 1), (clips, frames, 2, W/2 + 1) for one per channel (2) -- a frame's L row directly in front of its R row."""
        rows, frames = self.mask_dims(n_in)
        return (int(n_clips), frames, rows) if int(mask_channels) == 1 else (int(n_clips), frames, int(mask_channels), rows)

    def stereo_out_shape(self, n_clips, n_in):
        """Shape of execute_masked_stereo()'s output: (clips, n_in, 2), or (clips, 2, n_in, 2) under a MASKFILTER_REST plan, whose block 1 of a
        clip is the rest (the layout of a CENTER_SIDES plan)."""
        return (int(n_clips), 2, int(n_in), 2) if self.kind == _lib.MASKFILTER_REST else (int(n_clips), int(n_in), 2)

    def execute_masked_stereo(self, d_in, d_mask, d_out, n_clips, n_in, mask_channels):
        """Enqueue the mask filter of interleaved stereo clips on the plan's stream (asynchronous; zafx_execute_masked_stereo, mask filter plans
        of layout "TF" only; last_kernel: k_maskfilter_stereo): d_in (clips, n_in, 2) float32 sample frames, d_mask float32 of
        stereo_mask_shape(n_clips, n_in, mask_channels), d_out of stereo_out_shape(n_clips, n_in).  mask_channels 1: one mask for both
        channels; 2: one per channel.  Buffers of another dtype or of the wrong size raise ValueError before anything is enqueued."""
        self._execute_masked(_MASKED_STEREO, d_in, d_mask, d_out, n_clips, n_in, mask_channels)

    def stereo_ragged_layout(self, lengths, mask_channels):
        """Placement of a ragged stereo mask-filter batch (zafx_plan_stereo_ragged_layout, mask filter plans of layout "TF") for clips of `lengths`
        sample frames: -> (mask_offsets, out_offsets), int64 of len(lengths) + 1.  Clip i's masks, (T_i, mask_channels, W/2 + 1), start at
        float32 element mask_offsets[i] -- mask_channels x what mask_ragged_layout gives --, its output block, N_i sample frames or with rest
        two such, starts at SAMPLE FRAME out_offsets[i]; the last entries are the totals."""
        return self._masked_ragged_layout(_MASKED_STEREO, lengths, mask_channels)

    def _masked_ragged_layout(self, form, lengths, count):
        lengths = _as_lengths(lengths)
        mask_offs, out_offs = np.zeros(len(lengths) + 1, np.int64), np.zeros(len(lengths) + 1, np.int64)
        entry = f"zafx_plan{form.suffix}_ragged_layout"
        _lib.check(getattr(_lib.load(), entry)(self.handle, _i64p(lengths), len(lengths), int(count), _i64p(mask_offs), _i64p(out_offs)), entry)
        return mask_offs, out_offs

    def execute_masked_stereo_ragged(self, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets, mask_channels):
        """Enqueue the mask filter of stereo clips of different lengths as one launch on the plan's stream (asynchronous;
        zafx_execute_masked_stereo_ragged, mask filter plans of layout "TF" only; last_kernel: k_maskfilter_stereo_ragged).  in_offsets,
        lengths and out_offsets count sample frames (L, R), as in execute_center_ragged: clip i is lengths[i] sample frames at sample frame
        in_offsets[i] of d_in, its result goes to sample frame out_offsets[i] of d_out and, for a plan with rest, the rest directly behind.
        mask_offsets counts float32 elements: clip i's masks, (T_i, mask_channels, W/2 + 1) compact, start at element mask_offsets[i] of d_mask
        (stereo_ragged_layout gives the compact placement; its totals may stay on).  Clip i's block has the bits execute_masked_stereo gives
        that clip and its masks alone.  Output blocks that overlap are not detected."""
        self._execute_masked_ragged(_MASKED_STEREO, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets, mask_channels)

    def ragged_layout(self, lengths):
        """Placement of a ragged batch's results (zafx_plan_ragged_layout) for clips of `lengths` samples: -> (out_offsets, frames, pitch), int64
        arrays.  Clip i's block of the output array starts at element out_offsets[i] (out_offsets[-1]: elements in all) and holds F rows of
        pitch[i] elements ("FT"; frames[i] of them are the clip's) or frames[i] x F compact ("TF")."""
        lengths = _as_lengths(lengths)
        offs = self._ragged_offsets(lengths)
        frames = np.array([self.out_dims(n)[1] for n in lengths.tolist()], np.int64)
        pitch = np.array([self.row_pitch(n) for n in lengths.tolist()], np.int64)
        return offs, frames, pitch

    def _ragged_offsets(self, lengths):
        offs = np.zeros(len(lengths) + 1, np.int64)
        _lib.check(_lib.load().zafx_plan_ragged_layout(self.handle, _i64p(lengths), len(lengths), _i64p(offs)), "zafx_plan_ragged_layout")
        return offs

    def execute_ragged(self, d_in, in_offsets, lengths, d_out):
        """Enqueue one ragged batch on the plan's stream (asynchronous; zafx_execute_ragged): clip i is lengths[i] samples at element in_offsets[i]
        of d_in, its result goes to the block ragged_layout(lengths) assigns in d_out.  Float32 plans in the "FT" layout whose rows are whole
        128-byte lines run as one launch where the library has the kernel (last_kernel: k_stft_ft16_ragged / k_mel2_ragged); the others as one
        execute per clip ("per-clip <kernel>").  Float64 plans at window 2048 ("FT", rows of whole lines, d_in on 16 bytes): one launch of
        k_stft_ft8_f64_ragged (complex kinds), k_mdct_ft16_f64_ragged or k_mel_ft8_f64_ragged, at any offsets and lengths."""
        lengths, in_offsets = _as_lengths(lengths), _as_lengths(in_offsets, "in_offsets")
        if len(in_offsets) != len(lengths):
            raise ValueError("in_offsets and lengths must have one entry per clip")
        if d_in.dtype != self.in_dtype or d_out.dtype != self.out_dtype:
            raise ValueError(f"execute_ragged takes {self.in_dtype} samples and a {self.out_dtype} output buffer")
        if len(lengths) and int((in_offsets + lengths).max()) > d_in.nbytes // d_in.dtype.itemsize:
            raise ValueError("a clip reaches past the end of d_in")
        if int(self._ragged_offsets(lengths)[-1]) * self.out_dtype.itemsize > d_out.nbytes:
            raise ValueError("d_out is smaller than the ragged batch's output (ragged_layout)")
        _lib.check(_lib.load().zafx_execute_ragged(self.handle, d_in.ptr, _i64p(in_offsets), _i64p(lengths), d_out.ptr, len(lengths)),
                   "zafx_execute_ragged")

    def execute_center_ragged(self, d_in, in_offsets, lengths, d_out, out_offsets):
        """Enqueue the center / sides extraction of stereo clips of different lengths as one launch on the plan's stream (asynchronous;
        zafx_execute_center_ragged, center plans only; last_kernel: k_center_ragged).  Offsets and lengths count sample frames (L, R): clip i
        is lengths[i] sample frames at sample frame in_offsets[i] of d_in, its center goes to sample frame out_offsets[i] of d_out and, for a
        plan with sides, its sides directly behind.  Output blocks that overlap are not detected."""
        in_offsets, lengths, out_offsets = _as_int64(in_offsets, "in_offsets"), _as_int64(lengths, "lengths"), _as_int64(out_offsets, "out_offsets")
        if not len(in_offsets) == len(lengths) == len(out_offsets):
            raise ValueError("in_offsets, lengths and out_offsets must have one entry per clip")
        if d_in.dtype != np.float32 or d_out.dtype != np.float32:
            raise ValueError("execute_center_ragged takes float32 sample frames and a float32 output buffer")
        blocks = 2 if self.kind == _lib.CENTER_SIDES else 1
        if len(lengths) and min(int(lengths.min()), int(in_offsets.min()), int(out_offsets.min())) >= 0:   # (negative values: the library says so)
            if int((in_offsets + lengths).max()) * 8 > d_in.nbytes:
                raise ValueError("a clip reaches past the end of d_in")
            if int((out_offsets + blocks * lengths).max()) * 8 > d_out.nbytes:
                raise ValueError("a clip's result reaches past the end of d_out")
        _lib.check(_lib.load().zafx_execute_center_ragged(self.handle, d_in.ptr, _i64p(in_offsets), _i64p(lengths), d_out.ptr, _i64p(out_offsets),
                                                          len(lengths)), "zafx_execute_center_ragged")

    def mask_ragged_layout(self, lengths):
        """Placement of a ragged mask-filter batch's masks (zafx_plan_mask_ragged_layout) for clips of `lengths` samples: -> mask_offsets, int64
        of len(lengths) + 1.  Clip i's mask -- mask_dims(lengths[i]) rows at row_pitch(lengths[i]) in "FT", frames x rows compact in "TF" --
        starts at element mask_offsets[i] of the mask array, the masks lie back to back and mask_offsets[-1] counts the elements in all: the
        layout ragged_layout gives a one-sided magnitude STFT plan of the same window, layout and row_align."""
        lengths = _as_lengths(lengths)
        offs = np.zeros(len(lengths) + 1, np.int64)
        _lib.check(_lib.load().zafx_plan_mask_ragged_layout(self.handle, _i64p(lengths), len(lengths), _i64p(offs)), "zafx_plan_mask_ragged_layout")
        return offs

    def execute_masked_ragged(self, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets):
        """Enqueue the mask filter of mono clips of different lengths as one launch on the plan's stream (asynchronous;
        zafx_execute_masked_ragged, mask filter plans only; last_kernel: k_maskfilter_ragged).  Offsets and lengths count float32 elements:
        clip i is lengths[i] samples at element in_offsets[i] of d_in, its mask (shape and pitch as in mask_ragged_layout) starts at element
        mask_offsets[i] of d_mask, its filtered samples go to element out_offsets[i] of d_out and, for a plan with rest, the rest directly
        behind.  mask_offsets may carry the total mask_ragged_layout appends.  Output blocks that overlap are not detected."""
        self._execute_masked_ragged(_MASKED_REAL, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets)

    def _execute_masked_ragged(self, form, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets, count=None):
        """The ragged entry point of a kind behind _masked_ragged_args."""
        tail = () if count is None else (int(count),)
        in_offsets, lengths, mask_offsets, out_offsets = self._masked_ragged_args(form, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets, *tail)
        entry = f"zafx_execute_masked{form.suffix}_ragged"
        _lib.check(getattr(_lib.load(), entry)(self.handle, d_in.ptr, _i64p(in_offsets), _i64p(lengths), d_mask.ptr, _i64p(mask_offsets), d_out.ptr, _i64p(out_offsets),
                                               len(lengths), *tail), entry)

    def _masked_ragged_args(self, form, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets, count=None):
        """A ragged call of `form`: the per-clip arrays as int64 without the totals the layout calls append (out_offsets: of the kinds that have
        a layout call giving them), and the checks of the three buffers -> (in_offsets, lengths, mask_offsets, out_offsets).  mask_offsets count
        elements of the form's mask dtype, the other three what the form's lengths count."""
        in_offsets, lengths = _as_int64(in_offsets, "in_offsets"), _as_int64(lengths, "lengths")
        out_offsets, mask_offsets = _as_int64(out_offsets, "out_offsets"), _as_int64(mask_offsets, "mask_offsets")
        if len(mask_offsets) == len(lengths) + 1:
            mask_offsets = np.ascontiguousarray(mask_offsets[:-1])
        if form.count_name and len(out_offsets) == len(lengths) + 1:
            out_offsets = np.ascontiguousarray(out_offsets[:-1])
        if not len(in_offsets) == len(lengths) == len(out_offsets) == len(mask_offsets):
            raise ValueError("in_offsets, lengths, mask_offsets and out_offsets must have one entry per clip")
        _check_masked_dtypes(form, f"execute_masked{form.suffix}_ragged", d_in, d_mask, d_out)
        # (another kind or count, negative values, a clip the library refuses, a plan in "FT" where the form asks here: the library says so)
        ok = self.kind in (_lib.MASKFILTER, _lib.MASKFILTER_REST) and len(lengths) and form.count_ok(count)
        ok = ok and not (form.ragged_sizes_need_tf and self.layout != _lib.LAYOUT_TF)
        if ok and min(int(lengths.min()), int(in_offsets.min()), int(out_offsets.min()), int(mask_offsets.min())) >= 0 and not (
                form.per_clip_bound and int(lengths.max()) >= form.per_clip_bound(count)):
            h = int(self.params.window_length) // 2
            frames = (lengths + h - 1) // h + 1
            if self.layout == _lib.LAYOUT_FT and not form.tf_only:   # the last element the kernel may read: row H, the clip's last frame
                a = max(self.row_align, 1)
                mask_ends = mask_offsets + h * ((frames + a - 1) // a * a) + frames
            else:   # compact "TF" masks back to back
                mask_ends = mask_offsets + form.mask_blocks(count) * frames * (h + 1)
            blocks = form.out_blocks(count, self.kind == _lib.MASKFILTER_REST)
            live = lengths > 0   # (a clip of length 0 is skipped: its masks are never read)
            if int((in_offsets + lengths).max()) * form.unit_bytes > d_in.nbytes:
                raise ValueError("a clip reaches past the end of d_in")
            if live.any() and int(mask_ends[live].max()) * form.mask_dtype.itemsize > d_mask.nbytes:
                raise ValueError(f"a clip's {'masks reach' if form.count_name else 'mask reaches'} past the end of d_mask")
            if int((out_offsets + blocks * lengths).max()) * form.unit_bytes > d_out.nbytes:
                raise ValueError("a clip's result reaches past the end of d_out")
        return in_offsets, lengths, mask_offsets, out_offsets

    def execute_masked_complex_ragged(self, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets):
        """Enqueue the mask filter under complex masks for mono clips of different lengths as one launch on the plan's stream (asynchronous;
        zafx_execute_masked_complex_ragged, mask filter plans of layout "TF" only; last_kernel: k_maskfilter_complex_ragged).  in_offsets,
        lengths and out_offsets count float32 elements as in execute_masked_ragged; mask_offsets counts complex64 elements: clip i's mask,
        (T_i, W/2 + 1) compact, starts at complex element mask_offsets[i] of d_mask (mask_ragged_layout gives the compact placement; its total
        may stay on).  Clip i's block has the bits execute_masked_complex gives that clip and mask alone.  Output blocks that overlap are not
        detected."""
        self._execute_masked_ragged(_MASKED_COMPLEX, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets)

    def _pcm_masked_args(self, name, d_pcm, d_mask, d_out, n_channels, mask_channels):
        """The dtype checks of the PCM mask-filter calls -> (the form whose shapes the call has, its count or None, out_sample_bytes)."""
        if d_pcm.dtype != np.int16:
            raise ValueError(f"{name} takes int16 samples, got {d_pcm.dtype} (no silent cast: int32 and 24-bit material stay with the caller)")
        if d_mask.dtype != np.float32:
            raise ValueError(f"{name} takes float32 masks, got {d_mask.dtype}")
        if d_out.dtype not in (np.int16, np.float32):
            raise ValueError(f"{name} writes int16 or float32 samples, got an output buffer of {d_out.dtype}")
        n_channels, mask_channels = int(n_channels), int(mask_channels)
        form = _MASKED_STEREO if n_channels == 2 else _MASKED_PCM_MONO
        return form, (mask_channels if n_channels == 2 else None), d_out.dtype.itemsize

    def execute_masked_pcm(self, d_pcm, d_mask, d_out, n_clips, n_in, n_channels=1, mask_channels=1):
        """Enqueue the mask filter on 16-bit PCM on the plan's stream (asynchronous; zafx_execute_masked_pcm, mask filter plans of layout "TF"
        only; last_kernel: k_maskfilter_pcm / k_maskfilter_stereo_pcm): d_pcm int16, (clips, n_in) for n_channels 1 and (clips, n_in, 2)
        interleaved for 2; d_mask float32 of mask_shape(n_clips, n_in) (n_channels 1, mask_channels 1) or of
        stereo_mask_shape(n_clips, n_in, mask_channels); d_out of out_shape / stereo_out_shape, int16 or float32 -- the output type is read
        from d_out.dtype.  A sample s enters as s / 32768; a float32 output has the bits of execute_masked / execute_masked_stereo on the
        clip normalised that way, an int16 one is its quantisation (rint, ties to even, saturating, NaN -> 0) and the rest is
        clip(x - y_q) in integers.  Buffers of another dtype or too small for these clips raise ValueError before anything is enqueued."""
        form, count, out_bytes = self._pcm_masked_args("execute_masked_pcm", d_pcm, d_mask, d_out, n_channels, mask_channels)
        n_clips, n_in = int(n_clips), int(n_in)
        if n_clips < 0 or n_in < 0:
            raise ValueError("n_clips and n_in must not be negative")
        # (another kind, channel count or layout: the library says so)
        if self.kind in (_lib.MASKFILTER, _lib.MASKFILTER_REST) and self.layout == _lib.LAYOUT_TF and int(n_channels) in (1, 2) and form.count_ok(count):
            mask_shape, out_shape = form.mask_shape(self, n_clips, n_in, count), form.out_shape(self, n_clips, n_in, count)
            if d_pcm.nbytes < n_clips * n_in * 2 * int(n_channels):
                raise ValueError("d_pcm holds fewer than clips x n_in sample frames")
            if d_mask.nbytes != int(np.prod(mask_shape, dtype=np.int64)) * 4:
                raise ValueError(f"d_mask must hold {form.shape_call} = {mask_shape} float32, got {d_mask.nbytes} bytes")
            if d_out.nbytes < int(np.prod(out_shape, dtype=np.int64)) * out_bytes:
                raise ValueError("d_out is smaller than the plan's output for these clips")
        _lib.check(_lib.load().zafx_execute_masked_pcm(self.handle, d_pcm.ptr, d_mask.ptr, d_out.ptr, n_clips, n_in, int(n_channels), int(mask_channels), out_bytes),
                   "zafx_execute_masked_pcm")

    def execute_masked_pcm_ragged(self, d_pcm, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets, n_channels=1, mask_channels=1):
        """Enqueue the mask filter on 16-bit PCM clips of different lengths as one launch on the plan's stream (asynchronous;
        zafx_execute_masked_pcm_ragged, mask filter plans of layout "TF" only; last_kernel: k_maskfilter_pcm_ragged /
        k_maskfilter_stereo_pcm_ragged).  in_offsets, lengths and out_offsets count sample frames: clip i is lengths[i] sample frames at
        sample frame in_offsets[i] of d_pcm (int16), its result goes to sample frame out_offsets[i] of d_out (int16 or float32, read from
        d_out.dtype) and, for a plan with rest, the rest directly behind.  mask_offsets counts float32 elements, as mask_ragged_layout
        (n_channels 1) or stereo_ragged_layout (2) place them; their totals may stay on.  Clip i's block has the bits execute_masked_pcm
        gives that clip and its masks alone.  Output blocks that overlap are not detected."""
        form, count, out_bytes = self._pcm_masked_args("execute_masked_pcm_ragged", d_pcm, d_mask, d_out, n_channels, mask_channels)
        in_offsets, lengths = _as_int64(in_offsets, "in_offsets"), _as_int64(lengths, "lengths")
        out_offsets, mask_offsets = _as_int64(out_offsets, "out_offsets"), _as_int64(mask_offsets, "mask_offsets")
        if len(mask_offsets) == len(lengths) + 1:
            mask_offsets = np.ascontiguousarray(mask_offsets[:-1])
        if len(out_offsets) == len(lengths) + 1:
            out_offsets = np.ascontiguousarray(out_offsets[:-1])
        if not len(in_offsets) == len(lengths) == len(out_offsets) == len(mask_offsets):
            raise ValueError("in_offsets, lengths, mask_offsets and out_offsets must have one entry per clip")
        # (another kind, channel count or layout, negative values, a clip the library refuses: the library says so)
        ok = self.kind in (_lib.MASKFILTER, _lib.MASKFILTER_REST) and self.layout == _lib.LAYOUT_TF and len(lengths) and int(n_channels) in (1, 2) and form.count_ok(count)
        if ok and min(int(lengths.min()), int(in_offsets.min()), int(out_offsets.min()), int(mask_offsets.min())) >= 0 and int(lengths.max()) < form.per_clip_bound(count):
            h = int(self.params.window_length) // 2
            mask_ends = mask_offsets + form.mask_blocks(count) * ((lengths + h - 1) // h + 1) * (h + 1)
            blocks = 2 if self.kind == _lib.MASKFILTER_REST else 1
            live = lengths > 0   # (a clip of length 0 is skipped: its masks are never read)
            if int((in_offsets + lengths).max()) * 2 * int(n_channels) > d_pcm.nbytes:
                raise ValueError("a clip reaches past the end of d_pcm")
            if live.any() and int(mask_ends[live].max()) * 4 > d_mask.nbytes:
                raise ValueError("a clip's masks reach past the end of d_mask")
            if int((out_offsets + blocks * lengths).max()) * out_bytes * int(n_channels) > d_out.nbytes:
                raise ValueError("a clip's result reaches past the end of d_out")
        _lib.check(_lib.load().zafx_execute_masked_pcm_ragged(self.handle, d_pcm.ptr, _i64p(in_offsets), _i64p(lengths), d_mask.ptr, _i64p(mask_offsets), d_out.ptr,
                                                              _i64p(out_offsets), len(lengths), int(n_channels), int(mask_channels), out_bytes),
                   "zafx_execute_masked_pcm_ragged")

    def stems_ragged_layout(self, lengths, n_stems):
        """Placement of a ragged stems batch (zafx_plan_stems_ragged_layout, mask filter plans of layout "TF") for clips of `lengths` samples
        with n_stems masks each: -> (mask_offsets, out_offsets), int64 of len(lengths) + 1, in float32 elements.  Clip i's masks lie back to
        back as (n_stems, T_i, W/2 + 1) from element mask_offsets[i] -- n_stems x what mask_ragged_layout gives --, its output block,
        (n_stems, N_i) or with rest (n_stems + 1, N_i), starts at element out_offsets[i]; the last entries are the totals."""
        return self._masked_ragged_layout(_MASKED_STEMS, lengths, n_stems)

    def execute_masked_stems_ragged(self, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets, n_stems):
        """Enqueue the mask filter with n_stems masks per clip for mono clips of different lengths as one launch on the plan's stream
        (asynchronous; zafx_execute_masked_stems_ragged, mask filter plans of layout "TF" only; last_kernel: k_maskfilter_stems_ragged).
        Offsets and lengths count float32 elements: clip i is lengths[i] samples at element in_offsets[i] of d_in, its n_stems masks, each
        (T_i, W/2 + 1) compact, lie back to back from element mask_offsets[i] of d_mask, and its block -- (n_stems, N_i), with rest
        (n_stems + 1, N_i) -- starts at element out_offsets[i] of d_out; any placement will do (stems_ragged_layout: the compact one, whose
        arrays with their totals are accepted as they are).  Clip i's block has the bits execute_masked_stems gives that clip and its masks
        alone.  Output blocks that overlap are not detected."""
        self._execute_masked_ragged(_MASKED_STEMS, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets, n_stems)

    def execute_imdct_ragged(self, d_coefs, in_offsets, frames, d_out, out_offsets):
        """Enqueue the IMDCT of coefficient blocks of different frame counts on the plan's stream (asynchronous; zafx_execute_imdct_ragged,
        inverse MDCT plans only).  Block i starts at element in_offsets[i] of d_coefs: W/2 rows of frames[i] coefficients at the pitch
        row_pitch(frames[i]) ("FT" -- the blocks a forward plan's execute_ragged writes at the same row_align), or frames[i] x W/2 compact
        ("TF"); its max((W/2) (frames[i] - 1) - 1, 0) samples go to element out_offsets[i] of d_out.  Float32 "FT" plans of window 512, 1024
        and 2048 whose pitches are multiples of 4 run as one launch (last_kernel: k_imdct_ragged), the others as one execute per clip.  Output
        ranges that overlap are not detected."""
        m = int(self.params.window_length) // 2
        self._execute_blocks_ragged("zafx_execute_imdct_ragged", "coefficients", "d_coefs", m, lambda t: np.maximum(m * (t - 1) - 1, 0),
                                    d_coefs, in_offsets, frames, d_out, out_offsets)

    def execute_istft_ragged(self, d_spec, in_offsets, frames, d_out, out_offsets):
        """Enqueue the inverse STFT of spectra of different frame counts on the plan's stream (asynchronous; zafx_execute_istft_ragged,
        inverse STFT plans only).  Block i starts at complex element in_offsets[i] of d_spec: W rows (W/2 + 1 for a one-sided plan) of
        frames[i] bins at the pitch row_pitch(frames[i]) ("FT" -- the blocks an STFT plan's execute_ragged writes at the same row_align and
        spectrum), or frames[i] x rows compact ("TF"); its max(frames[i] H - (W - H), 0) samples go to element out_offsets[i] of d_out.
        Float32 "FT" plans of window 256 ... 2048 run as one launch (last_kernel: k_istft_ragged), the others as one execute per clip.
        Output ranges that overlap are not detected."""
        w, h = int(self.params.window_length), int(self.params.step_length)
        self._execute_blocks_ragged("zafx_execute_istft_ragged", "spectra", "d_spec", w // 2 + 1 if self.params.spectrum else w,
                                    lambda t: np.maximum(t * h - (w - h), 0), d_spec, in_offsets, frames, d_out, out_offsets)

    def _execute_blocks_ragged(self, entry, what, name, rows, out_len, d_in, in_offsets, frames, d_out, out_offsets):
        """execute_imdct_ragged / execute_istft_ragged: the checks of the per-block arrays and of both buffers, then the library's `entry`.  A
        block is `rows` rows; `out_len`: the samples blocks of these frame counts give; `what` and `name`: d_in in the messages."""
        in_offsets, frames, out_offsets = _as_int64(in_offsets, "in_offsets"), _as_int64(frames, "frames"), _as_int64(out_offsets, "out_offsets")
        if not len(in_offsets) == len(frames) == len(out_offsets):
            raise ValueError("in_offsets, frames and out_offsets must have one entry per block")
        if d_in.dtype != self.in_dtype or d_out.dtype != self.out_dtype:
            raise ValueError(f"{entry[5:]} takes {self.in_dtype} {what} and a {self.out_dtype} output buffer")
        if len(frames) and min(int(frames.min()), int(in_offsets.min()), int(out_offsets.min())) >= 0:   # (negative values: the library says so)
            if self.layout == _lib.LAYOUT_FT:
                a = max(self.row_align, 1)
                ends = in_offsets + rows * ((frames + a - 1) // a * a)   # (whole rows: the 16-byte gather may read a row's pad columns)
            else:
                ends = in_offsets + frames * rows
            if int(ends.max()) * d_in.dtype.itemsize > d_in.nbytes:
                raise ValueError(f"a block reaches past the end of {name}")
            if int((out_offsets + out_len(frames)).max()) * d_out.dtype.itemsize > d_out.nbytes:
                raise ValueError("a clip's result reaches past the end of d_out")
        _lib.check(getattr(_lib.load(), entry)(self.handle, d_in.ptr, _i64p(in_offsets), _i64p(frames), d_out.ptr, _i64p(out_offsets), len(frames)), entry)

    def sync(self):
        _lib.check(_lib.load().zafx_sync(self.handle), "zafx_sync")

    def pcm_to_float(self, d_pcm, d_out, n_clips, n_frames, n_channels):
        """Enqueue wavread's normalisation + channel mean on this plan's stream (int16/int32 PCM in)."""
        _lib.check(_lib.load().zafx_pcm_to_float(self.handle, d_pcm.ptr, d_out.ptr, int(n_clips), int(n_frames),
                                                int(n_channels), d_pcm.dtype.itemsize), "zafx_pcm_to_float")

    def execute_pcm(self, d_pcm, d_out, n_clips, n_frames, n_channels=1):
        """execute() on integer PCM that is already on the device: d_pcm = (clips, frames[, channels]) int16 / int32 interleaved.  At window 2048
        mel, mfcc (and their one-pass form), the complex and the |X| / |X|^2 kinds of the STFT and the MDCT read int16 (one or two channels)
        in their own loads -- 2 bytes per sample and channel of HBM traffic instead of the pre-pass's 6 + 4 --, every other plan converts,
        in chunks of clips, into a bounded staging array it owns first (zafx_execute_pcm, include/zafx.h; zaf.py:1202 and :65 either way)."""
        if d_pcm.dtype not in (np.dtype(np.int16), np.dtype(np.int32)):
            raise ValueError("execute_pcm takes an int16 or int32 DeviceBuffer (wavread's other dtypes: convert on the host)")
        n_clips, n_frames, n_channels = int(n_clips), int(n_frames), int(n_channels)
        if int(np.prod(d_pcm.shape, dtype=np.int64)) < n_clips * n_frames * n_channels:
            raise ValueError("d_pcm holds fewer than clips x frames x channels samples")
        if d_out.nbytes < n_clips * self.clip_bytes(n_frames)[1]:
            raise ValueError("d_out is smaller than the plan's output for these clips")
        with self.lock:   # (the plan's staging array of the two-step route is shared state)
            _lib.check(_lib.load().zafx_execute_pcm(self.handle, d_pcm.ptr, d_out.ptr, n_clips, n_frames, n_channels,
                                                   d_pcm.dtype.itemsize), "zafx_execute_pcm")

    def execute_ragged_pcm(self, d_pcm, in_offsets, lengths, d_out, n_channels=1):
        """execute_ragged() on integer PCM that is already on the device (asynchronous; zafx_execute_ragged_pcm): d_pcm holds interleaved int16 /
        int32 sample frames of n_channels channels, clip i is lengths[i] sample frames at sample frame in_offsets[i], and its result -- that of
        execute_ragged on the normalised mono clip -- goes to the block ragged_layout(lengths) assigns in d_out.  int16 mono / stereo at window
        2048 on a grid of lines is read by the ragged kernels themselves (last_kernel as execute_ragged's; even hop and offsets, d_pcm on 8
        bytes -- the MDCT: offsets and lengths multiples of 4, d_pcm on 16 bytes); every other batch converts, in groups of clips, into a
        bounded staging array the plan owns and runs execute_ragged on that (include/zafx.h)."""
        lengths, in_offsets = _as_lengths(lengths), _as_lengths(in_offsets, "in_offsets")
        n_channels = int(n_channels)
        if len(in_offsets) != len(lengths):
            raise ValueError("in_offsets and lengths must have one entry per clip")
        if n_channels < 1:
            raise ValueError("n_channels must be at least 1")
        if d_pcm.dtype not in (np.dtype(np.int16), np.dtype(np.int32)) or d_out.dtype != self.out_dtype:
            raise ValueError(f"execute_ragged_pcm takes int16 or int32 sample frames and a {self.out_dtype} output buffer")
        if len(lengths) and int((in_offsets + lengths).max()) > d_pcm.nbytes // (d_pcm.dtype.itemsize * n_channels):
            raise ValueError("a clip reaches past the end of d_pcm")
        if int(self._ragged_offsets(lengths)[-1]) * self.out_dtype.itemsize > d_out.nbytes:
            raise ValueError("d_out is smaller than the ragged batch's output (ragged_layout)")
        # (the plan's staging array of the convert-first route is shared state: serialise calls on one plan, as the *_pcm_ragged functions do
        # under the plan's lock)
        _lib.check(_lib.load().zafx_execute_ragged_pcm(self.handle, d_pcm.ptr, _i64p(in_offsets), _i64p(lengths), d_out.ptr, len(lengths),
                                                      n_channels, d_pcm.dtype.itemsize), "zafx_execute_ragged_pcm")

    def timer_start(self):
        _lib.check(_lib.load().zafx_timer_start(self.handle), "zafx_timer_start")

    def timer_stop(self):
        ms = ctypes.c_float(0)
        _lib.check(_lib.load().zafx_timer_stop(self.handle, ctypes.byref(ms)), "zafx_timer_stop")
        return ms.value

    @property
    def kernel_name(self):
        """The kernel family the plan was built for (does not change with the calls)."""
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.load().zafx_plan_kernel_name(self.handle, buf, 128), "zafx_plan_kernel_name")
        return buf.value.decode()

    @property
    def last_kernel(self):
        """The kernel the last execute / run_host really launched (carry, band and generic forms are chosen per call);
        the planned name before the first one."""
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.load().zafx_plan_last_kernel_name(self.handle, buf, 128), "zafx_plan_last_kernel_name")
        return buf.value.decode() or self.kernel_name

    def _compute_units(self):
        used, device = ctypes.c_int(), ctypes.c_int()
        _lib.check(_lib.load().zafx_plan_compute_units(self.handle, ctypes.byref(used), ctypes.byref(device)), "zafx_plan_compute_units")
        return used.value, device.value

    @property
    def compute_units(self):
        """The compute units the plan sizes its launches for: the device's, or fewer under ZAFX_COMPUTE_UNITS at the plan's creation."""
        return self._compute_units()[0]

    @property
    def device_compute_units(self):
        """The compute units of the plan's device."""
        return self._compute_units()[1]

    @property
    def cqt_form(self):
        """The form of k_cqt the last execute of a float32 CQT / chroma plan launched (zafx_plan_cqt_form): "matrix-core" or "lane-reduction";
        None before the first launch and for every other plan."""
        form = ctypes.c_int()
        _lib.check(_lib.load().zafx_plan_cqt_form(self.handle, ctypes.byref(form)), "zafx_plan_cqt_form")
        return {1: "matrix-core", 2: "lane-reduction"}.get(form.value)

    def clip_bytes(self, n_in):
        """(input bytes, output bytes) of ONE clip for `n_in` (zafx_plan_clip_bytes; rows at the plan's pitch)."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.load().zafx_plan_clip_bytes(self.handle, int(n_in), ctypes.byref(a), ctypes.byref(b)), "zafx_plan_clip_bytes")
        return int(a.value), int(b.value)

    def run_host(self, array, n_in, out=None, chunk_clips=0):
        """Host array in -> device transform -> host array out: the reference's own boundary (zaf.py:45), PCIe both ways.

        One call of zafx_run_host: the clips travel in chunks over two HIP streams with plan-owned staging buffers in HBM,
        so the upload, the kernel and the download of neighbouring chunks overlap.  `out`: destination array of
        Plan.out_shape(n_clips, n_in) and Plan.out_dtype -- with page-locked arrays on both sides (pinned_empty, reused
        across calls) the call runs at the PCIe rate of its slower direction; pageable arrays work and are staged."""
        array = np.asarray(array)
        if np.iscomplexobj(array) and self.in_dtype.kind != "c":
            raise ValueError("this plan takes real input")
        frames = None
        if self.row_align > 1 and self.kind not in self._FORWARD and array.ndim == 3:
            # padded rows on the device, compact (F, T) indexing on the host side.  An array that already IS rows of this pitch -- the view a
            # forward *_batch call handed back -- goes as it lies; anything else is copied into a padded array first
            pitch = self.row_pitch(n_in)
            whole = _rows_with_pitch(array, pitch) if array.dtype == self.in_dtype else None
            if whole is None:
                whole = np.zeros(array.shape[:2] + (pitch,), dtype=self.in_dtype)
                whole[:, :, :array.shape[2]] = array
            array = whole
        array = np.ascontiguousarray(array, dtype=self.in_dtype)   # (an array of another dtype would be reinterpreted byte-wise)
        n_clips = array.shape[0]
        if self.row_align > 1 and self.kind in self._FORWARD:
            frames = self.out_dims(n_in)[1]
        shape = self.out_shape(n_clips, n_in)
        if out is None:
            out = np.empty(shape, dtype=self.out_dtype)
        elif tuple(out.shape) != tuple(shape) or out.dtype != self.out_dtype or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError(f"out must be a writeable C-contiguous {self.out_dtype} array of shape {tuple(shape)}")
        in_b, out_b = self.clip_bytes(n_in)
        if array.nbytes != n_clips * in_b or out.nbytes != n_clips * out_b:   # (the library walks both arrays by these sizes)
            raise ValueError(f"array sizes do not match the plan: {array.nbytes} B in for {n_clips} clips of {in_b} B, "
                             f"{out.nbytes} B out for clips of {out_b} B")
        if n_clips and out.nbytes:
            with self.lock:
                _lib.check(_lib.load().zafx_run_host(self.handle, _ptr(array), _ptr(out), n_clips, int(n_in), int(chunk_clips)),
                           "zafx_run_host")
        return out if frames is None else out[:, :, :frames]

    def run_host_pcm(self, pcm, out=None, chunk_clips=0):
        """run_host for integer PCM as wavread's source holds it (zaf.py:1187-1204): pcm = (clips, frames[, channels]) int16 or
        int32, interleaved.  The integers cross PCIe (2-4 bytes per sample and channel), x / 2^(bits-1) (zaf.py:1202) and the
        channel mean (zaf.py:65) run on the device in front of the transform (zafx_run_host_pcm)."""
        pcm = np.ascontiguousarray(pcm)
        if pcm.dtype not in (np.dtype(np.int16), np.dtype(np.int32)):
            raise ValueError("PCM ingest takes int16 or int32 samples (wavread's other dtypes: convert on the host)")
        if pcm.ndim == 2:
            pcm = pcm[:, :, None]
        if pcm.ndim != 3:
            raise ValueError("pcm must be (clips, frames) or (clips, frames, channels)")
        if self.f64 or self.kind not in self._FORWARD + (_lib.DCT,):
            raise ValueError("PCM ingest feeds the float32 plans that take samples")
        n_clips, n_in, channels = pcm.shape
        frames = self.out_dims(n_in)[1] if self.row_align > 1 else None
        shape = self.out_shape(n_clips, n_in)
        if out is None:
            out = np.empty(shape, dtype=self.out_dtype)
        elif tuple(out.shape) != tuple(shape) or out.dtype != self.out_dtype or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError(f"out must be a writeable C-contiguous {self.out_dtype} array of shape {tuple(shape)}")
        if n_clips and out.nbytes:
            with self.lock:
                _lib.check(_lib.load().zafx_run_host_pcm(self.handle, _ptr(pcm), _ptr(out), n_clips, n_in, channels, pcm.dtype.itemsize,
                                                         int(chunk_clips)), "zafx_run_host_pcm")
        return out if frames is None else out[:, :, :frames]

    def destroy(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            _lib.load().zafx_plan_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Comm:
    """RCCL communicator (one process per GPU); only used to broadcast plan constants."""

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.load().zafx_comm_unique_id(buf), "zafx_comm_unique_id")
        return buf.raw

    def __init__(self, device, rank, n_ranks, unique_id):
        if len(unique_id) != 128:
            raise ValueError("unique_id must be 128 bytes")
        self._id = ctypes.create_string_buffer(bytes(unique_id), 128)
        h = ctypes.c_void_p()
        _lib.check(_lib.load().zafx_comm_create(ctypes.byref(h), int(device), int(rank), int(n_ranks), self._id), "zafx_comm_create")
        self.handle = h
        self.rank, self.n_ranks = int(rank), int(n_ranks)

    def count(self):
        """Number of ranks in the communicator as RCCL reports it (ncclCommCount)."""
        n = ctypes.c_int(0)
        _lib.check(_lib.load().zafx_comm_count(self.handle, ctypes.byref(n)), "zafx_comm_count")
        return n.value

    def user_rank(self):
        """This process's rank as RCCL reports it (ncclCommUserRank)."""
        n = ctypes.c_int(-1)
        _lib.check(_lib.load().zafx_comm_user_rank(self.handle, ctypes.byref(n)), "zafx_comm_user_rank")
        return n.value

    def broadcast_constants(self, plan, root=0):
        _lib.check(_lib.load().zafx_comm_broadcast_constants(self.handle, plan.handle, int(root)), "zafx_comm_broadcast_constants")

    def destroy(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            _lib.load().zafx_comm_destroy(self.handle)
            self.handle = ctypes.c_void_p()


# ======================================================================================
# plan cache (thread safe): plans are keyed by geometry + a digest of their constants
# ======================================================================================
_cache = {}
_cache_lock = threading.Lock()
_CACHE_MAX = 32


def _digest(*arrays):
    import hashlib
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _cached(key, factory):
    """The plan under `key`, built by `factory()` on a miss.  The factory runs OUTSIDE the cache lock (a dct / dst plan builds
    an N x N float64 matrix, O(N^2) trigonometry: other threads' lookups must not wait for it); when two threads miss on the
    same key at once both build, the first insert wins and the loser's plan is destroyed."""
    with _cache_lock:
        plan = _cache.get(key)
    if plan is not None:
        return plan
    fresh = factory()
    with _cache_lock:
        plan = _cache.get(key)
        if plan is None:
            if len(_cache) >= _CACHE_MAX:
                _cache.pop(next(iter(_cache)))   # freed by Plan.__del__ once no caller still holds it
            _cache[key] = plan = fresh
            fresh = None
    if fresh is not None:
        fresh.destroy()
    return plan


def clear_plan_cache():
    with _cache_lock:
        for plan in _cache.values():
            plan.destroy()
        _cache.clear()
    DeviceBuffer.drain_pool()


# ======================================================================================
# argument checking shared by the drop-in and batched entry points
# ======================================================================================
def _pow2(n):
    return n > 0 and not n & (n - 1)


def _tuned(n):
    """Window lengths of the tiled float32 kernels (powers of two)."""
    return _pow2(n) and 64 <= n <= 8192


def _f32_window(n):
    """Window lengths with float32 kernels: the powers of two 64 ... 8192 (tiled kernels) and every other length 33 ... 8192
    (float32 Bluestein forms of STFT / ISTFT / MDCT / IMDCT, zafx_bs32.hip); the rest (below 33 samples) runs in float64."""
    return _tuned(n) or (33 <= n <= 8192 and not _pow2(n))


def _as_window(window_function, any_length=False):
    """any_length: windows that are not a power of two, up to 8192 samples (float32 Bluestein forms; the float64 ones stop
    at 2048)."""
    w = np.asarray(window_function, dtype=np.float64)
    if w.ndim != 1:
        raise ValueError("window_function must be 1-D")
    n = len(w)
    if any_length and not _tuned(n):
        if n < 2 or n > 8192:
            raise ValueError(f"zafx takes windows of 2 ... 8192 samples, got {n}")
        return w
    if not _tuned(n):
        raise ValueError(f"zafx kernels need a power-of-two window_length in [64, 8192], got {n}")
    return w


def _check_f64_window(n, f64):
    """float64 plans take the powers of two 64 ... 8192 and any other length up to 2048 (the float64 Bluestein forms stop
    there; the float32 ones reach 8192): validated here, ahead of the device."""
    if f64 and not _pow2(n) and n > 2048:
        raise ValueError(f"f64=True takes windows that are not a power of two only up to 2048 samples, got {n}")


def _as_step(step_length):
    if isinstance(step_length, (bool, np.bool_)) or not isinstance(step_length, (int, np.integer)):
        raise ValueError("step_length must be an int (as in zaf.stft)")
    if step_length < 1:
        raise ValueError("step_length must be >= 1")
    return int(step_length)


def _as_clips(audio, ndim_name="audio_signal", dtype=np.float32):
    a = np.asarray(audio)
    if a.ndim != 2:
        raise ValueError(f"{ndim_name} batch must be 2-D (clips, samples)")
    if np.iscomplexobj(a):
        raise ValueError(f"{ndim_name} must be real")
    return np.ascontiguousarray(a, dtype=dtype)


def _as_signal(audio_signal, dtype=np.float32):
    a = np.asarray(audio_signal)
    if a.ndim != 1:
        raise ValueError("audio_signal must be 1-D (one clip); use the *_batch functions for (clips, samples)")
    return _as_clips(a[None, :], dtype=dtype)


# Arithmetic of the drop-in transforms (every zaf.* function on the path): "f32" (default, the tuned kernels) or "f64" (the
# reference's own dtype on the device, within 1e-12 of zaf.py).
_PRECISION = {"value": "f32"}


def set_precision(precision):
    """Select the device arithmetic of the drop-in transforms (`stft`, `istft`, `mdct`, `imdct`, `melspectrogram`, `mfcc`,
    `cqtspectrogram`, `cqtchromagram`): "f32" (the tuned kernels) or "f64" (the reference's own dtype, within 1e-12 of it)."""
    if precision not in ("f32", "f64"):
        raise ValueError('precision must be "f32" or "f64"')
    _PRECISION["value"] = precision


def get_precision():
    return _PRECISION["value"]


# ======================================================================================
# plan factories
# ======================================================================================
def stft_plan(window_function, step_length, layout="FT", device=0, onesided=False, f64=False, row_align=0):
    """row_align (every 2-D plan factory): pad the rows of the device (F, T) array to a multiple of this many elements
    (16 for complex64, 32 for float32 = one 128-byte line) so that the reference-layout kernels run at their aligned
    rate for any T; Plan.out_shape / Plan.row_pitch give the padded geometry, 0 keeps the reference's compact order.
    A window outside the float32 kernels (below 33 samples) yields a float64 plan whatever `f64` says: Plan.in_dtype /
    Plan.out_dtype tell which arrays it takes."""
    w, h = _as_window(window_function, any_length=True), _as_step(step_length)   # (a hop above the window skips samples, as zaf.stft does)
    f64 = bool(f64) or not _f32_window(len(w))   # (windows below 33 samples: float64 Bluestein kernels)
    _check_f64_window(len(w), f64)
    key = ("stft", device, len(w), h, _LAYOUTS[layout], _spectrum_of(onesided), bool(f64), _as_row_align(row_align, layout), _digest(w))

    def make():
        p = Plan(_lib.STFT, device, window_length=len(w), step_length=h, layout=layout, onesided=onesided, f64=f64,
                 row_align=row_align)
        p.set_window(w)
        return p
    return _cached(key, make)


def istft_plan(window_function, step_length, layout="FT", device=0, onesided=False, f64=False, row_align=0):
    w, h = _as_window(window_function, any_length=True), _as_step(step_length)
    if h > len(w):
        raise ValueError("step_length must not exceed window_length")
    if onesided not in (False, True):
        raise ValueError("istft takes a complex spectrum: onesided must be False or True")
    # the tiled float32 overlap-add keeps 16 frames in LDS (8 at W = 4096, 4 at 8192); for a hop so small that more frames than
    # that cover one sample -- and for every window that is not a power of two -- the library takes the float32 frames +
    # gather overlap-add form of zafx_bs32.hip, which has no such limit (zafx_plan_create decides)
    f64 = bool(f64) or not _f32_window(len(w))
    _check_f64_window(len(w), f64)
    key = ("istft", device, len(w), h, _LAYOUTS[layout], bool(onesided), bool(f64), _as_row_align(row_align, layout), _digest(w))

    def make():
        p = Plan(_lib.ISTFT, device, window_length=len(w), step_length=h, layout=layout, onesided=onesided, f64=f64,
                 row_align=row_align)
        p.set_window(w)
        return p
    return _cached(key, make)


def mdct_plan(window_function, layout="FT", device=0, inverse=False, row_align=0, f64=False):
    w = _as_window(window_function, any_length=True)
    if len(w) % 2 or len(w) < 4:
        raise ValueError("the MDCT needs an even window_length >= 4")
    f64 = bool(f64) or not _f32_window(len(w))   # (even lengths below 34: float64 Bluestein kernels)
    _check_f64_window(len(w), f64)
    key = ("imdct" if inverse else "mdct", device, len(w), _LAYOUTS[layout], _as_row_align(row_align, layout), bool(f64), _digest(w))

    def make():
        p = Plan(_lib.IMDCT if inverse else _lib.MDCT, device, window_length=len(w), layout=layout, row_align=row_align, f64=f64)
        p.set_window(w)
        return p
    return _cached(key, make)


def _dense_filterbank(mel_filterbank, window_length):
    if not hasattr(mel_filterbank, "toarray"):
        raise ValueError("mel_filterbank must be a scipy.sparse matrix (as returned by melfilterbank)")
    fb = np.asarray(mel_filterbank.toarray(), dtype=np.float64)
    if fb.ndim != 2 or fb.shape[1] != window_length // 2:
        raise ValueError("mel_filterbank must have window_length/2 columns")
    return fb


def mel_plan(window_function, step_length, mel_filterbank, number_coefficients=None, layout="FT", device=0, row_align=0, f64=False, also_mel=False):
    """also_mel (with number_coefficients): the one-pass melspectrogram + mfcc plan (zafx_params.with_mel) -- its output holds the melspectrogram's
    rows, then the MFCCs' (mel_mfcc_batch splits them).  float32, window 2048, up to 128 filters and 32 coefficients: mel_mfcc_supported()."""
    w, h = _as_window(window_function, any_length=True), _as_step(step_length)
    if not hasattr(mel_filterbank, "toarray"):
        raise ValueError("mel_filterbank must be a scipy.sparse matrix (as returned by melfilterbank)")
    if mel_filterbank.ndim != 2 or mel_filterbank.shape[1] != len(w) // 2:
        raise ValueError("mel_filterbank must have window_length/2 columns")
    n_filters = mel_filterbank.shape[0]
    mfcc = number_coefficients is not None
    ncoef = int(number_coefficients) if mfcc else 0
    if mfcc and not 1 <= ncoef <= n_filters - 1:
        raise ValueError("number_coefficients must be in [1, number_filters - 1]")
    if len(w) > 8192:
        raise ValueError(f"melspectrogram / mfcc take windows of up to 8192 samples, got {len(w)}")
    # W = 4096: the fused two-band kernel; W = 8192 and windows that are not a power of two (33 ... 8192 samples: the float32 Bluestein
    # STFT) run as a spectrum kernel + the banded filterbank kernel k_melfb over a plan-owned scratch, in float32 -- as do filterbanks of 257 ... 576 rows at any
    # window; filterbanks above 576 rows and windows below 33 samples run on the float64 kernel (any power-of-two window and, up to 2048 samples, any other length)
    f64 = bool(f64) or n_filters > 576 or not _f32_window(len(w))
    if f64 and len(w) > 2048 and not _pow2(len(w)):
        raise ValueError(f"melspectrogram / mfcc in float64 (f64=True, or more than 576 filters) take windows of up to 2048 samples or the powers of two 4096 and 8192, got {len(w)}")
    # the cache key hashes the sparse triplet (a few KB), not the dense matrix (1 MB: 1.8 ms per call)
    csr = mel_filterbank.tocsr()
    also_mel = bool(also_mel)
    if also_mel and not mel_mfcc_supported(len(w), n_filters, ncoef if mfcc else 0, f64):
        raise ValueError("also_mel needs number_coefficients <= 32, a float32 plan of window 2048 and up to 128 filters (mel_mfcc_batch runs two plans otherwise)")
    key = ("mfcc" if mfcc else "mel", device, len(w), h, _LAYOUTS[layout], ncoef, n_filters, _as_row_align(row_align, layout), bool(f64), also_mel,
           _digest(w, csr.data, csr.indices, csr.indptr))

    def make():
        fb = _dense_filterbank(mel_filterbank, len(w))
        p = Plan(_lib.MFCC if mfcc else _lib.MEL, device, window_length=len(w), step_length=h, layout=layout,
                 n_filters=fb.shape[0], n_coefs=ncoef, row_align=row_align, f64=f64, with_mel=also_mel)
        p.set_window(w)
        p.set_mel_filterbank(fb)
        if mfcc:
            p.set_dct(constants.dct2_rows(n_filters, ncoef))
        return p
    return _cached(key, make)


def mel_mfcc_supported(window_length, number_filters, number_coefficients, f64=False):
    """Geometries of the one-pass melspectrogram + mfcc kernel (k_mel2 MODE 4)."""
    return (not f64) and window_length == 2048 and 1 <= number_filters <= 128 and 1 <= number_coefficients <= min(32, number_filters - 1)


def _cqt_f32_max_bins(fft_length):
    """Rows of a kernel matrix the float32 k_cqt holds at this fft_length (zafx_cqt_max_bins); 0 outside its sizes."""
    n = ctypes.c_int(0)
    _lib.check(_lib.load().zafx_cqt_max_bins(int(fft_length), ctypes.byref(n)), "zafx_cqt_max_bins")
    return n.value


_CQT_MIN_FFT = 512   # shortest frame of the device kernels


def _cqt_embed(cqt_kernel, step, target=_CQT_MIN_FFT):
    """A kernel whose fft_length L is below the device kernels' minimum, rewritten for frames of `target` samples.

    K . fft(frame) = G . frame with G = fft(K, axis=1) (the kernel's rows in the time domain, zaf.py:630-632), so the same
    numbers come out of K' . fft(frame') for the longer frame' when G' holds G at the offset d by which the longer frame
    starts earlier (left padding ceil((L - step) / 2) -> ceil((target - step) / 2), zaf.py:612-620) and zeros elsewhere,
    and K' = ifft(G', axis=1).  K' is dense (target columns per row): small, since L < target."""
    import scipy.sparse
    k = np.asarray(cqt_kernel.toarray(), dtype=np.complex128)
    length = k.shape[1]
    d = -((step - target) // 2) - -((step - length) // 2)   # ceil((target - step) / 2) - ceil((L - step) / 2)
    g = np.zeros((k.shape[0], target), np.complex128)
    g[:, d:d + length] = np.fft.fft(k, axis=1)
    return scipy.sparse.csr_matrix(np.fft.ifft(g, axis=1))


def cqt_plan(sampling_frequency, time_resolution, cqt_kernel, octave_resolution=None, layout="FT", device=0, row_align=0, f64=False):
    if not hasattr(cqt_kernel, "tocsr"):
        raise ValueError("cqt_kernel must be a scipy.sparse matrix (as returned by cqtkernel)")
    n_bins, fft_length = cqt_kernel.shape
    step = round(sampling_frequency / time_resolution)   # zaf.py:603 (banker's rounding)
    if step < 1:
        raise ValueError("time_resolution too high for this sampling_frequency")
    if step > fft_length:   # (the reference's right padding floor((fft_length - step) / 2) is negative there: np.pad raises, zaf.py:612-620)
        raise ValueError("step (sampling_frequency / time_resolution) exceeds the kernel's fft_length")
    if 2 <= fft_length < _CQT_MIN_FFT:
        # (a short kernel -- few bins per octave, high minimum frequency -- of any length, power of two or not)
        cqt_kernel = _cqt_embed(cqt_kernel, step)
        fft_length = _CQT_MIN_FFT
    if fft_length < _CQT_MIN_FFT or fft_length > 131072 or fft_length & (fft_length - 1):
        raise ValueError(f"zafx CQT kernels need a power-of-two fft_length in [512, 131072] (or any length below 512), got {fft_length}")
    # a frame above 65536 samples runs on the float64 kernel, which decimates the frame; so do kernels with more rows than
    # fit beside the frame (k_cqt keeps the whole frame + one output column of the kernel's rows in the 160 KB of LDS:
    # about 4 000 rows at fft_length 32768 -- the reference's own 208-row example is far inside)
    csr = cqt_kernel.tocsr()
    # fft_length 65536 (minimum frequencies down to 23 Hz at 44.1 kHz, 24 bins per octave) runs on the float32 kernel as the even and
    # the odd bins of two 16384-point transforms when the matrix touches the low bins 1 ... 8191 (and their mirrors) only
    low_band = True
    if fft_length == 65536 and csr.nnz:
        m = np.minimum(csr.indices, fft_length - csr.indices)
        low_band = bool(m.min() >= 1 and m.max() <= 8191)
    f64 = bool(f64) or fft_length > 65536 or not low_band or n_bins > _cqt_f32_max_bins(fft_length)
    chroma = octave_resolution is not None
    key = ("chroma" if chroma else "cqt", device, fft_length, step, n_bins, int(octave_resolution or 0), _LAYOUTS[layout],
           _as_row_align(row_align, layout), bool(f64),
           _digest(csr.indptr, csr.indices, csr.data))

    def make():
        p = Plan(_lib.CHROMA if chroma else _lib.CQT, device, step_length=step, layout=layout, fft_length=fft_length,
                 n_bins=n_bins, octave_resolution=int(octave_resolution or 0), row_align=row_align, f64=f64)
        p.set_cqt_kernel(csr)
        return p
    return _cached(key, make)


def _center_window(window_function, step_length):
    """Window and hop of the center / sides kinds, checked without the library: float32 kernels for the powers of two 256 ... 2048,
    and only the hop window_length / 2 (zaf.stft pads W/2 in front, zaf.istft trims W - H: the example works at no other hop)."""
    w = np.asarray(window_function, dtype=np.float64)
    if w.ndim != 1:
        raise ValueError("window_function must be 1-D")
    if not _pow2(len(w)) or not 256 <= len(w) <= 2048:
        raise ValueError(f"center / sides kernels need a power-of-two window_length in [256, 2048], got {len(w)}")
    if step_length is not None and _as_step(step_length) != len(w) // 2:
        raise ValueError(f"step_length must be window_length / 2 = {len(w) // 2} for the center / sides extraction, got {step_length}")
    return w


def center_plan(window_function, device=0, sides=True):
    """Plan of the center / sides extraction (zaf.py:155-198) at step_length = window_length / 2: stereo (B, N, 2) float32 in,
    (B, 2, N, 2) out (block 0 the center, block 1 the sides), or (B, N, 2), the center alone, with sides=False."""
    w = _center_window(window_function, None)
    key = ("center", device, len(w), bool(sides), _digest(w))

    def make():
        p = Plan(_lib.CENTER_SIDES if sides else _lib.CENTER, device, window_length=len(w), step_length=len(w) // 2)
        p.set_window(w)
        return p
    return _cached(key, make)


def _maskfilter_window(window_function, step_length):
    """Window and hop of the mask filter kinds, checked without the library: those of the center / sides kinds."""
    w = np.asarray(window_function, dtype=np.float64)
    if w.ndim != 1:
        raise ValueError("window_function must be 1-D")
    if not _pow2(len(w)) or not 256 <= len(w) <= 2048:
        raise ValueError(f"the mask filter needs a power-of-two window_length in [256, 2048], got {len(w)}")
    if step_length is not None and _as_step(step_length) != len(w) // 2:
        raise ValueError(f"step_length must be window_length / 2 = {len(w) // 2} for the mask filter, got {step_length}")
    return w


def maskfilter_plan(window_function, rest=False, layout="FT", device=0, row_align=0):
    """Plan of the mask filter y = istft(concat(m, m[-2:0:-1]) * stft(x))[0:N] (zaf.py:185-195 with the caller's mask) at step_length =
    window_length / 2: mono (B, N) float32 and a mask of Plan.mask_shape in, (B, N) out, or (B, 2, N) -- block 0 the filtered clip, block 1
    the rest x - y -- with rest=True.  layout / row_align: of the mask; "TF", (B, T, W/2 + 1), is the faster one."""
    w = _maskfilter_window(window_function, None)
    a = _as_row_align(row_align, layout)
    key = ("maskfilter", device, len(w), bool(rest), _LAYOUTS[layout], a, _digest(w))

    def make():
        p = Plan(_lib.MASKFILTER_REST if rest else _lib.MASKFILTER, device, window_length=len(w), step_length=len(w) // 2, layout=layout, row_align=a)
        p.set_window(w)
        return p
    return _cached(key, make)


def linear_plan(matrix, device=0):
    """y = matrix @ x for every clip (the carrier of the dct / dst transforms)."""
    m = np.ascontiguousarray(matrix, dtype=np.float64)
    if m.ndim != 2 or not (1 <= m.shape[0] <= 16384 and 1 <= m.shape[1] <= 16384):
        raise ValueError("matrix must be 2-D with both sides in [1, 16384]")
    key = ("linear", device, m.shape, _digest(m))

    def make():
        p = Plan(_lib.LINEAR, device, window_length=m.shape[1], n_filters=m.shape[0])
        p.set_matrix(m)
        return p
    return _cached(key, make)


# ======================================================================================
# batched API (build-defined extension): (clips, samples) float32 in, float32/complex64 out
# ======================================================================================
def _run_host_into(plan, x, n_in, out):
    """Plan.run_host with the caller's `out` honoured even when the library promoted the plan to float64 (windows under 33
    samples, more than 576 filters, a CQT outside the float32 kernel's reach): the float64 result is then cast into `out`
    -- which is returned -- instead of raising on the dtype."""
    if out is None or np.dtype(out.dtype) == plan.out_dtype:
        return plan.run_host(x, n_in, out=out)
    res = plan.run_host(x, n_in)
    if tuple(out.shape) != tuple(res.shape) or not out.flags.writeable:
        raise ValueError(f"out must be a writeable array of shape {tuple(res.shape)}")
    np.copyto(out, res, casting="same_kind")
    return out


_ROW_PADDING = {"value": "auto"}


def set_row_padding(mode):
    """How the *_batch functions of the STFT / MDCT families lay out the device (F, T) array when the caller passes neither `out` nor
    `row_align`: "auto" (default) pads the rows to whole 128-byte lines whenever T is off that grid and hands back a view of the padded result
    (_line_grid); "compact" always keeps the reference's own memory order (C-contiguous results, the kernels' off-grid forms)."""
    if mode not in ("auto", "compact"):
        raise ValueError('row padding must be "auto" or "compact"')
    _ROW_PADDING["value"] = mode


def get_row_padding():
    return _ROW_PADDING["value"]


def _line_grid(plan, n_in, out, padded_plan, frames=None, row_align=None):
    """The plan a *_batch call of the STFT / MDCT families runs: when the frame count T is off the 128-byte line grid of the (F, T) rows in the
    reference layout (the usual case: T % 16 != 0 for complex64 rows), the device array gets padded rows (row_align = one line) -- the kernels then
    run at the rate they have on the grid (T = 433 against 432: ISTFT 0.47 -> 0.63 of HBM, |X| rows 0.34 -> 0.49, MDCT 0.46 -> 0.58)
    -- and the NumPy array handed back is a VIEW of the padded result: the reference's shape, dtype and indexing, rows `pitch` elements apart
    instead of T (C-contiguity of the result is not part of the reference's contract; np.ascontiguousarray(result) gives the compact
    array).  A caller's own `out` array, the frame-major layout and frame counts on the grid keep the compact plan.  row_align (of the *_batch
    functions): None = this rule, 0 = always the compact device array (the reference's own memory order), n = rows padded to n elements."""
    if row_align is not None:
        return padded_plan(int(row_align)) if int(row_align) > 1 and plan.layout == _lib.LAYOUT_FT else plan
    if out is not None or plan.layout != _lib.LAYOUT_FT or plan.row_align > 1 or _ROW_PADDING["value"] != "auto":
        return plan
    t = plan.out_dims(n_in)[1] if frames is None else int(frames)
    elem = plan.out_dtype if frames is None else plan.in_dtype   # the dtype of the 2-D side
    a = _line_elements(elem)
    return padded_plan(a) if t % a else plan


def stft_batch(clips, window_function, step_length, layout="FT", device=0, onesided=False, f64=False, out=None, row_align=None):
    """(B, N) -> (B, W, T) complex64 [layout "FT"] or (B, T, W) ["TF"].

    out (every *_batch function): destination array of the result's shape and dtype, e.g. a reused zafx.pinned_empty
    array -- with page-locked arrays on both sides the chunked, double-buffered transfer (Plan.run_host) runs at the PCIe rate.
    When the library computes a float32 request in float64 (see Plan.f64) the result is cast into `out` afterwards.

    onesided=True keeps rows 0..W/2 only -- what every example of the reference slices out of the
    result (zaf.py:83) -- and halves the bytes written; onesided="magnitude" / "power" returns |X| / |X|^2
    of those rows as a real array."""
    x = _as_clips(clips, dtype=np.float64 if f64 else np.float32)
    plan = _line_grid(stft_plan(window_function, step_length, layout, device, onesided, f64), x.shape[1], out,
                      lambda a: stft_plan(window_function, step_length, layout, device, onesided, f64, row_align=a), row_align=row_align)
    out = _run_host_into(plan, x.astype(plan.in_dtype, copy=False), x.shape[1], out)
    if f64 or not plan.f64:
        return out
    return out.astype(np.complex64 if np.iscomplexobj(out) else np.float32, copy=False)   # (computed in float64: window not a power of two)


def istft_batch(spectra, window_function, step_length, layout="FT", device=0, onesided=False, f64=False, out=None, row_align=None):
    """(B, W, T) ["FT"] or (B, T, W) ["TF"] complex -> (B, T*H - (W-H)) float32.

    onesided=True takes rows 0..W/2 and completes X[W-k] = conj X[k]: the result equals the two-sided
    call on the spectrum of a real signal."""
    w = _as_window(window_function, any_length=True)
    s = np.asarray(spectra)
    if s.ndim != 3:
        raise ValueError("spectra must be 3-D")
    wl, nt = (s.shape[1], s.shape[2]) if _LAYOUTS[layout] == _lib.LAYOUT_FT else (s.shape[2], s.shape[1])
    if wl != (len(w) // 2 + 1 if onesided else len(w)):
        raise ValueError("spectrum rows must equal window_length (window_length/2 + 1 when onesided)")
    plan = _line_grid(istft_plan(w, step_length, layout, device, onesided, f64), nt, None,
                      lambda a: istft_plan(w, step_length, layout, device, onesided, f64, row_align=a), frames=nt, row_align=row_align)
    out = _run_host_into(plan, s if plan.row_align > 1 else np.ascontiguousarray(s, dtype=plan.in_dtype), nt, out)
    return out if f64 else out.astype(np.float32, copy=False)   # (a very small hop is computed in float64 whatever f64 says)


def centersides_batch(clips, window_function, step_length=None, sides=True, device=0, out=None):
    """The center / sides example of zaf.istft's docstring (zaf.py:155-198) for a batch of stereo clips, in one kernel:
    (B, N, 2) -> (center, sides), float32 (B, N, 2) each -- views of one (B, 2, N, 2) result (which `out`, if given, is) -- or the
    center alone with sides=False.  step_length: None or window_length / 2, the only hop at which the example works.

    The masks are (b < a) ? b / a : 1 and (a < b) ? a / b : 1 of the channels' magnitudes a, b: the reference's min(a, b) / a
    wherever that is finite; where the reference divides 0 by 0 (an exactly silent bin: it returns a frame of NaNs) the
    masked bin is 0, the limit value."""
    w = _center_window(window_function, step_length)
    a = np.asarray(clips)
    if a.ndim != 3 or a.shape[2] != 2:
        raise ValueError(f"clips must be stereo, (clips, sample frames, 2), got shape {a.shape}")
    if np.iscomplexobj(a):
        raise ValueError("clips must be real")
    x = np.ascontiguousarray(a, dtype=np.float32)
    res = center_plan(w, device, sides).run_host(x, x.shape[1], out=out)
    return (res[:, 0], res[:, 1]) if sides else res


def maskfilter_batch(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0, out=None):
    """The mask filter for a batch of mono clips in one kernel: clips (B, N) and real masks (B, W/2 + 1, T) -- (B, T, W/2 + 1) with layout "TF" --,
    T = ceil(N / (W/2)) + 1 as zaf.stft gives -> y = istft(concat(m, m[-2:0:-1]) * stft(x))[0:N] (zaf.py:185-195), float32 (B, N); with rest=True
    (y, rest = x - y), views of one (B, 2, N) result (which `out`, if given, is).  step_length: None or window_length / 2."""
    return _maskfilter_batch(_MASKED_REAL, clips, window_function, masks, step_length, rest, layout, device, out)


def _maskfilter_batch(form, clips, window_function, masks, step_length, rest, layout, device, out):
    """maskfilter_batch and its stems, complex and stereo forms: the checks of clips, masks and `out` ahead of any device call, "FT" masks of a
    kind the device reads in "TF" only transposed, the round trip, and the result split into (filtered, rest) views."""
    w = _maskfilter_window(window_function, step_length)
    a, m = np.asarray(clips), form.as_masks(masks)
    stereo = form.unit_bytes == 8
    if a.ndim != (3 if stereo else 2) or (stereo and a.shape[2] != 2):
        raise ValueError(f"clips must be {'stereo, (clips, sample frames, 2)' if stereo else 'mono, (clips, samples)'}, got shape {a.shape}")
    if form.mask_dtype.kind == "c":
        if np.iscomplexobj(a):
            raise ValueError("clips must be real")
    elif np.iscomplexobj(a) or np.iscomplexobj(m):
        raise ValueError("clips and masks must be real")
    count = form.batch_count(m) if form.batch_count else None
    n_clips, n = a.shape[:2]
    h = len(w) // 2
    ft = _LAYOUTS[layout] == _lib.LAYOUT_FT
    want = (n_clips,) + form.host_shape(count, (n + h - 1) // h + 1, h + 1, ft)
    if m.shape != want:
        raise ValueError(f"masks must have shape {want} for clips of {n} {form.units} (layout {layout!r}), got {m.shape}")
    blocks = form.out_blocks(count, rest)
    shape = (n_clips,) + ((blocks,) if form.stems_out or rest else ()) + a.shape[1:]
    if out is None:
        out = np.empty(shape, np.float32)
    elif tuple(out.shape) != shape or out.dtype != np.float32 or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError(f"out must be a writeable C-contiguous float32 array of shape {shape}")
    if out.size:
        plan = maskfilter_plan(w, rest, "TF" if form.tf_only else layout, device)
        if ft and form.tf_only:
            m = m.transpose((0,) + tuple(i + 1 for i in form.ft_axes(count)))
        tail = () if count is None else (count,)
        _masked_round_trip(plan, a, m, out, lambda d_in, d_mask, d_out: plan._execute_masked(form, d_in, d_mask, d_out, n_clips, n, *tail), form.mask_dtype)
    if form.stems_out:
        return (out[:, :count], out[:, count]) if rest else out
    return (out[:, 0], out[:, 1]) if rest else out


def _masked_round_trip(plan, clips, masks, out, execute, mask_dtype):
    """_maskfilter_batch: clips up as float32 and masks as mask_dtype, execute(d_in, d_mask, d_out) and the wait under the plan's lock, the
    result down into `out`."""
    x, m = np.ascontiguousarray(clips, dtype=np.float32), np.ascontiguousarray(masks, dtype=mask_dtype)
    d_in, d_mask, d_out = (DeviceBuffer(b.shape, b.dtype, plan.device) for b in (x, m, out))
    try:
        d_in.upload(x)
        d_mask.upload(m)
        with plan.lock:
            execute(d_in, d_mask, d_out)
            plan.sync()
            d_out.download(out=out)
    finally:
        for b in (d_in, d_mask, d_out):
            b.free()


def maskfilter_stems_batch(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0, out=None):
    """The mask filter with several masks per clip -- the stems of a source separation -- in one kernel: clips (B, N) and real masks
    (B, S, W/2 + 1, T), the reference's order -- (B, S, T, W/2 + 1) with layout "TF" --, S in 1 .. 8, T = ceil(N / (W/2)) + 1 -> float32
    (B, S, N), stem s of clip b being maskfilter_batch of that clip with masks[b, s], bit for bit; the forward transform of a clip runs once
    for all its stems (k_maskfilter_stems).  With rest=True (stems, rest), rest = ((x - y_0) - y_1) - ... - y_{S-1} in float32, (B, N): views
    of one (B, S + 1, N) result (which `out`, if given, is).  The device reads "TF" masks only: "FT" masks are transposed on the host before
    the upload -- one more pass over the masks in host memory, B S T (W/2 + 1) floats copied with a strided read; hand over "TF" masks where
    that matters.  step_length: None or window_length / 2."""
    return _maskfilter_batch(_MASKED_STEMS, clips, window_function, masks, step_length, rest, layout, device, out)


def maskfilter_complex_batch(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0, out=None):
    """The mask filter under COMPLEX masks for a batch of mono clips in one kernel (k_maskfilter_complex): clips (B, N) real and masks
    (B, W/2 + 1, T), the reference's order -- (B, T, W/2 + 1) with layout "TF" --, real or complex (cast to complex64), T = ceil(N / (W/2)) + 1
    -> y = istft(concat(M, conj(M[-2:0:-1])) * stft(x))[0:N] (zaf.py:185-195 with the mask's Hermitian mirror; istft keeps the real part),
    float32 (B, N); with rest=True (y, rest = x - y), views of one (B, 2, N) result (which `out`, if given, is).  The imaginary parts of mask
    rows 0 and W/2 have no effect.  The device reads "TF" masks only: "FT" masks are transposed on the host before the upload, as
    maskfilter_stems_batch does.  step_length: None or window_length / 2."""
    return _maskfilter_batch(_MASKED_COMPLEX, clips, window_function, masks, step_length, rest, layout, device, out)


def maskfilter_stereo_batch(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0, out=None):
    """The mask filter for a batch of interleaved stereo clips in one kernel (k_maskfilter_stereo): clips (B, N, 2) and real masks, one for both
    channels, (B, W/2 + 1, T) -- (B, T, W/2 + 1) with layout "TF" --, or one per channel, (B, 2, W/2 + 1, T) -- (B, T, 2, W/2 + 1) with "TF" --,
    T = ceil(N / (W/2)) + 1 -> y[:, :, c] = istft(concat(m_c, m_c[-2:0:-1]) * stft(x[:, :, c]))[0:N] (zaf.py:176-198 with the caller's masks),
    float32 (B, N, 2); with rest=True (y, rest = x - y), views of one (B, 2, N, 2) result (which `out`, if given, is).  Both channels of a
    frame share one transform: rounding and non-finite values of one channel reach the other channel of the same frames, never another clip.
    The device reads "TF" masks only: "FT" masks are transposed on the host before the upload, as maskfilter_stems_batch does.
    step_length: None or window_length / 2."""
    return _maskfilter_batch(_MASKED_STEREO, clips, window_function, masks, step_length, rest, layout, device, out)


def _as_pcm_out_dtype(out_dtype):
    dt = np.dtype(out_dtype)
    if dt not in (np.int16, np.float32):
        raise ValueError(f"out_dtype must be int16 or float32, got {dt}")
    return dt


def _as_int16_clips(a, what):
    """`a` as it is if it holds int16; anything else raises (no silent cast: a float or int32 array handed in by mistake would be wrapped)."""
    a = np.asarray(a)
    if a.dtype != np.int16:
        raise ValueError(f"{what} must be int16 PCM, got dtype {a.dtype} (int32 and 24-bit material: convert to float32 and use the float functions)")
    return a


def maskfilter_pcm_batch(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0, out=None, out_dtype=np.int16):
    """The mask filter for a batch of 16-bit PCM clips in one kernel, the integers read and written by the kernel itself (k_maskfilter_pcm,
    k_maskfilter_stereo_pcm): clips int16, (B, N) mono or (B, N, 2) interleaved stereo, uploaded as integers; masks as maskfilter_batch takes
    them for mono clips and as maskfilter_stereo_batch takes them for stereo ones (one for both channels or one per channel).  A sample s
    enters as s / 32768 (zaf.wavread).  out_dtype float32: the bits of maskfilter_batch / maskfilter_stereo_batch on
    clips.astype(float32) / 32768.  out_dtype int16 (the default): that result quantised -- rint(y * 32768), ties to even, saturating at
    -32768 and 32767, NaN -> 0 -- and, with rest=True, rest = clip(x - y_q, -32768, 32767) in integers, so y_q + rest == x wherever the rest
    did not saturate.  -> (B, N[, 2]) of out_dtype; with rest=True (y, rest), views of one (B, 2, N[, 2]) result (which `out`, if given, is).
    The device reads "TF" masks only: "FT" masks are transposed on the host before the upload.  Clips of any other dtype raise ValueError."""
    w = _maskfilter_window(window_function, step_length)
    a = _as_int16_clips(clips, "clips")
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 2):
        raise ValueError(f"clips must be mono, (clips, samples), or interleaved stereo, (clips, sample frames, 2), got shape {a.shape}")
    stereo = a.ndim == 3
    form = _MASKED_STEREO if stereo else _MASKED_PCM_MONO
    dt = _as_pcm_out_dtype(out_dtype if out is None else out.dtype)
    m = np.asarray(masks)
    if np.iscomplexobj(m) or m.dtype.kind not in "biuf":
        raise ValueError(f"masks must be real numbers, got dtype {m.dtype}")
    count = form.batch_count(m) if form.batch_count else None
    n_clips, n = a.shape[:2]
    h = len(w) // 2
    ft = _LAYOUTS[layout] == _lib.LAYOUT_FT
    want = (n_clips,) + form.host_shape(count, (n + h - 1) // h + 1, h + 1, ft)
    if m.shape != want:
        raise ValueError(f"masks must have shape {want} for clips of {n} {form.units} (layout {layout!r}), got {m.shape}")
    shape = (n_clips,) + ((2,) if rest else ()) + a.shape[1:]
    if out is None:
        out = np.empty(shape, dt)
    elif tuple(out.shape) != shape or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError(f"out must be a writeable C-contiguous int16 or float32 array of shape {shape}")
    if out.size:
        plan = maskfilter_plan(w, rest, "TF", device)
        if ft:
            m = m.transpose((0,) + tuple(i + 1 for i in form.ft_axes(count)))
        x, m = np.ascontiguousarray(a), np.ascontiguousarray(m, dtype=np.float32)
        d_in, d_mask, d_out = (DeviceBuffer(b.shape, b.dtype, plan.device) for b in (x, m, out))
        try:
            d_in.upload(x)
            d_mask.upload(m)
            with plan.lock:
                plan.execute_masked_pcm(d_in, d_mask, d_out, n_clips, n, 2 if stereo else 1, count or 1)
                plan.sync()
                d_out.download(out=out)
        finally:
            for b in (d_in, d_mask, d_out):
                b.free()
    return (out[:, 0], out[:, 1]) if rest else out


def mdct_batch(clips, window_function, layout="FT", device=0, f64=False, out=None, row_align=None):
    """(B, N) -> (B, W/2, T) float32 ["FT"] or (B, T, W/2) ["TF"]; f64: float64 arrays and arithmetic."""
    x = _as_clips(clips, dtype=np.float64 if f64 else np.float32)
    plan = _line_grid(mdct_plan(window_function, layout, device, f64=f64), x.shape[1], out,
                      lambda a: mdct_plan(window_function, layout, device, row_align=a, f64=f64), row_align=row_align)
    out = _run_host_into(plan, x.astype(plan.in_dtype, copy=False), x.shape[1], out)
    return out if f64 else out.astype(np.float32, copy=False)


def imdct_batch(coefficients, window_function, layout="FT", device=0, f64=False, out=None, row_align=None):
    """(B, W/2, T) ["FT"] or (B, T, W/2) ["TF"] -> (B, (W/2)(T-1) - 1) float32 (float64 with f64)."""
    c = np.asarray(coefficients)
    if c.dtype != (np.float64 if f64 else np.float32):
        c = c.astype(np.float64 if f64 else np.float32)
    w = _as_window(window_function, any_length=True)
    if c.ndim != 3:
        raise ValueError("coefficients must be 3-D")
    nf, nt = (c.shape[1], c.shape[2]) if _LAYOUTS[layout] == _lib.LAYOUT_FT else (c.shape[2], c.shape[1])
    if 2 * nf != len(w):
        raise ValueError("coefficient rows must equal window_length/2")
    plan = _line_grid(mdct_plan(w, layout, device, inverse=True, f64=f64), nt, None,
                      lambda a: mdct_plan(w, layout, device, inverse=True, row_align=a, f64=f64), frames=nt, row_align=row_align)
    out = _run_host_into(plan, c if plan.row_align > 1 else c.astype(plan.in_dtype, copy=False), nt, out)
    return out if f64 else out.astype(np.float32, copy=False)


def melspectrogram_batch(clips, window_function, step_length, mel_filterbank, layout="FT", device=0, f64=False, out=None):
    """(B, N) -> (B, n_filters, T) float32 (float64 arrays and arithmetic with f64)."""
    x = _as_clips(clips, dtype=np.float64 if f64 else np.float32)   # (validated before any device call)
    plan = mel_plan(window_function, step_length, mel_filterbank, None, layout, device, f64=f64)
    x = x.astype(plan.in_dtype, copy=False)
    out = _run_host_into(plan, x, x.shape[1], out)
    return out if f64 else out.astype(np.float32, copy=False)   # (a long window is computed in float64 whatever f64 says)


def mfcc_batch(clips, window_function, step_length, mel_filterbank, number_coefficients, layout="FT", device=0, f64=False, out=None):
    """(B, N) -> (B, number_coefficients, T) float32 (float64 arrays and arithmetic with f64)."""
    x = _as_clips(clips, dtype=np.float64 if f64 else np.float32)   # (validated before any device call)
    plan = mel_plan(window_function, step_length, mel_filterbank, number_coefficients, layout, device, f64=f64)
    x = x.astype(plan.in_dtype, copy=False)
    out = _run_host_into(plan, x, x.shape[1], out)
    return out if f64 else out.astype(np.float32, copy=False)


def _split_mel_mfcc(both, n_filters, layout):
    """(mel, mfcc) views of the one-pass plan's output: rows 0 .. n_filters - 1 and the rest (the last axis in the frame-major layout)."""
    if _LAYOUTS[layout] == _lib.LAYOUT_FT:
        return both[:, :n_filters], both[:, n_filters:]
    return both[:, :, :n_filters], both[:, :, n_filters:]


def mel_mfcc_batch(clips, window_function, step_length, mel_filterbank, number_coefficients, layout="FT", device=0, f64=False, out=None):
    """zaf.melspectrogram AND zaf.mfcc of the same clips from ONE set of transforms (both start with the same zaf.stft, zaf.py:369 and :436;
    BASELINE config 3): (B, N) -> ((B, n_filters, T), (B, number_coefficients, T)), views of one (B, n_filters + number_coefficients, T)
    array (`out`, when given, is that array); both bit-identical to melspectrogram_batch / mfcc_batch.  Geometries outside the one-pass
    kernel (mel_mfcc_supported: float32, window 2048, <= 128 filters, <= 32 coefficients) run the two plans."""
    x = _as_clips(clips, dtype=np.float64 if f64 else np.float32)
    w = _as_window(window_function, any_length=True)
    n_filters = mel_filterbank.shape[0] if hasattr(mel_filterbank, "shape") else 0
    if not mel_mfcc_supported(len(w), n_filters, int(number_coefficients), f64):
        mel = melspectrogram_batch(x, w, step_length, mel_filterbank, layout, device, f64)
        cep = mfcc_batch(x, w, step_length, mel_filterbank, number_coefficients, layout, device, f64)
        if out is None:
            return mel, cep
        np.copyto(out, np.concatenate([mel, cep], axis=1 if _LAYOUTS[layout] == _lib.LAYOUT_FT else 2), casting="same_kind")
        return _split_mel_mfcc(out, n_filters, layout)
    plan = mel_plan(w, step_length, mel_filterbank, number_coefficients, layout, device, also_mel=True)
    both = _run_host_into(plan, x, x.shape[1], out)
    return _split_mel_mfcc(both, n_filters, layout)


def mel_mfcc_pcm_batch(pcm, window_function, step_length, mel_filterbank, number_coefficients, layout="FT", device=0, out=None):
    """mel_mfcc_batch of integer PCM clips (see stft_pcm_batch): int16 read inside the kernel's own loads."""
    w = _as_window(window_function, any_length=True)
    n_filters = mel_filterbank.shape[0]
    if not mel_mfcc_supported(len(w), n_filters, int(number_coefficients)):
        return mel_mfcc_batch(pcm_to_mono(pcm, device), w, step_length, mel_filterbank, number_coefficients, layout, device, out=out)
    plan = mel_plan(w, step_length, mel_filterbank, number_coefficients, layout, device, also_mel=True)
    return _split_mel_mfcc(plan.run_host_pcm(pcm, out=out), n_filters, layout)


# ======================================================================================
# ragged batches: clips of different lengths in one call (zafx_execute_ragged)
# ======================================================================================
_RAGGED_ALIGN = 32   # elements between clip starts in a packed batch: 128 bytes of float32


def _as_ragged_items(batch, ndim, name, items, noun, rule=None, empty_ok=False, complex_ok=False):
    """A ragged batch -- a sequence of real arrays of rank `ndim` (complex_ok: real or complex ones) -- validated ahead of any device call: ->
    the list of arrays.  `name`, `items` and `noun` are the words of the messages; rule(a): what is wrong with the shape of an item
    ("must ...") or None."""
    if isinstance(batch, np.ndarray) and batch.dtype != object and batch.ndim <= ndim:
        raise ValueError(f"a {name} is a sequence of {items}, not one array")
    try:
        arrays = list(batch)
    except TypeError:
        raise ValueError(f"a {name} is a sequence of {items}") from None
    if not arrays and not empty_ok:
        raise ValueError(f"a {name} needs at least one {noun}")
    for i, c in enumerate(arrays):
        arrays[i] = a = np.asarray(c)
        wrong = None
        if a.ndim != ndim:
            wrong = f"must be {ndim}-D, got {a.ndim}-D"
        elif a.dtype.kind not in ("biufc" if complex_ok else "biuf"):
            wrong = "must be numeric" if complex_ok else "must be real"
        elif rule:
            wrong = rule(a)
        if wrong:
            raise ValueError(f"{noun} {i} of the {name} {wrong}")
    return arrays


def _as_ragged(clips):
    return _as_ragged_items(clips, 1, "ragged batch", "1-D clips", "clip")


def _back_to_back(sizes, align=1):
    """-> (offsets, total): slots of `sizes` elements, each rounded up to a multiple of `align`, laid back to back."""
    slots = (sizes + align - 1) // align * align
    offsets = np.zeros(len(sizes), np.int64)
    offsets[1:] = np.cumsum(slots)[:-1]
    return offsets, int(slots.sum())


def _round_trip(plan, x, n_out, enqueue):
    """x up (an empty one is not copied), enqueue(d_in, d_out) and the wait under the plan's lock, the `n_out` results -- items of x's trailing
    shape; at least one is allocated -- down: -> the one downloaded array.  Both buffers are freed whatever happens."""
    d_in = DeviceBuffer((max(len(x), 1),) + x.shape[1:], x.dtype, plan.device)
    d_out = DeviceBuffer((max(n_out, 1),) + x.shape[1:], plan.out_dtype, plan.device)
    try:
        if len(x):
            d_in.upload(x)
        with plan.lock:
            enqueue(d_in, d_out)
            plan.sync()
            return d_out.download()
    finally:
        d_in.free()
        d_out.free()


def pack_ragged(clips, dtype=np.float32):
    """One contiguous array of a ragged batch: -> (packed, in_offsets, lengths).  Clip i starts at element in_offsets[i], a multiple of 32
    elements (128 bytes of float32), and the gaps between the clips are zeros -- so that the kernels' aligned loads apply whenever the hop is
    even (zafx_execute_ragged)."""
    arrays = _as_ragged(clips)
    lengths = np.array([len(a) for a in arrays], np.int64)
    offsets, total = _back_to_back(lengths, _RAGGED_ALIGN)
    packed = np.zeros(max(total, _RAGGED_ALIGN), dtype)
    for a, o in zip(arrays, offsets.tolist()):
        packed[o:o + len(a)] = a
    return packed, offsets, lengths


def _run_ragged(plan, clips):
    """One ragged batch through `plan`: one upload, one execute_ragged, one download.  -> list of per-clip views of the one result buffer,
    (F, T_i) for the "FT" layout (rows at the plan's pitch), (T_i, F) for "TF"."""
    x, in_offsets, lengths = pack_ragged(clips, plan.in_dtype)
    offs, frames, pitch = plan.ragged_layout(lengths)
    rows = plan.out_dims(0)[0]
    res = _round_trip(plan, x, int(offs[-1]), lambda d_in, d_out: plan.execute_ragged(d_in, in_offsets, lengths, d_out))
    return _ragged_views(plan, res, rows, offs, frames, pitch)


def _ragged_views(plan, res, rows, offs, frames, pitch):
    """The per-clip views of a ragged batch's downloaded result (Plan.ragged_layout)."""
    if plan.layout == _lib.LAYOUT_FT:
        return [res[o:o + rows * p].reshape(rows, p)[:, :t] for o, t, p in zip(offs.tolist(), frames.tolist(), pitch.tolist())]
    return [res[o:o + t * rows].reshape(t, rows) for o, t in zip(offs.tolist(), frames.tolist())]


def _ragged_grid(plan, padded_plan, inverse=False):
    """The plan of a ragged call in the reference layout: rows padded to whole 128-byte lines (as _line_grid), where the native ragged kernels run.
    inverse: the 2-D side is the plan's input."""
    return padded_plan(_line_elements(plan.in_dtype if inverse else plan.out_dtype)) if plan.layout == _lib.LAYOUT_FT else plan


def _as_f32_views(views, plan, f64):
    """A plan the library promoted to float64 (short windows, large filterbanks): the float32 / complex64 result the caller asked for."""
    if f64 or not plan.f64 or not views:
        return views
    return [v.astype(np.complex64 if np.iscomplexobj(v) else np.float32) for v in views]


def stft_ragged(clips, window_function, step_length, layout="FT", device=0, onesided=False, f64=False):
    """stft_batch of clips of different lengths in one call: a sequence of 1-D arrays -> a list of (W, T_i) complex64 arrays ["FT"] or (T_i, W)
    ["TF"] (rows 0..W/2, or |X| / |X|^2 as float32, with `onesided` as in stft_batch; complex128 / float64 with f64), each clip's frames
    T_i as zaf.stft gives them for that clip alone.  The arrays are views of one result buffer.  "FT" with f64 at window 2048, two-sided or
    rows 0..W/2, runs in one launch as the float32 plans do (k_stft_ft8_f64_ragged); |X| / |X|^2 and other windows in float64 run one
    execute per clip."""
    clips = _as_ragged(clips)
    _spectrum_of(onesided)
    plan = stft_plan(window_function, step_length, layout, device, onesided, f64)
    plan = _ragged_grid(plan, lambda a: stft_plan(window_function, step_length, layout, device, onesided, f64, row_align=a))
    return _as_f32_views(_run_ragged(plan, clips), plan, f64)


def mdct_ragged(clips, window_function, layout="FT", device=0, f64=False):
    """mdct_batch of clips of different lengths in one call: a sequence of 1-D arrays -> a list of (W/2, T_i) float32 arrays ["FT"] or
    (T_i, W/2) ["TF"] (float64 arrays and arithmetic with f64), each clip's frames T_i = ceil(N_i / (W/2)) + 1 as zaf.mdct gives them for that
    clip alone (a clip of length 0: one frame of zeros).  The arrays are views of one result buffer.  "FT" / float32 at window 512, 1024 and
    2048 runs in one launch (k_mdct_ft32_ragged), and so does "FT" with f64 at window 2048 (k_mdct_ft16_f64_ragged); an empty list gives an
    empty list."""
    w = _as_window(window_function, any_length=True)
    if len(w) % 2 or len(w) < 4:
        raise ValueError("the MDCT needs an even window_length >= 4")
    _check_f64_window(len(w), bool(f64) or not _f32_window(len(w)))
    _as_row_align(0, layout)   # (an unknown layout fails here)
    if isinstance(clips, (list, tuple)) and not len(clips):
        return []
    clips = _as_ragged(clips)
    plan = mdct_plan(w, layout, device, f64=f64)
    plan = _ragged_grid(plan, lambda a: mdct_plan(w, layout, device, row_align=a, f64=f64))
    return _as_f32_views(_run_ragged(plan, clips), plan, f64)


def _as_ragged_blocks(coefficients, rows, layout):
    """A ragged batch of MDCT coefficient blocks: (rows, T_i) ["FT"] or (T_i, rows) ["TF"]; it may be empty."""
    axis = 0 if _LAYOUTS[layout] == _lib.LAYOUT_FT else 1
    return _as_ragged_items(coefficients, 2, "ragged batch of coefficients", "2-D blocks", "block", empty_ok=True,
                            rule=lambda a: None if a.shape[axis] == rows else f"must have window_length/2 = {rows} coefficient rows, got shape {a.shape}")


def imdct_ragged(coefficients, window_function, layout="FT", device=0, f64=False, lengths=None):
    """imdct_batch of coefficient blocks of different frame counts in one call: a sequence of (W/2, T_i) real arrays ["FT"] or (T_i, W/2)
    ["TF"] -> a list of 1-D float32 arrays (float64 arrays and arithmetic with f64) of max((W/2) (T_i - 1) - 1, 0) samples, as zaf.imdct gives
    them for that block alone; with lengths=[N_i] each is cut to its first N_i samples (the clip mdct_ragged was given).  The arrays are views
    of one result buffer.  One upload, one execute, one download; the views mdct_ragged returns are taken as they lie.  "FT" / float32 at
    window 512, 1024 and 2048 runs in one launch (k_imdct_ragged); an empty list gives an empty list."""
    w = _as_window(window_function, any_length=True)
    if len(w) % 2 or len(w) < 4:
        raise ValueError("the MDCT needs an even window_length >= 4")
    _check_f64_window(len(w), bool(f64) or not _f32_window(len(w)))
    _as_row_align(0, layout)   # (an unknown layout fails here)
    m = len(w) // 2
    blocks = _as_ragged_blocks(coefficients, m, layout)
    ft = _LAYOUTS[layout] == _lib.LAYOUT_FT
    frames = np.array([b.shape[1 if ft else 0] for b in blocks], np.int64)
    return _blocks_ragged(blocks, m, frames, np.maximum(m * (frames - 1) - 1, 0), lengths, ft, f64, "execute_imdct_ragged",
                          lambda a=0: mdct_plan(w, layout, device, inverse=True, row_align=a, f64=f64))


def _blocks_ragged(blocks, rows, frames, out_len, lengths, ft, f64, execute, make_plan):
    """imdct_ragged / istft_ragged behind their own checks: blocks of `rows` rows and frames[i] frames that give out_len[i] samples, through the
    plan make_plan() (make_plan(row_align): the same on a grid of lines) and its method `execute`."""
    if lengths is not None:
        lengths = _as_lengths(lengths)
        if len(lengths) != len(blocks):
            raise ValueError("lengths must have one entry per block")
        for i, (n, o) in enumerate(zip(lengths.tolist(), out_len.tolist())):
            if n > o:
                raise ValueError(f"lengths[{i}] = {n} exceeds the {o} samples block {i} gives")
    if not blocks:
        return []
    plan = _ragged_grid(make_plan(), make_plan, inverse=True)
    # the blocks back to back at the plan's pitch (every block starts on a 128-byte line), the clips' samples on a grid of lines
    a = max(plan.row_align, 1)
    pitch = (frames + a - 1) // a * a if ft else np.full(len(blocks), rows, np.int64)
    elems = rows * pitch if ft else frames * rows
    in_offsets, n_in = _back_to_back(elems)
    out_offsets, n_out = _back_to_back(out_len, _RAGGED_ALIGN)
    packed = np.empty(max(n_in, 1), plan.in_dtype)   # (the pad columns are never used: they stay as they come)
    for b, o, t, p in zip(blocks, in_offsets.tolist(), frames.tolist(), pitch.tolist()):
        if ft:
            packed[o:o + rows * p].reshape(rows, p)[:, :t] = b   # (rows of a view at any pitch: copied row by row)
        else:
            packed[o:o + t * rows].reshape(t, rows)[...] = b
    res = _round_trip(plan, packed, n_out, lambda d_in, d_out: getattr(plan, execute)(d_in, in_offsets, frames, d_out, out_offsets))
    keep = out_len if lengths is None else lengths
    return _as_f32_views([res[o:o + n] for o, n in zip(out_offsets.tolist(), keep.tolist())], plan, f64)


def istft_ragged(spectra, window_function, step_length, layout="FT", device=0, onesided=False, f64=False, lengths=None):
    """istft_batch of spectra of different frame counts in one call: a sequence of (W, T_i) complex arrays ["FT"] -- (W/2 + 1, T_i) with
    onesided -- or their transposes ["TF"] -> a list of 1-D float32 arrays (float64 with f64) of max(T_i H - (W - H), 0) samples, as zaf.istft
    gives them for that spectrum alone; with lengths=[N_i] each is cut to its first N_i samples (the clip stft_ragged was given).  The arrays
    are views of one result buffer.  One upload, one execute, one download; the views stft_ragged returns are taken as they lie.  "FT" /
    float32 at window 256 ... 2048 runs in one launch (k_istft_ragged); an empty list gives an empty list."""
    w, h = _as_window(window_function, any_length=True), _as_step(step_length)
    if h > len(w):
        raise ValueError("step_length must not exceed window_length")
    if onesided not in (False, True):
        raise ValueError("istft takes a complex spectrum: onesided must be False or True")
    _check_f64_window(len(w), bool(f64) or not _f32_window(len(w)))
    _as_row_align(0, layout)   # (an unknown layout fails here)
    ft = _LAYOUTS[layout] == _lib.LAYOUT_FT
    rows = len(w) // 2 + 1 if onesided else len(w)
    axis = 0 if ft else 1
    blocks = _as_ragged_items(spectra, 2, "ragged batch of spectra", "2-D blocks", "block", empty_ok=True, complex_ok=True,
                              rule=lambda a: None if a.shape[axis] == rows else
                              f"must have {'window_length/2 + 1' if onesided else 'window_length'} = {rows} spectrum rows, got shape {a.shape}")
    frames = np.array([b.shape[1 - axis] for b in blocks], np.int64)
    return _blocks_ragged(blocks, rows, frames, np.maximum(frames * h - (len(w) - h), 0), lengths, ft, f64, "execute_istft_ragged",
                          lambda a=0: istft_plan(w, h, layout, device, onesided, f64, row_align=a))


def melspectrogram_ragged(clips, window_function, step_length, mel_filterbank, layout="FT", device=0, f64=False):
    """melspectrogram_batch of clips of different lengths: -> a list of (n_filters, T_i) float32 arrays (float64 with f64).  With f64, "FT" at
    window 2048 and up to 128 filters runs in one launch (k_mel_ft8_f64_ragged), everything else in float64 one execute per clip."""
    clips = _as_ragged(clips)
    plan = mel_plan(window_function, step_length, mel_filterbank, None, layout, device, f64=f64)
    plan = _ragged_grid(plan, lambda a: mel_plan(window_function, step_length, mel_filterbank, None, layout, device, row_align=a, f64=f64))
    return _as_f32_views(_run_ragged(plan, clips), plan, f64)


def mfcc_ragged(clips, window_function, step_length, mel_filterbank, number_coefficients, layout="FT", device=0, f64=False):
    """mfcc_batch of clips of different lengths: -> a list of (number_coefficients, T_i) float32 arrays (float64 with f64).  With f64 -- the
    arithmetic in which the MFCCs of tonal material hold 1e-10 --, "FT" at window 2048 and up to 128 filters runs in one launch
    (k_mel_ft8_f64_ragged), everything else in float64 one execute per clip."""
    clips = _as_ragged(clips)
    plan = mel_plan(window_function, step_length, mel_filterbank, number_coefficients, layout, device, f64=f64)
    plan = _ragged_grid(plan, lambda a: mel_plan(window_function, step_length, mel_filterbank, number_coefficients, layout, device, row_align=a,
                                                 f64=f64))
    return _as_f32_views(_run_ragged(plan, clips), plan, f64)


def mel_mfcc_ragged(clips, window_function, step_length, mel_filterbank, number_coefficients, layout="FT", device=0, f64=False):
    """mel_mfcc_batch of clips of different lengths: -> (list of (n_filters, T_i), list of (number_coefficients, T_i)), from one set of
    transforms where the one-pass kernel takes the geometry (mel_mfcc_supported), else from the two plans -- with f64 always the two: one
    launch each at window 2048 (k_mel_ft8_f64_ragged, as melspectrogram_ragged and mfcc_ragged)."""
    clips = _as_ragged(clips)
    w = _as_window(window_function, any_length=True)
    n_filters = mel_filterbank.shape[0] if hasattr(mel_filterbank, "shape") else 0
    if not mel_mfcc_supported(len(w), n_filters, int(number_coefficients), f64):
        return (melspectrogram_ragged(clips, w, step_length, mel_filterbank, layout, device, f64),
                mfcc_ragged(clips, w, step_length, mel_filterbank, number_coefficients, layout, device, f64))
    plan = mel_plan(w, step_length, mel_filterbank, number_coefficients, layout, device, also_mel=True)
    plan = _ragged_grid(plan, lambda a: mel_plan(w, step_length, mel_filterbank, number_coefficients, layout, device, row_align=a, also_mel=True))
    both = _run_ragged(plan, clips)
    ft = plan.layout == _lib.LAYOUT_FT
    return ([b[:n_filters] if ft else b[:, :n_filters] for b in both], [b[n_filters:] if ft else b[:, n_filters:] for b in both])


# ---- ragged batches of integer PCM (zafx_execute_ragged_pcm) ----------------------------------
_RAGGED_PCM_ALIGN = 64   # sample frames between clip starts in a packed PCM batch: 128 bytes of int16 mono


def _as_ragged_pcm(clips, empty_ok=False):
    """A ragged batch of integer PCM -- a sequence of (N_i,) or (N_i, C) arrays of ONE integer dtype (int16 or int32) and one channel count --
    validated ahead of any device call: -> (list of (N_i, C) arrays, C, dtype, whether every clip came 1-D)."""
    name, items, noun = "ragged PCM batch", "(N,) or (N, C) integer clips", "clip"
    if isinstance(clips, np.ndarray) and clips.dtype != object and clips.ndim <= 1:
        raise ValueError(f"a {name} is a sequence of {items}, not one array")
    try:
        arrays = list(clips)
    except TypeError:
        raise ValueError(f"a {name} is a sequence of {items}") from None
    if not arrays and not empty_ok:
        raise ValueError(f"a {name} needs at least one {noun}")
    flat = True
    for i, c in enumerate(arrays):
        a = np.asarray(c)
        wrong = None
        if a.ndim not in (1, 2):
            wrong = f"must be 1-D or (N, C), got {a.ndim}-D"
        elif a.dtype not in (np.dtype(np.int16), np.dtype(np.int32)):
            wrong = f"must be int16 or int32 (wavread's other dtypes: convert on the host), got {a.dtype}"
        elif a.ndim == 2 and a.shape[1] < 1:
            wrong = f"must have at least one channel, got shape {a.shape}"
        if wrong:
            raise ValueError(f"{noun} {i} of the {name} {wrong}")
        flat = flat and a.ndim == 1
        arrays[i] = a = a[:, None] if a.ndim == 1 else a
        if a.dtype != arrays[0].dtype:
            raise ValueError(f"{noun} {i} of the {name} must be {arrays[0].dtype} as clip 0 (one dtype per batch), got {a.dtype}")
        if a.shape[1] != arrays[0].shape[1]:
            raise ValueError(f"{noun} {i} of the {name} must have {arrays[0].shape[1]} channel(s) as clip 0 (one channel count per batch), got {a.shape[1]}")
    ch, dtype = (arrays[0].shape[1], arrays[0].dtype) if arrays else (1, np.dtype(np.int16))
    return arrays, ch, dtype, flat


def _pack_ragged_pcm(arrays, ch, dtype):
    lengths = np.array([len(a) for a in arrays], np.int64)
    offsets, total = _back_to_back(lengths, _RAGGED_PCM_ALIGN)
    packed = np.zeros((max(total, _RAGGED_PCM_ALIGN), ch), dtype)
    for a, o in zip(arrays, offsets.tolist()):
        packed[o:o + len(a)] = a
    return packed, offsets, lengths


def pack_ragged_pcm(clips):
    """One contiguous array of a ragged batch of integer PCM: a sequence of (N_i,) or (N_i, C) int16 / int32 arrays of one dtype and one channel
    count -> (packed, in_offsets, lengths), offsets and lengths in sample frames; packed is (S,) for 1-D clips, (S, C) interleaved otherwise.
    Clip i starts at sample frame in_offsets[i], a multiple of 64 (128 bytes of int16 mono), and the gaps between the clips are zeros -- so that
    the kernels that read int16 themselves apply whenever the hop is even (zafx_execute_ragged_pcm).  The array is never empty."""
    arrays, ch, dtype, flat = _as_ragged_pcm(clips)
    packed, offsets, lengths = _pack_ragged_pcm(arrays, ch, dtype)
    return (packed[:, 0] if flat else packed), offsets, lengths


def _run_ragged_pcm(make_plan, float_fn, batch):
    """One ragged PCM batch (_as_ragged_pcm's result) through the plan make_plan() -- make_plan(row_align): the same on a grid of lines --: one
    upload of the integers, one execute_ragged_pcm, one download.  -> list of per-clip views of the one result buffer, as _run_ragged.  A plan
    the library runs in float64 (windows outside the float32 kernels) normalises on the device and takes float_fn(clips), as _pcm_batch."""
    arrays, ch, dtype, _ = batch
    plan = make_plan()
    x, in_offsets, lengths = _pack_ragged_pcm(arrays, ch, dtype)
    if plan.f64:
        mono = pcm_to_mono(x[None], plan.device)[0]
        return float_fn([mono[o:o + n] for o, n in zip(in_offsets.tolist(), lengths.tolist())])
    plan = _ragged_grid(plan, make_plan)
    offs, frames, pitch = plan.ragged_layout(lengths)
    res = _round_trip(plan, x.reshape(-1), int(offs[-1]), lambda d_in, d_out: plan.execute_ragged_pcm(d_in, in_offsets, lengths, d_out, ch))
    return _ragged_views(plan, res, plan.out_dims(0)[0], offs, frames, pitch)


def stft_pcm_ragged(clips, window_function, step_length, layout="FT", device=0, onesided=False):
    """stft_ragged of integer PCM clips of different lengths: a sequence of (N_i,) or (N_i, C) int16 / int32 arrays -> the list stft_ragged gives
    for the normalised mono clips (zaf.py:1202 x / 2^(bits-1), zaf.py:65 mean over the channels).  One upload of the integers (2-4 bytes per
    sample and channel), one execute, one download; int16 mono / stereo at window 2048 with an even hop is read by the kernel itself."""
    batch = _as_ragged_pcm(clips)
    _spectrum_of(onesided)
    return _run_ragged_pcm(lambda a=0: stft_plan(window_function, step_length, layout, device, onesided, row_align=a),
                           lambda x: stft_ragged(x, window_function, step_length, layout, device, onesided), batch)


def mdct_pcm_ragged(clips, window_function, layout="FT", device=0):
    """mdct_ragged of integer PCM clips of different lengths (see stft_pcm_ragged); int16 mono / stereo at window 2048 is read by the kernel
    itself when every clip's length is a multiple of 4 sample frames.  An empty list gives an empty list."""
    w = _as_window(window_function, any_length=True)
    if len(w) % 2 or len(w) < 4:
        raise ValueError("the MDCT needs an even window_length >= 4")
    _as_row_align(0, layout)   # (an unknown layout fails here)
    if isinstance(clips, (list, tuple)) and not len(clips):
        return []
    batch = _as_ragged_pcm(clips)
    return _run_ragged_pcm(lambda a=0: mdct_plan(w, layout, device, row_align=a), lambda x: mdct_ragged(x, w, layout, device), batch)


def melspectrogram_pcm_ragged(clips, window_function, step_length, mel_filterbank, layout="FT", device=0):
    """melspectrogram_ragged of integer PCM clips of different lengths (see stft_pcm_ragged)."""
    batch = _as_ragged_pcm(clips)
    return _run_ragged_pcm(lambda a=0: mel_plan(window_function, step_length, mel_filterbank, None, layout, device, row_align=a),
                           lambda x: melspectrogram_ragged(x, window_function, step_length, mel_filterbank, layout, device), batch)


def mfcc_pcm_ragged(clips, window_function, step_length, mel_filterbank, number_coefficients, layout="FT", device=0):
    """mfcc_ragged of integer PCM clips of different lengths (see stft_pcm_ragged)."""
    batch = _as_ragged_pcm(clips)
    return _run_ragged_pcm(lambda a=0: mel_plan(window_function, step_length, mel_filterbank, number_coefficients, layout, device, row_align=a),
                           lambda x: mfcc_ragged(x, window_function, step_length, mel_filterbank, number_coefficients, layout, device), batch)


def mel_mfcc_pcm_ragged(clips, window_function, step_length, mel_filterbank, number_coefficients, layout="FT", device=0):
    """mel_mfcc_ragged of integer PCM clips of different lengths (see stft_pcm_ragged): -> (list of (n_filters, T_i), list of
    (number_coefficients, T_i)), from one set of transforms where the one-pass kernel takes the geometry (mel_mfcc_supported), else from the
    two plans."""
    batch = _as_ragged_pcm(clips)
    w = _as_window(window_function, any_length=True)
    n_filters = mel_filterbank.shape[0] if hasattr(mel_filterbank, "shape") else 0
    if not mel_mfcc_supported(len(w), n_filters, int(number_coefficients), False):
        return (melspectrogram_pcm_ragged(batch[0], w, step_length, mel_filterbank, layout, device),
                mfcc_pcm_ragged(batch[0], w, step_length, mel_filterbank, number_coefficients, layout, device))
    both = _run_ragged_pcm(lambda a=0: mel_plan(w, step_length, mel_filterbank, number_coefficients, layout, device, row_align=a, also_mel=True),
                           None, batch)
    ft = _LAYOUTS[layout] == _lib.LAYOUT_FT
    return ([b[:n_filters] if ft else b[:, :n_filters] for b in both], [b[n_filters:] if ft else b[:, n_filters:] for b in both])


def _as_ragged_stereo(clips):
    return _as_ragged_items(clips, 2, "ragged stereo batch", "(N, 2) clips", "clip",
                            rule=lambda a: None if a.shape[1] == 2 else f"must be stereo, (sample frames, 2), got shape {a.shape}")


def pack_ragged_stereo(clips):
    """One contiguous float32 array of a ragged stereo batch: a sequence of (N_i, 2) real arrays -> (packed (S, 2), in_offsets, lengths), in
    sample frames.  The clips lie back to back without gaps (in_offsets are the running sums of the lengths): k_center pads every clip through
    a buffer descriptor of its own, so a neighbour right behind a clip is never read as its tail."""
    arrays = _as_ragged_stereo(clips)
    lengths = np.array([len(a) for a in arrays], np.int64)
    offsets, total = _back_to_back(lengths)
    packed = np.empty((total, 2), np.float32)
    for a, o in zip(arrays, offsets.tolist()):
        packed[o:o + len(a)] = a
    return packed, offsets, lengths


def centersides_ragged(clips, window_function, step_length=None, sides=True, device=0):
    """centersides_batch of stereo clips of different lengths in one launch: a sequence of (N_i, 2) real arrays -> a list of (center_i, sides_i)
    pairs, or of centers with sides=False, each float32 (N_i, 2) and a view of the one result buffer; every clip's result has the bits
    centersides_batch gives for that clip alone.  One upload, one launch (k_center_ragged), one download.  Window and step_length as in
    centersides_batch."""
    w = _center_window(window_function, step_length)
    x, in_offsets, lengths = pack_ragged_stereo(clips)
    plan = center_plan(w, device, sides)
    blocks = 2 if sides else 1
    out_offsets = blocks * in_offsets
    res = _round_trip(plan, x, blocks * len(x), lambda d_in, d_out: plan.execute_center_ragged(d_in, in_offsets, lengths, d_out, out_offsets))
    if not sides:
        return [res[o:o + n] for o, n in zip(out_offsets.tolist(), lengths.tolist())]
    return [(res[o:o + n], res[o + n:o + 2 * n]) for o, n in zip(out_offsets.tolist(), lengths.tolist())]


def _pack_ragged_masks(form, masks, lengths, window_length, layout, row_align=0):
    """The four pack_ragged_*masks: the masks of a ragged batch, one item per clip of `lengths`, validated and packed as the device reads them
    -> (packed 1-D of the form's mask dtype, mask_offsets of len(lengths) + 1, count).  Masks of a kind the device reads in "TF" only are
    transposed here; the real kind's "FT" masks keep their rows, at the frame count rounded up to row_align."""
    lengths = _as_lengths(lengths)
    ft = _LAYOUTS[layout] == _lib.LAYOUT_FT
    a = max(_as_row_align(row_align, layout), 1)
    masks, count = form.ragged_count_first(masks) if form.ragged_count_first else (masks, None)
    h = int(window_length) // 2
    arrays = _as_ragged_items(masks, len(form.tf_shape(count, 0, 0)), form.batch_words[0], form.batch_words[1](count), "mask", empty_ok=True,
                              complex_ok=form.mask_dtype.kind == "c")
    if len(arrays) != len(lengths):
        raise ValueError(f"masks and lengths must have one entry per clip, got {len(arrays)} masks for {len(lengths)} clips")
    if form.ragged_count:
        count = form.ragged_count(arrays)
    frames = (lengths + h - 1) // h + 1
    pitched = ft and not form.tf_only
    pitch = (frames + a - 1) // a * a if pitched else frames
    offsets = np.zeros(len(lengths) + 1, np.int64)
    offsets[1:] = np.cumsum(form.mask_blocks(count) * pitch * (h + 1))
    packed = np.zeros(max(int(offsets[-1]), 1), form.mask_dtype)
    for i, (m, o, t, p) in enumerate(zip(arrays, offsets.tolist(), frames.tolist(), pitch.tolist())):
        if form.stems_out and m.shape[0] != count:
            raise ValueError(f"mask {i} has {m.shape[0]} stems, mask 0 has {count}: the stem count is one for the batch")
        want = form.host_shape(count, t, h + 1, ft)
        if m.shape != want:
            raise ValueError(f"mask {i} must have shape {want} for clip {i} of {int(lengths[i])} {form.units} (layout {layout!r}), got {m.shape}")
        if pitched:
            packed[o:o + (h + 1) * p].reshape(h + 1, p)[:, :t] = m
        else:
            packed[o:offsets[i + 1]].reshape(form.tf_shape(count, t, h + 1))[...] = m.transpose(form.ft_axes(count)) if ft else m
    return packed, offsets, count


def pack_ragged_masks(masks, lengths, window_length, layout="FT", row_align=0):
    """One contiguous float32 array of a ragged batch's masks: a sequence of real (W/2 + 1, T_i) arrays -- (T_i, W/2 + 1) with layout "TF" --,
    T_i = ceil(lengths[i] / (W/2)) + 1 -> (packed 1-D, mask_offsets of len(lengths) + 1), the layout of Plan.mask_ragged_layout for a plan of
    that window_length, layout and row_align: the masks back to back, "FT" rows at the frame count rounded up to row_align (the pad columns
    are zeros).  A mask of another shape raises ValueError with the clip's index."""
    return _pack_ragged_masks(_MASKED_REAL, masks, lengths, window_length, layout, row_align)[:2]


def maskfilter_ragged(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0):
    """maskfilter_batch of mono clips of different lengths in one launch: a sequence of 1-D real clips and one of real masks, (W/2 + 1, T_i) --
    (T_i, W/2 + 1) with layout "TF" --, T_i = ceil(N_i / (W/2)) + 1 -> a list of float32 (N_i,) arrays, or of (y_i, rest_i) pairs with
    rest=True, each a view of the one result buffer; every clip's result has the bits maskfilter_batch gives for that clip alone.  One upload
    each of clips and masks, one launch (k_maskfilter_ragged), one download.  Window and step_length as in maskfilter_batch."""
    return _maskfilter_ragged(_MASKED_REAL, clips, window_function, masks, step_length, rest, layout, device)


def _maskfilter_ragged(form, clips, window_function, masks, step_length, rest, layout, device):
    """maskfilter_ragged and its stems, complex and stereo forms: the clips packed back to back (the kernel pads every clip through a descriptor
    of its own) and the packed masks up, one launch, the result -- the clips back to back, each with its output blocks -- down, and the
    per-clip views of it."""
    w = _maskfilter_window(window_function, step_length)
    if form.unit_bytes == 8:
        x, in_offsets, lengths = pack_ragged_stereo(clips)
    else:
        arrays = _as_ragged_items(clips, 1, "ragged batch", "1-D clips", "clip")
        lengths = np.array([len(a) for a in arrays], np.int64)
        in_offsets, total = _back_to_back(lengths)
        x = np.empty(max(total, 1), np.float32)
        for a, o in zip(arrays, in_offsets.tolist()):
            x[o:o + len(a)] = a
    m, mask_offsets, count = _pack_ragged_masks(form, masks, lengths, len(w), layout)
    plan = maskfilter_plan(w, rest, "TF" if form.tf_only else layout, device)
    blocks = form.out_blocks(count, rest)
    out_offsets = blocks * in_offsets
    tail = () if count is None else (count,)
    d_mask = DeviceBuffer(m.shape, m.dtype, plan.device)
    try:
        d_mask.upload(m)
        res = _round_trip(plan, x, blocks * len(x), lambda d_in, d_out: plan._execute_masked_ragged(form, d_in, in_offsets, lengths, d_mask, mask_offsets, d_out,
                                                                                                   out_offsets, *tail))
    finally:
        d_mask.free()
    out = [res[o:o + n].reshape((blocks, n // blocks) + res.shape[1:]) for o, n in zip(out_offsets.tolist(), (blocks * lengths).tolist())]
    if form.stems_out:
        return [(b[:count], b[count]) for b in out] if rest else out
    return [(b[0], b[1]) for b in out] if rest else [b[0] for b in out]


def pack_ragged_complex_masks(masks, lengths, window_length, layout="FT"):
    """One contiguous complex64 array of a ragged batch's complex masks: a sequence of real or complex (W/2 + 1, T_i) arrays -- (T_i, W/2 + 1)
    with layout "TF" --, T_i = ceil(lengths[i] / (W/2)) + 1 -> (packed 1-D complex64, mask_offsets of len(lengths) + 1 in complex64 elements),
    the layout of Plan.mask_ragged_layout for a "TF" plan of that window_length: clip i's mask as (T_i, W/2 + 1) compact, the clips back to
    back.  The device reads "TF" masks only: "FT" masks are transposed here, on the host.  A mask of another shape raises ValueError with
    the clip's index."""
    return _pack_ragged_masks(_MASKED_COMPLEX, masks, lengths, window_length, layout)[:2]


def maskfilter_complex_ragged(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0):
    """maskfilter_complex_batch of mono clips of different lengths in one launch: a sequence of 1-D real clips and one of real or complex masks,
    (W/2 + 1, T_i) -- (T_i, W/2 + 1) with layout "TF" --, T_i = ceil(N_i / (W/2)) + 1 -> a list of float32 (N_i,) arrays, or of (y_i, rest_i)
    pairs with rest=True, each a view of the one result buffer; every clip's result has the bits maskfilter_complex_batch gives for that clip
    alone.  One upload each of clips and masks, one launch (k_maskfilter_complex_ragged), one download.  "FT" masks are transposed on the
    host (pack_ragged_complex_masks).  Window and step_length as in maskfilter_batch."""
    return _maskfilter_ragged(_MASKED_COMPLEX, clips, window_function, masks, step_length, rest, layout, device)


def pack_ragged_stereo_masks(masks, lengths, window_length, layout="FT"):
    """One contiguous float32 array of a ragged stereo batch's masks: a sequence of real arrays, all (W/2 + 1, T_i) -- one mask for both
    channels; (T_i, W/2 + 1) with layout "TF" -- or all (2, W/2 + 1, T_i) -- one per channel; (T_i, 2, W/2 + 1) with "TF" --,
    T_i = ceil(lengths[i] / (W/2)) + 1 -> (packed 1-D, mask_offsets of len(lengths) + 1, mask_channels), the layout of Plan.stereo_ragged_layout:
    clip i's masks as (T_i, mask_channels, W/2 + 1) compact, the clips back to back.  The device reads "TF" masks only: "FT" masks are
    transposed here, on the host.  A mask of another shape than the first one's kind raises ValueError with the clip's index."""
    return _pack_ragged_masks(_MASKED_STEREO, masks, lengths, window_length, layout)


def maskfilter_stereo_ragged(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0):
    """maskfilter_stereo_batch of stereo clips of different lengths in one launch: a sequence of (N_i, 2) real clips and one of real masks, all
    for both channels, (W/2 + 1, T_i) -- (T_i, W/2 + 1) with layout "TF" --, or all per channel, (2, W/2 + 1, T_i) -- (T_i, 2, W/2 + 1) --,
    T_i = ceil(N_i / (W/2)) + 1 -> a list of float32 (N_i, 2) arrays, or of (y_i, rest_i) pairs with rest=True, each a view of the one result
    buffer; every clip's result has the bits maskfilter_stereo_batch gives for that clip alone.  One upload each of clips and masks, one
    launch (k_maskfilter_stereo_ragged), one download.  "FT" masks are transposed on the host (pack_ragged_stereo_masks).  Window and
    step_length as in maskfilter_stereo_batch."""
    return _maskfilter_ragged(_MASKED_STEREO, clips, window_function, masks, step_length, rest, layout, device)


def maskfilter_pcm_ragged(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0, out_dtype=np.int16):
    """maskfilter_pcm_batch of 16-bit PCM clips of different lengths in one launch: a sequence of int16 clips, all 1-D (mono) or all (N_i, 2)
    (interleaved stereo), and one of real masks as maskfilter_ragged / maskfilter_stereo_ragged take them -> a list of (N_i[, 2]) arrays of
    out_dtype (int16 or float32), or of (y_i, rest_i) pairs with rest=True, each a view of the one result buffer; every clip's result has
    the bits maskfilter_pcm_batch gives for that clip alone.  One upload each of clips (as integers) and masks, one launch
    (k_maskfilter_pcm_ragged / k_maskfilter_stereo_pcm_ragged), one download.  Clips of any other dtype raise ValueError."""
    w = _maskfilter_window(window_function, step_length)
    dt = _as_pcm_out_dtype(out_dtype)
    try:
        arrays = [np.asarray(c) for c in clips] if not (isinstance(clips, np.ndarray) and clips.dtype != object) else None
    except TypeError:
        arrays = None
    if arrays is None:
        raise ValueError("a ragged PCM batch is a sequence of int16 clips, 1-D or (N, 2), not one array")
    if not arrays:
        raise ValueError("a ragged PCM batch needs at least one clip")
    stereo = arrays[0].ndim == 2
    for i, c in enumerate(arrays):
        _as_int16_clips(c, f"clip {i} of the ragged PCM batch")
        if c.ndim != (2 if stereo else 1) or (stereo and c.shape[1] != 2):
            raise ValueError(f"clip {i} of the ragged PCM batch must be {'(sample frames, 2)' if stereo else '1-D'} as clip 0 is, got shape {c.shape}")
    form = _MASKED_STEREO if stereo else _MASKED_PCM_MONO
    lengths = np.array([len(c) for c in arrays], np.int64)
    in_offsets, total = _back_to_back(lengths)
    x = np.zeros((max(total, 1),) + ((2,) if stereo else ()), np.int16)
    for c, o in zip(arrays, in_offsets.tolist()):
        x[o:o + len(c)] = c
    m, mask_offsets, count = _pack_ragged_masks(form, masks, lengths, len(w), layout)
    plan = maskfilter_plan(w, rest, "TF", device)
    blocks = 2 if rest else 1
    out_offsets = blocks * in_offsets
    res = np.empty((max(blocks * total, 1),) + x.shape[1:], dt)
    d_in, d_mask, d_out = (DeviceBuffer(b.shape, b.dtype, plan.device) for b in (x, m, res))
    try:
        d_in.upload(x)
        d_mask.upload(m)
        with plan.lock:
            plan.execute_masked_pcm_ragged(d_in, in_offsets, lengths, d_mask, mask_offsets, d_out, out_offsets, 2 if stereo else 1, count or 1)
            plan.sync()
            d_out.download(out=res)
    finally:
        for b in (d_in, d_mask, d_out):
            b.free()
    out = [res[o:o + blocks * n].reshape((blocks, n) + res.shape[1:]) for o, n in zip(out_offsets.tolist(), lengths.tolist())]
    return [(b[0], b[1]) for b in out] if rest else [b[0] for b in out]


def pack_ragged_stems_masks(masks, lengths, window_length, layout="FT"):
    """One contiguous float32 array of a ragged stems batch's masks: a sequence of real (S, W/2 + 1, T_i) arrays -- (S, T_i, W/2 + 1) with
    layout "TF" --, T_i = ceil(lengths[i] / (W/2)) + 1, S the same for every clip -> (packed 1-D, mask_offsets of len(lengths) + 1), the layout
    of Plan.stems_ragged_layout: clip i's masks back to back as (S, T_i, W/2 + 1), the clips back to back.  The device reads "TF" masks only:
    "FT" masks are transposed here, on the host, as maskfilter_stems_batch does.  A mask of another shape, or a stem count that differs from
    the first clip's, raises ValueError with the clip's index."""
    return _pack_ragged_masks(_MASKED_STEMS, masks, lengths, window_length, layout)[:2]


def maskfilter_stems_ragged(clips, window_function, masks, step_length=None, rest=False, layout="FT", device=0):
    """maskfilter_stems_batch of mono clips of different lengths in one launch: a sequence of 1-D real clips and one of real masks,
    (S, W/2 + 1, T_i) -- (S, T_i, W/2 + 1) with layout "TF" --, S in 1 .. 8 the same for every clip, T_i = ceil(N_i / (W/2)) + 1 -> a list of
    float32 (S, N_i) arrays, or of (stems_i, rest_i) pairs with rest=True, rest_i = ((x - y_0) - y_1) - ... in float32, each a view of the
    one result buffer; every clip's result has the bits maskfilter_stems_batch gives for that clip alone.  One upload each of clips and
    masks, one launch (k_maskfilter_stems_ragged), one download.  "FT" masks are transposed on the host (pack_ragged_stems_masks).  Window and
    step_length as in maskfilter_batch."""
    return _maskfilter_ragged(_MASKED_STEMS, clips, window_function, masks, step_length, rest, layout, device)


def cqtspectrogram_batch(clips, sampling_frequency, time_resolution, cqt_kernel, layout="FT", device=0, f64=False, out=None):
    """(B, N) -> (B, n_bins, T) float32 (float64 arrays and arithmetic with f64)."""
    x = _as_clips(clips, dtype=np.float64 if f64 else np.float32)   # (validated before any device call)
    plan = cqt_plan(sampling_frequency, time_resolution, cqt_kernel, None, layout, device, f64=f64)
    x = x.astype(plan.in_dtype, copy=False)
    out = _run_host_into(plan, x, x.shape[1], out)
    return out if f64 else out.astype(np.float32, copy=False)   # (a long kernel is computed in float64 whatever f64 says)


def cqtchromagram_batch(clips, sampling_frequency, time_resolution, octave_resolution, cqt_kernel, layout="FT", device=0, f64=False, out=None):
    """(B, N) -> (B, octave_resolution, T) float32 (float64 arrays and arithmetic with f64)."""
    x = _as_clips(clips, dtype=np.float64 if f64 else np.float32)   # (validated before any device call)
    plan = cqt_plan(sampling_frequency, time_resolution, cqt_kernel, int(octave_resolution), layout, device, f64=f64)
    x = x.astype(plan.in_dtype, copy=False)
    out = _run_host_into(plan, x, x.shape[1], out)
    return out if f64 else out.astype(np.float32, copy=False)


def _pcm_device_mono(plan, pcm):
    """Upload integer PCM (clips, frames[, channels]) and return the normalised mono f32 DeviceBuffer."""
    pcm = np.ascontiguousarray(pcm)
    if pcm.dtype not in (np.dtype(np.int16), np.dtype(np.int32)):
        raise ValueError("PCM ingest takes int16 or int32 samples (wavread's other dtypes: convert on the host)")
    if pcm.ndim == 2:
        pcm = pcm[:, :, None]
    if pcm.ndim != 3:
        raise ValueError("pcm must be (clips, frames) or (clips, frames, channels)")
    b, n, ch = pcm.shape
    d_pcm = DeviceBuffer.from_host(pcm, plan.device)
    d_x = DeviceBuffer((b, n), np.float32, plan.device)
    plan.pcm_to_float(d_pcm, d_x, b, n, ch)
    return d_pcm, d_x


def _pcm_batch(plan, batch_fn, pcm, out):
    """A *_pcm_batch call: the chunked three-stream pipeline with integer uploads (Plan.run_host_pcm); plans the library runs in
    float64 (windows outside the float32 kernels) normalise on the device and take the general path, `out` included."""
    if plan.f64:
        return batch_fn(pcm_to_mono(pcm, plan.device), out)
    return plan.run_host_pcm(pcm, out=out)


def stft_pcm_batch(pcm, window_function, step_length, layout="FT", device=0, onesided=False, out=None):
    """STFT of integer PCM clips (clips, frames[, channels]): wavread's x / 2^(bits-1) and the channel mean
    (zaf.py:1202, :65) run on the device in front of the transform; only 2-4 B per sample and channel cross PCIe."""
    plan = stft_plan(window_function, step_length, layout, device, onesided)
    return _pcm_batch(plan, lambda x, o: stft_batch(x, window_function, step_length, layout, device, onesided, out=o), pcm, out)


def mdct_pcm_batch(pcm, window_function, layout="FT", device=0, out=None):
    """mdct_batch of integer PCM clips (see stft_pcm_batch)."""
    plan = mdct_plan(window_function, layout, device)
    return _pcm_batch(plan, lambda x, o: mdct_batch(x, window_function, layout, device, out=o), pcm, out)


def melspectrogram_pcm_batch(pcm, window_function, step_length, mel_filterbank, layout="FT", device=0, out=None):
    """melspectrogram_batch of integer PCM clips (see stft_pcm_batch): 2 bytes per sample up, 4 n_filters / hop down."""
    plan = mel_plan(window_function, step_length, mel_filterbank, None, layout, device)
    return _pcm_batch(plan, lambda x, o: melspectrogram_batch(x, window_function, step_length, mel_filterbank, layout, device, out=o), pcm, out)


def mfcc_pcm_batch(pcm, window_function, step_length, mel_filterbank, number_coefficients, layout="FT", device=0, out=None):
    """mfcc_batch of integer PCM clips (see stft_pcm_batch)."""
    plan = mel_plan(window_function, step_length, mel_filterbank, number_coefficients, layout, device)
    return _pcm_batch(plan, lambda x, o: mfcc_batch(x, window_function, step_length, mel_filterbank, number_coefficients, layout, device, out=o), pcm, out)


def cqtspectrogram_pcm_batch(pcm, sampling_frequency, time_resolution, cqt_kernel, layout="FT", device=0, out=None):
    """cqtspectrogram_batch of integer PCM clips (see stft_pcm_batch)."""
    plan = cqt_plan(sampling_frequency, time_resolution, cqt_kernel, None, layout, device)
    return _pcm_batch(plan, lambda x, o: cqtspectrogram_batch(x, sampling_frequency, time_resolution, cqt_kernel, layout, device, out=o), pcm, out)


def cqtchromagram_pcm_batch(pcm, sampling_frequency, time_resolution, octave_resolution, cqt_kernel, layout="FT", device=0, out=None):
    """cqtchromagram_batch of integer PCM clips (see stft_pcm_batch)."""
    plan = cqt_plan(sampling_frequency, time_resolution, cqt_kernel, int(octave_resolution), layout, device)
    return _pcm_batch(plan, lambda x, o: cqtchromagram_batch(x, sampling_frequency, time_resolution, octave_resolution, cqt_kernel, layout, device, out=o), pcm, out)


def pcm_to_mono(pcm, device=0):
    """(clips, frames[, channels]) int16/int32 -> (clips, frames) float32: mean over channels of x / 2^(bits-1)."""
    plan = stft_plan(constants.hamming(64), 32, "FT", device)   # any plan provides the stream
    with plan.lock:
        d_pcm, d_x = _pcm_device_mono(plan, pcm)
        try:
            plan.sync()
            return d_x.download()
        finally:
            d_pcm.free()
            d_x.free()


def dct_fft_length(length, kind, sine):
    """M, the complex FFT length zafx_dct.hip runs for a dct / dst of this length and type -- or None when the length is
    outside that kernel (M must be a power of two in [32, 8192]): N/2 for types 2-4, N-1 (dct) / N+1 (dst) for type 1."""
    n = int(length)
    m = (n + 1 if sine else n - 1) if kind == 1 else (n // 2 if n % 2 == 0 else 0)
    return m if 32 <= m <= 8192 and m & (m - 1) == 0 else None


DCT_CHIRP_MAX = 8192   # longest vector of the chirp-z form (its convolution of 2^ceil(log2(2N - 1)) <= 16384 points lives in LDS)


def dct_plan(length, kind, sine=False, device=0):
    """Plan of the orthonormal dct (sine=False) / dst of type `kind` of vectors of `length` samples (zaf.py:703-839, :842-981).
    Lengths with N/2 (type 1: N -/+ 1) a power of two in [32, 8192] run ONE M-point complex transform per vector (k_dct, instead of the
    reference's 2N-2 ... 8N-point one); every other length from 2 to 8192 runs on the Bluestein machinery -- types 2-4 of a length 4 j as the
    same maps around an N/2-point convolution (k_dct_bsh: two transforms of 2^ceil(log2(N - 1)) points), the rest as a chirp-z sum over all N
    points (k_dct_bs32: two of 2^ceil(log2(2N - 1))) -- O(N log N) for every length the reference takes."""
    n = int(length)
    if dct_fft_length(n, kind, sine) is None and not 2 <= n <= DCT_CHIRP_MAX:
        raise ValueError("dct / dst plans take lengths 2 ... 8192, and longer ones whose N/2 (type 1: N-1 / N+1) is a power of two up to 8192")
    return _cached(("dct_fft", n, int(kind), bool(sine), device),
                   lambda: Plan(_lib.DCT, device, window_length=n, transform_type=int(kind), transform_sine=bool(sine)))


def _transform_batch(vectors, matrix_fn, kind, device, out=None):
    x = np.ascontiguousarray(vectors, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("vectors must be 2-D (batch, length) with length >= 1")
    n = x.shape[1]
    if kind not in (1, 2, 3, 4):
        raise ValueError("type must be 1, 2, 3 or 4")
    sine = matrix_fn is constants.dst_matrix
    if dct_fft_length(n, kind, sine) is not None or 2 <= n <= DCT_CHIRP_MAX:   # O(N log N): on the FFT core, as the reference computes it
        return dct_plan(n, kind, sine, device).run_host(x, n, out=out)
    # what is left -- one sample, or 8192 < N <= 16384 off the power-of-two grid (a convolution of 32768 points does not fit LDS) --: the
    # transform as a dense matrix on the matrix cores, O(N^2) arithmetic and an N x N table, so bounded
    if n > 16384:
        raise ValueError("dct / dst lengths above 16384 are not supported (above 8192: N/2, or N-1 / N+1 for type 1, must be a power of two)")

    def make():   # the N x N matrix (O(N^2) trigonometry, 8 N^2 bytes) is built once per (transform, type, N, device)
        m = np.ascontiguousarray(matrix_fn(n, kind), dtype=np.float64)
        p = Plan(_lib.LINEAR, device, window_length=m.shape[1], n_filters=m.shape[0])
        p.set_matrix(m)
        return p
    plan = _cached((matrix_fn.__name__, int(kind), n, device), make)
    return plan.run_host(x, n, out=out)


def dct_batch(vectors, dct_type, device=0, out=None):
    """(B, N) -> (B, N) float32: orthonormal DCT of type 1-4 of every row (zaf.dct per row)."""
    return _transform_batch(vectors, constants.dct_matrix, dct_type, device, out)


def dst_batch(vectors, dst_type, device=0, out=None):
    """(B, N) -> (B, N) float32: orthonormal DST of type 1-4 of every row (zaf.dst per row)."""
    return _transform_batch(vectors, constants.dst_matrix, dst_type, device, out)


def dct(audio_signal, dct_type):
    """Drop-in for zaf.dct (zaf.py:703): (N,) -> (N,) float64, type 1, 2, 3 or 4."""
    x = np.asarray(audio_signal)
    if x.ndim != 1:
        raise ValueError("audio_signal must be 1-D; use dct_batch for (batch, length)")
    return dct_batch(x[None, :], dct_type)[0].astype(np.float64)


def dst(audio_signal, dst_type):
    """Drop-in for zaf.dst (zaf.py:842): (N,) -> (N,) float64, type 1, 2, 3 or 4."""
    x = np.asarray(audio_signal)
    if x.ndim != 1:
        raise ValueError("audio_signal must be 1-D; use dst_batch for (batch, length)")
    return dst_batch(x[None, :], dst_type)[0].astype(np.float64)


# ======================================================================================
# drop-in API: the zaf.* signatures (1 clip, float64 / complex128 results)
# ======================================================================================
def stft(audio_signal, window_function, step_length):
    """Drop-in for zaf.stft (zaf.py:45): (N,) -> (W, T) complex128, two-sided."""
    f64 = _PRECISION["value"] == "f64"
    x = _as_signal(audio_signal, np.float64 if f64 else np.float32)
    return stft_batch(x, window_function, step_length, f64=f64)[0].astype(np.complex128)


def istft(audio_stft, window_function, step_length):
    """Drop-in for zaf.istft (zaf.py:144): (W, T) -> (T*H - (W-H),) float64."""
    s = np.asarray(audio_stft)
    if s.ndim != 2:
        raise ValueError("audio_stft must be 2-D (window_length, number_times)")
    return istft_batch(s[None], window_function, step_length, f64=_PRECISION["value"] == "f64")[0].astype(np.float64)


def centersides(audio_signal, window_function, step_length):
    """The example of zaf.istft's docstring (zaf.py:155-198) in one call: (N, 2) stereo -> (center_signal, sides_signal), float64 (N, 2)
    each; step_length must be window_length / 2 (see centersides_batch, also for the mask's one departure from the reference)."""
    a = np.asarray(audio_signal)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"audio_signal must be stereo, (sample frames, 2), got shape {a.shape}")
    center, sides = centersides_batch(a[None], window_function, step_length)
    return center[0].astype(np.float64), sides[0].astype(np.float64)


def maskfilter(audio_signal, window_function, step_length, mask):
    """zaf.istft(np.concatenate((mask, mask[-2:0:-1])) * zaf.stft(audio_signal, window_function, step_length), window_function,
    step_length)[0:N] (zaf.py:185-195) in one call: a 1-D signal and a real (W/2 + 1, T) mask -> float64 (N,); step_length must be
    window_length / 2 (see maskfilter_batch)."""
    a, m = np.asarray(audio_signal), np.asarray(mask)
    if a.ndim != 1:
        raise ValueError(f"audio_signal must be 1-D, got shape {a.shape}")
    if m.ndim != 2:
        raise ValueError(f"mask must be 2-D (window_length / 2 + 1, number_times), got shape {m.shape}")
    return maskfilter_batch(a[None], window_function, m[None], step_length)[0].astype(np.float64)


def maskfilter_complex(audio_signal, window_function, step_length, mask):
    """zaf.istft(np.concatenate((mask, np.conj(mask[-2:0:-1]))) * zaf.stft(audio_signal, window_function, step_length), window_function,
    step_length)[0:N] in one call: a 1-D signal and a complex (or real) (W/2 + 1, T) mask -> float64 (N,); step_length must be
    window_length / 2 (see maskfilter_complex_batch)."""
    a, m = np.asarray(audio_signal), np.asarray(mask)
    if a.ndim != 1:
        raise ValueError(f"audio_signal must be 1-D, got shape {a.shape}")
    if m.ndim != 2:
        raise ValueError(f"mask must be 2-D (window_length / 2 + 1, number_times), got shape {m.shape}")
    return maskfilter_complex_batch(a[None], window_function, m[None], step_length)[0].astype(np.float64)


def maskfilter_stereo(audio_signal, window_function, step_length, mask):
    """The center / sides example's filter (zaf.py:176-198) with masks of the caller's in one call: an (N, 2) stereo signal and a real mask
    (W/2 + 1, T) for both channels, or (2, W/2 + 1, T), one per channel -> float64 (N, 2), column c being zaf.istft(np.concatenate((m_c,
    m_c[-2:0:-1])) * zaf.stft(audio_signal[:, c], ...), ...)[0:N]; step_length must be window_length / 2 (see maskfilter_stereo_batch)."""
    a, m = np.asarray(audio_signal), np.asarray(mask)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"audio_signal must be stereo, (sample frames, 2), got shape {a.shape}")
    _stereo_mask_channels(m.ndim, 2, "mask")
    return maskfilter_stereo_batch(a[None], window_function, m[None], step_length)[0].astype(np.float64)


def maskfilter_pcm(audio_pcm, window_function, step_length, mask, out_dtype=np.int16):
    """maskfilter / maskfilter_stereo on 16-bit PCM as zaf.wavread finds it on disk, in one call: an int16 signal, (N,) mono or (N, 2) stereo,
    and a real mask (W/2 + 1, T) -- for a stereo signal also (2, W/2 + 1, T), one per channel -> (N[, 2]) of out_dtype: int16 (the default;
    what zaf.wavwrite takes) or float32 (the filtered signal at the level of audio_pcm / 32768).  step_length must be window_length / 2;
    any dtype other than int16 raises ValueError (see maskfilter_pcm_batch)."""
    a, m = _as_int16_clips(audio_pcm, "audio_pcm"), np.asarray(mask)
    if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] != 2):
        raise ValueError(f"audio_pcm must be mono, (samples,), or interleaved stereo, (sample frames, 2), got shape {a.shape}")
    if a.ndim == 2:
        _stereo_mask_channels(m.ndim, 2, "mask")
    elif m.ndim != 2:
        raise ValueError(f"mask must be 2-D, (W/2 + 1, frames), got {m.ndim} dimensions")
    return maskfilter_pcm_batch(a[None], window_function, m[None], step_length, out_dtype=out_dtype)[0]


def maskfilter_stems(audio_signal, window_function, step_length, masks):
    """maskfilter for S masks of one signal in one call: a 1-D signal and real masks (S, W/2 + 1, T), S in 1 .. 8 -> float64 (S, N), row s
    being maskfilter(audio_signal, window_function, step_length, masks[s]); the signal is transformed once (see maskfilter_stems_batch)."""
    a, m = np.asarray(audio_signal), np.asarray(masks)
    if a.ndim != 1:
        raise ValueError(f"audio_signal must be 1-D, got shape {a.shape}")
    if m.ndim != 3:
        raise ValueError(f"masks must be 3-D (stems, window_length / 2 + 1, number_times), got shape {m.shape}")
    return maskfilter_stems_batch(a[None], window_function, m[None], step_length)[0].astype(np.float64)


def melspectrogram(audio_signal, window_function, step_length, mel_filterbank):
    """Drop-in for zaf.melspectrogram (zaf.py:324): (N,) -> (n_filters, T) float64."""
    f64 = _PRECISION["value"] == "f64"
    x = _as_signal(audio_signal, np.float64 if f64 else np.float32)
    return melspectrogram_batch(x, window_function, step_length, mel_filterbank, f64=f64)[0].astype(np.float64)


def mfcc(audio_signal, window_function, step_length, mel_filterbank, number_coefficients):
    """Drop-in for zaf.mfcc (zaf.py:378): (N,) -> (number_coefficients, T) float64."""
    f64 = _PRECISION["value"] == "f64"
    x = _as_signal(audio_signal, np.float64 if f64 else np.float32)
    return mfcc_batch(x, window_function, step_length, mel_filterbank, number_coefficients, f64=f64)[0].astype(np.float64)


def cqtspectrogram(audio_signal, sampling_frequency, time_resolution, cqt_kernel):
    """Drop-in for zaf.cqtspectrogram (zaf.py:562): (N,) -> (n_bins, T) float64."""
    f64 = _PRECISION["value"] == "f64"
    x = _as_signal(audio_signal, np.float64 if f64 else np.float32)
    return cqtspectrogram_batch(x, sampling_frequency, time_resolution, cqt_kernel, f64=f64)[0].astype(np.float64)


def cqtchromagram(audio_signal, sampling_frequency, time_resolution, octave_resolution, cqt_kernel):
    """Drop-in for zaf.cqtchromagram (zaf.py:638): (N,) -> (octave_resolution, T) float64."""
    f64 = _PRECISION["value"] == "f64"
    x = _as_signal(audio_signal, np.float64 if f64 else np.float32)
    return cqtchromagram_batch(x, sampling_frequency, time_resolution, octave_resolution, cqt_kernel, f64=f64)[0].astype(np.float64)


def mdct(audio_signal, window_function):
    """Drop-in for zaf.mdct (zaf.py:984): (N,) -> (W/2, T) float64."""
    f64 = _PRECISION["value"] == "f64"
    x = _as_signal(audio_signal, np.float64 if f64 else np.float32)
    return mdct_batch(x, window_function, f64=f64)[0].astype(np.float64)


def imdct(audio_mdct, window_function):
    """Drop-in for zaf.imdct (zaf.py:1078): (W/2, T) -> ((W/2)(T-1) - 1,) float64."""
    c = np.asarray(audio_mdct)
    if c.ndim != 2:
        raise ValueError("audio_mdct must be 2-D (number_frequencies, number_times)")
    return imdct_batch(c[None], window_function, f64=_PRECISION["value"] == "f64")[0].astype(np.float64)
