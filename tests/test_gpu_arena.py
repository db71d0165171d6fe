"""Every kernel route on device arrays that start OFF the allocation grid (-m gpu; the harness is tests/arena.py).

A fresh allocation sits on a 256-byte boundary, so of the launchers' address tests (`uintptr_t` in zaf-python_amd/csrc) only one outcome
ever ran under the rest of the suite.  Here the arrays are views at delta bytes into NaN-filled arenas; every case runs the offset pairs
(delta, delta), (128, delta), (delta, 128) for delta in 4, 8, 16, 64 and (128, 128) -- the fresh allocation's own route, now between guards --
and checks, per pair: nothing written outside the array, every element written (row padding: none), the float64 oracle's numbers within
the project's bounds (TOL_FFT 1e-5, TOL_FB 1e-4, float64 1e-12, mfcc 1e-10; |X|^2 2 TOL_FFT as everywhere in tests/test_gpu_parity.py:
d|X|^2 = 2 |X| d|X|), clips 0 and 2 bit-identical once clip 1 is all NaN, and the kernel the launcher's code says that pair reaches.

Shapes: 3 clips; T = two whole tiles of the route ("on": the rows are whole 128-byte lines) and the same clip one sample longer
("off": T + 1, a partial third tile, rows off the grid, odd clip length, the clips' own bases alternating in phase).  The CQT's frame count
is floor(n / step): its "off" clip is one step and one sample longer.

Route table -- geometry: (delta_in, delta_out) -> kernel, as the launchers read (d_i / d_o: the offsets mod the named power of two):

  STFT float32, reference layout (zafx_stft.hip run_stft)
    W 2048, 256 two- / one-sided     rows off the grid or d_o % 128 != 0, d_o % 8 == 0 -> k_stft_ft16c (b0 = d_o / 8 != 0 for 8, 16, 64);
                                     d_o % 8 != 0 (4) -> k_stft_ft16 (its 8-byte stores unaligned); on the grid at 128 -> k_stft_ft16 (claimed tiles)
    W 1024 two-sided                 k_stft_ft16c at every d_o % 8 == 0 (the carry form always), k_stft_ft16 at 4
    W 2048 |X|, |X|^2                k_mel2 (launch_spec2; rows as 16- / 8- / 4-byte pieces by d_o % 16, % 8: zafx_mel.hip:837)
    W 1024, 256 |X|, |X|^2           k_stft_ft16
    W 4096                           on the grid at d_o % 128 == 0 -> k_stft_ft16b; else d_o % 8 == 0 (one-sided: and 2 hop >= W) -> k_stft_ft16bc;
                                     else k_stft; |X|, |X|^2 -> k_stft_ft16b
    W 8192                           two-sided off the grid or d_o % 128 != 0 -> k_stft, everything else k_stft_ft16q
    W 64 -> k_stft, W 1000 -> k_stft_bs32; hop 777: as W 2048 with `aligned` false whatever d_i is
    frame-major layout               W 256 ... 2048 -> k_stft_tf, W 64, 4096, 8192 -> k_stft, W 1000 -> k_stft_bs32
    d_i % 8 (zafx_stft.hip:2646, :2608, zafx_mel.hip:1180) selects the ALIGNED template of the same kernel: no name changes
  ISTFT float32 (run_istft)
    W 2048, 1024 -> k_istft_ft16 (16-byte gathers at d_i % 8 == 0, 8-byte ones at 4; y_base_aligned by d_o % 8)
    W 2048 / 100 -> k_ifft_frames_bs32 (frames + gather)
    W 4096 / 2048                    d_i % 8 == 0 and d_o % 16 == 0 -> k_istft_ft16d; d_i % 8 == 0 -> k_istft_ft16b; else k_istft
    W 4096 / 1024                    d_i % 8 == 0 -> k_istft_ft16b, else k_istft
    W 8192 / 4096                    d_i % 8 == 0 and d_o % 16 == 0 -> k_istft_ft8q, else k_istft
    frame-major: W 256 ... 2048 -> k_istft_ft16, others k_istft
  MDCT / IMDCT float32 (zafx_mdct.hip run_mdct, run_imdct)
    W 2048, 512 -> k_mdct_ft32 (carry form inside it at d_i % 16 == 0, n % 4 == 0 and rows off the 64-byte grid or d_o % 64 != 0: b0 = d_o / 4)
    W 4096                           n % 4 == 0 and d_i % 16 == 0: k_mdct_ft32b on the grid at d_o % 64 == 0, else k_mdct_ft32bc; otherwise k_mdct
    W 8192 -> k_mdct_ft32q; W 64 -> k_mdct; W 1000 -> k_mdct_bs32; frame-major: W 512, 2048 -> k_mdct_ft32, else k_mdct
    IMDCT W 8192                     pitch % 4 == 0 and d_i % 16 == 0 -> k_imdct_q, else k_imdct; W 1000 -> k_imdct_frames_bs32; others k_imdct
  mel / mfcc / both (either layout): W 2048 -> k_mel2; W 4096 -> k_mel_ft16b; 300 filters -> a spectrum kernel, then k_melfb (what last_kernel names);
    W 1024 / 64 filters -> k_mel; d_i % 8 (zafx_mel.hip:1263, zafx_stft.hip:2608) selects the ALIGNED template
  CQT / chromagram -> k_cqt (d_i % 8: ALIGNED template)
  DCT / DST: N 64, 1024 types 2-4 -> k_dct; N 100 types 2-4 -> k_dct_bsh; type 1 of these lengths and N 441 -> k_dct_bs32
  LINEAR -> k_linear; 16384 x 32 on 64 clips: d_i % 16 == 0 -> k_linear128 (zafx_linear.hip:168), else k_linear.  That case is ONE K tile, whole
    row tiles and one clip tile: the tile edges of both kernels, k_linear128's double buffer and scalar stores (rows % 4 != 0, or d_o % 16 != 0)
    run under the same harness in tests/test_gpu_linear.py (cases: tests/linear_cases.py), where the two kernels must also agree bit for bit
  int16 PCM: direct (the plan's own kernel reads int16) at d_i % 8 == 0 (MDCT: % 16), staged through k_pcm_to_float otherwise: same names
  float64: STFT d_i % 16 == 0 and d_o % 16 == 0 -> k_stft_ft8_f64 else k_stft_f64; mel / mfcc, CQT: d_i % 16 == 0 -> k_mel_ft8_f64 / k_cqt_ft_f64 else
    k_mel_f64 / k_cqt_f64; ISTFT, MDCT, IMDCT W 2048 -> k_istft_ft8_f64, k_mdct_ft16_f64, k_imdct_ft16_f64 at every offset; W 256: the generic kernels
  center / sides -> k_center (no address test in zafx_center.hip)
  ragged: d_o % 128 == 0 -> one launch (k_stft_ft16_ragged / k_mel2_ragged / k_mdct_ft32_ragged), d_o = 8 -> "per-clip ..."
    k_mdct_ft32_ragged (zafx_capi.cpp zafx_execute_ragged): the 16-byte-load form at d_i % 16 == 0 with every offset and length a multiple of 4,
    the 4-byte form otherwise -- aligned lengths on a base 4 or 8 bytes off included: one name
    k_imdct_ragged (zafx_execute_imdct_ragged): every d_i, d_o on the 4-byte grid at pitches that are multiples of 4 (16-byte buffer loads at any
    4-byte alignment, pair stores that need their dword only); k_center_ragged (zafx_execute_center_ragged): every d_i, d_o on the 4-byte grid
    (no address test: 8-byte pieces at the clip's base plus multiples of 8)
  The entry points that take free offsets (all three ragged ones on the input side; center and IMDCT on the output side too) run with gaps of
  1, 3 and 5 elements between the clips: poison on the input side, arena.gap_block on the output side.

Not reachable through the entry points: the `d_matrix` / `d_window` / `win` tests (zafx_linear.hip:168, zafx_mdct.hip:70, :1847 -- plan-owned
allocations, always on the grid); `x % 4`, `out % 4`, `coefs % 4` (zafx_stft.hip:2603, :2670-:2688, zafx_mdct.hip:1081, :1573, :1585-:1586: a float32
array off the 4-byte grid is not a float32 array: include/zafx.h)."""
import functools

import numpy as np
import pytest
import scipy.sparse

import arena
from conftest import GOLDEN, relerr, synth_clip
from oracle import zaf_oracle as orc

pytestmark = pytest.mark.gpu

TOL_FFT = 1e-5
TOL_FB = 1e-4
TOL_F64 = 1e-12
TOL_F64_MFCC = 1e-10

OTHER_FORM = 2e-6   # the same frames through another form of a kernel (carry / plain, streamed / not): tests/test_gpu_parity.py _run_padded

DELTAS = (4, 8, 16, 64)
DELTAS_F64 = (8, 16)


def pairs(deltas):
    out = [(128, 128)]
    for d in deltas:
        out += [(d, d), (128, d), (d, 128)]
    return out


_DEVICE_ERROR = []


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    z.set_row_padding("compact")
    yield z
    z.set_row_padding("auto")


class Prep:
    """One case, ready to run: the input, the output's blocks (with the oracle's results), the launch and the kernel each pair must reach."""

    def __init__(self, plan, x, n_in, blocks, tol, want, err=relerr, launch=None, poisoned=None, exact=None, exact_kernel=None, n_clips=None, out_dtype=None,
                 middle=1):
        self.plan, self.x, self.n_in, self.blocks, self.tol, self.want, self.err, self.middle = plan, x, n_in, blocks, tol, want, err, middle
        self.poisoned, self.exact, self.exact_kernel, self.out_dtype = poisoned, exact, exact_kernel, np.dtype(out_dtype or plan.out_dtype)
        n_clips = len(x) if n_clips is None else n_clips
        self.launch = launch or (lambda d_in, d_out: (plan.execute(d_in, d_out, n_clips, n_in), plan.sync()))
        out_bytes = max(int(np.prod(b.shape, dtype=np.int64)) for b in blocks) * self.out_dtype.itemsize
        self.guard = arena.guard_bytes(-(-x.nbytes // n_clips), out_bytes)


def run(zafx, prep, which):
    """Every offset pair of one case; the failures of all pairs in one report.  A device error ends the module: nothing more is launched."""
    if _DEVICE_ERROR:
        pytest.fail(f"not run: an earlier case met a device error ({_DEVICE_ERROR[0]})")
    failures, seen = [], []
    for pair in which:
        try:
            arena.run_case(zafx, prep.x, prep.out_dtype, prep.blocks, prep.guard, pair, prep.launch, prep.tol, prep.err,
                           poisoned=prep.poisoned, exact=prep.exact, exact_tol=0.0 if prep.want(*pair) == prep.exact_kernel else OTHER_FORM,
                           middle=prep.middle)
        except AssertionError as exc:
            failures.append(f"{pair}: {exc}")
        except zafx.ZafxError as exc:
            _DEVICE_ERROR.append(f"{pair}: {exc}")
            raise
        got, want = prep.plan.last_kernel, prep.want(*pair)
        seen.append(f"{pair}: {got}")
        if not (want is None or (got.startswith(want[:-1]) if want.endswith("*") else got == want)):   # (None: the call launches no plan kernel)
            failures.append(f"{pair}: ran {got}, the launcher's code says {want}")
    print("; ".join(seen))
    assert not failures, "\n".join(failures)


def clips(seed, n, dtype=np.float32, count=3):
    return np.stack([synth_clip(seed, c, n) for c in range(count)]).astype(dtype)


def window(zafx, w, mdct=False):
    return zafx.kaiser_bessel_derived(w) if mdct else zafx.hamming(w)


def as_tf(ref):
    return [np.ascontiguousarray(r.T) for r in ref]


def blocks_2d(plan, n_clips, n_in, ref):
    """Blocks of a forward plan's (clips, F, pitch) or (clips, T, F) array."""
    return arena.uniform_blocks(plan.out_shape(n_clips, n_in), plan.out_dims(n_in)[1] if plan.layout == _FT else None, ref)


_FT = 0   # zafx.LAYOUT_FT (asserted where a plan is made)


def of_kind(spec, kind, w):
    if kind is False:
        return spec
    one = spec[:, :w // 2 + 1]
    return one if kind is True else np.abs(one) if kind == "magnitude" else np.abs(one) ** 2


# ------------------------------------------------------------------------------------------------ STFT
@functools.lru_cache(maxsize=32)
def stft_ref(w, hop, n, f64):
    x = clips(w + hop, n, np.float64 if f64 else np.float32)
    return x, orc.stft_batch(x.astype(np.float64), orc.hamming_periodic(w), hop)


def stft_want(w, hop, kind, layout, T, f64=False):
    spec = {False: 0, True: 1, "magnitude": 2, "power": 3}[kind]
    pow2 = w & (w - 1) == 0

    def want(di, do):
        if f64:
            if not pow2:
                return "k_stft_bs_f64"
            return "k_stft_ft8_f64" if w == 2048 and layout == "FT" and spec < 2 and di % 16 == 0 and do % 16 == 0 else "k_stft_f64"
        if not pow2:
            return "k_stft_bs32"
        if layout == "TF":
            return "k_stft_tf" if 256 <= w <= 2048 else "k_stft"
        whole = T % 16 == 0 and do % 128 == 0
        if w == 2048 and spec >= 2:
            return "k_mel2"
        if w == 4096:
            if spec < 2 and not whole and (spec == 0 or 2 * hop >= w) and do % 8 == 0:
                return "k_stft_ft16bc"
            return "k_stft_ft16b" if spec >= 2 or whole else "k_stft"
        if w == 8192:
            return "k_stft_ft16q" if spec != 0 or whole else "k_stft"
        if w < 256:
            return "k_stft"
        if spec < 2 and ((spec == 0 and w == 1024) or not whole) and do % 8 == 0:
            return "k_stft_ft16c"
        return "k_stft_ft16"
    return want


STFT_GEOMETRIES = [(2048, 1024), (1024, 512), (256, 64), (4096, 2048), (8192, 4096), (64, 32), (1000, 250), (2048, 777)]


def stft_prep(zafx, w, hop, kind, layout, grid, f64=False, tile=16):
    n = (2 * tile - 1) * hop + (grid == "off")
    x, ref = stft_ref(w, hop, n, f64)
    plan = zafx.stft_plan(window(zafx, w), hop, layout=layout, onesided=kind, f64=f64)
    assert plan.f64 == f64 and zafx.LAYOUT_FT == _FT
    T = plan.out_dims(n)[1]
    assert T == 2 * tile + (grid == "off") == ref.shape[2]
    r = list(of_kind(ref, kind, w))
    tol = TOL_F64 if f64 else 2 * TOL_FFT if kind == "power" else TOL_FFT
    return Prep(plan, x, n, blocks_2d(plan, 3, n, as_tf(r) if layout == "TF" else r), tol, stft_want(w, hop, kind, layout, T, f64))


@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("layout", ["FT", "TF"])
@pytest.mark.parametrize("kind", [False, True, "magnitude", "power"], ids=["two", "one", "mag", "pow"])
@pytest.mark.parametrize("w,hop", STFT_GEOMETRIES)
def test_stft(zafx, w, hop, kind, layout, grid):
    run(zafx, stft_prep(zafx, w, hop, kind, layout, grid), pairs(DELTAS))


# ------------------------------------------------------------------------------------------------ ISTFT
@functools.lru_cache(maxsize=32)
def istft_ref(w, hop, T, one, f64):
    """The spectra (two-sided: with a non-Hermitian perturbation, the reference takes real(ifft(.)), zaf.py:223) rounded to the plan's input
    dtype, and the oracle's inverse of exactly those numbers."""
    x = clips(3 * w + hop, (T - 1) * hop, np.float64)
    win = orc.hamming_periodic(w)
    spec = orc.stft_batch(x, win, hop)
    assert spec.shape[2] == T
    if one:
        spec = spec[:, :w // 2 + 1]
    else:
        rng = np.random.default_rng(9)
        spec = spec + 0.05 * (rng.standard_normal(spec.shape) + 1j * rng.standard_normal(spec.shape))
    spec = spec.astype(np.complex128 if f64 else np.complex64)
    full = spec.astype(np.complex128)
    if one:
        full = np.concatenate([full, np.conj(full[:, -2:0:-1])], axis=1)
    return spec, [orc.istft(s, win, hop) for s in full]


def istft_want(w, hop, layout, pitch, f64=False):
    pow2 = w & (w - 1) == 0

    def want(di, do):
        if f64:
            return "k_istft_ft8_f64" if w == 2048 and layout == "FT" and 2 * hop >= w else "k_ifft_frames_f64"
        if not pow2 or -(-w // hop) - 1 >= (16 if w <= 2048 else 8 if w == 4096 else 4):
            return "k_ifft_frames_bs32"
        if layout == "TF":
            return "k_istft_ft16" if 256 <= w <= 2048 else "k_istft"
        if w == 4096:
            if hop == 2048 and di % 8 == 0 and do % 16 == 0:
                return "k_istft_ft16d"
            return "k_istft_ft16b" if hop % 4 == 0 and 512 <= hop and di % 8 == 0 else "k_istft"
        if w == 8192:
            return "k_istft_ft8q" if hop == 4096 and di % 8 == 0 and do % 16 == 0 else "k_istft"
        return "k_istft_ft16" if w >= 256 else "k_istft"
    return want


ISTFT_GEOMETRIES = [(2048, 1024), (2048, 512), (4096, 2048), (4096, 1024), (8192, 4096), (2048, 100)]


def istft_prep(zafx, w, hop, one, layout, grid, row_align=0, f64=False, tile=16):
    T = 2 * tile + (grid == "off")
    spec, ref = istft_ref(w, hop, T, one, f64)
    plan = zafx.istft_plan(window(zafx, w), hop, layout=layout, onesided=one, row_align=row_align, f64=f64)
    assert plan.f64 == f64
    pitch = plan.row_pitch(T)
    if layout == "TF":
        x = np.ascontiguousarray(spec.transpose(0, 2, 1))
    else:
        x = np.full(spec.shape[:2] + (pitch,), np.nan, dtype=spec.dtype)   # (row padding of the input: NaN, which must not reach the output)
        x[:, :, :T] = spec
    return Prep(plan, x, T, arena.uniform_blocks(plan.out_shape(3, T), None, ref), TOL_F64 if f64 else TOL_FFT, istft_want(w, hop, layout, pitch, f64))


@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("layout", ["FT", "TF"])
@pytest.mark.parametrize("one", [False, True], ids=["two", "one"])
@pytest.mark.parametrize("w,hop", ISTFT_GEOMETRIES)
def test_istft(zafx, w, hop, one, layout, grid):
    run(zafx, istft_prep(zafx, w, hop, one, layout, grid), pairs(DELTAS))


def test_istft_padded_rows(zafx):
    """row_align = 16: T = 33 frames in rows of 48, the 15 padding elements of every input row NaN."""
    run(zafx, istft_prep(zafx, 2048, 1024, False, "FT", "off", row_align=16), pairs(DELTAS))


# ------------------------------------------------------------------------------------------------ MDCT / IMDCT
@functools.lru_cache(maxsize=32)
def mdct_ref(w, n, f64):
    x = clips(w + 1, n, np.float64 if f64 else np.float32)
    return x, orc.mdct_batch(x.astype(np.float64), orc.kbd_window(w))


def mdct_want(w, layout, n, T, pitch, f64=False):
    pow2 = w & (w - 1) == 0

    def want(di, do):
        if f64:
            return "k_mdct_ft16_f64" if w == 2048 and layout == "FT" else "k_mdct_f64"
        if not pow2:
            return "k_mdct_bs32"
        if w in (512, 2048):
            return "k_mdct_ft32"
        if layout == "TF" or w < 256:
            return "k_mdct"
        if w == 4096:
            if n % 4 or di % 16:
                return "k_mdct"
            return "k_mdct_ft32bc" if pitch % 16 or do % 64 else "k_mdct_ft32b"
        return "k_mdct_ft32q"
    return want


MDCT_WINDOWS = [2048, 4096, 8192, 512, 64, 1000]


def mdct_prep(zafx, w, layout, grid, row_align=0, f64=False, tile=32):
    n = (2 * tile - 1) * (w // 2) + (grid == "off")
    x, ref = mdct_ref(w, n, f64)
    plan = zafx.mdct_plan(window(zafx, w, True), layout=layout, row_align=row_align, f64=f64)
    assert plan.f64 == f64 and zafx.LAYOUT_FT == _FT
    T = plan.out_dims(n)[1]
    assert T == 2 * tile + (grid == "off") == ref.shape[2]
    r = list(ref)
    return Prep(plan, x, n, blocks_2d(plan, 3, n, as_tf(r) if layout == "TF" else r), TOL_F64 if f64 else TOL_FFT,
                mdct_want(w, layout, n, T, plan.row_pitch(n), f64))


@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("layout,row_align", [("FT", 0), ("FT", 32), ("TF", 0)])
@pytest.mark.parametrize("w", MDCT_WINDOWS)
def test_mdct(zafx, w, layout, row_align, grid):
    run(zafx, mdct_prep(zafx, w, layout, grid, row_align), pairs(DELTAS))


@pytest.mark.parametrize("w", [2048, 4096, 512])
def test_mdct_padded_rows_odd_frames(zafx, w):
    """row_align = 32 with n a multiple of 4 and T = 39, odd: rows of 64 with 25 padding elements.  On an output base off the 64-byte grid the
    launchers take the carry forms (inside k_mdct_ft32; k_mdct_ft32bc at W = 4096), whose pair store of frames (38, 39) used to reach the first
    padding element: test_mdct's "on" grid has an even T and its "off" grid a length off the 4-sample grid, which takes other forms."""
    m = w // 2
    n = 37 * m + 4
    x, ref = mdct_ref(w, n, False)
    plan = zafx.mdct_plan(window(zafx, w, True), row_align=32)
    T, pitch = plan.out_dims(n)[1], plan.row_pitch(n)
    assert (T, pitch) == (39, 64) and ref.shape[2] == T and n % 4 == 0
    run(zafx, Prep(plan, x, n, blocks_2d(plan, 3, n, list(ref)), TOL_FFT, mdct_want(w, "FT", n, T, pitch)), pairs(DELTAS))


@functools.lru_cache(maxsize=32)
def imdct_ref(w, T, f64):
    x = clips(w + 2, (T - 1) * (w // 2), np.float64)
    win = orc.kbd_window(w)
    coefs = orc.mdct_batch(x, win).astype(np.float64 if f64 else np.float32)
    assert coefs.shape[2] == T
    return coefs, [orc.imdct(c.astype(np.float64), win) for c in coefs]


def imdct_want(w, layout, pitch, f64=False):
    def want(di, do):
        if f64:
            return "k_imdct_ft16_f64" if w == 2048 and layout == "FT" else "k_imdct_frames_f64"
        if w & (w - 1):
            return "k_imdct_frames_bs32"
        return "k_imdct_q" if w == 8192 and layout == "FT" and pitch % 4 == 0 and di % 16 == 0 else "k_imdct"
    return want


def imdct_prep(zafx, w, layout, grid, row_align=0, f64=False, tile=32):
    T = 2 * tile + (grid == "off")
    coefs, ref = imdct_ref(w, T, f64)
    plan = zafx.mdct_plan(window(zafx, w, True), layout=layout, inverse=True, row_align=row_align, f64=f64)
    assert plan.f64 == f64
    pitch = plan.row_pitch(T)
    if layout == "TF":
        x = np.ascontiguousarray(coefs.transpose(0, 2, 1))
    else:
        x = np.full(coefs.shape[:2] + (pitch,), np.nan, dtype=coefs.dtype)
        x[:, :, :T] = coefs
    return Prep(plan, x, T, arena.uniform_blocks(plan.out_shape(3, T), None, ref), TOL_F64 if f64 else TOL_FFT, imdct_want(w, layout, pitch, f64))


@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("layout,row_align", [("FT", 0), ("FT", 32), ("TF", 0)])
@pytest.mark.parametrize("w", MDCT_WINDOWS)
def test_imdct(zafx, w, layout, row_align, grid):
    run(zafx, imdct_prep(zafx, w, layout, grid, row_align), pairs(DELTAS))


# ------------------------------------------------------------------------------------------------ mel / mfcc / both
MEL_GEOMETRIES = [(2048, 1024, 44100, 128, 20), (4096, 2048, 44100, 128, 20), (2048, 1024, 44100, 300, 20), (1024, 256, 22050, 64, 13)]


@functools.lru_cache(maxsize=32)
def mel_ref(w, hop, fs, nmel, ncoef, n, f64):
    x = clips(w + nmel, n, np.float64 if f64 else np.float32)
    win, fb = orc.hamming_periodic(w), orc.melfilterbank(fs, w, nmel)
    mel = [orc.melspectrogram(c.astype(np.float64), win, hop, fb) for c in x]
    cep = [orc.mfcc(c.astype(np.float64), win, hop, fb, ncoef) for c in x]
    return x, mel, cep


def mel_want(w, nmel, what, layout, f64=False):
    """zafx_capi.cpp's mel route: W 2048 up to 256 filters -> k_mel2 (either layout), W 4096 -> k_mel_ft16b, more than 256 filters -> a spectrum
    kernel + k_melfb, other windows -> k_mel."""
    def want(di, do):
        if f64:
            return "k_mel_ft8_f64" if w == 2048 and layout == "FT" and di % 16 == 0 else "k_mel_f64"
        if nmel > 256:
            return "k_melfb"
        return "k_mel2" if w == 2048 else "k_mel_ft16b" if w == 4096 else "k_mel"
    return want


def mel_prep(zafx, w, hop, fs, nmel, ncoef, what, layout, grid, f64=False, tile=16):
    n = (2 * tile - 1) * hop + (grid == "off")
    x, mel, cep = mel_ref(w, hop, fs, nmel, ncoef, n, f64)
    fb = zafx.melfilterbank(fs, w, nmel)
    plan = zafx.mel_plan(window(zafx, w), hop, fb, None if what == "mel" else ncoef, layout=layout, f64=f64, also_mel=what == "both")
    assert plan.f64 == f64 and zafx.LAYOUT_FT == _FT
    ref = {"mel": mel, "mfcc": cep}.get(what) or [np.concatenate([m, c]) for m, c in zip(mel, cep)]
    tol = (TOL_F64 if what == "mel" else TOL_F64_MFCC) if f64 else TOL_FB
    return Prep(plan, x, n, blocks_2d(plan, 3, n, as_tf(ref) if layout == "TF" else ref), tol, mel_want(w, nmel, what, layout, f64))


@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("layout", ["FT", "TF"])
@pytest.mark.parametrize("w,hop,fs,nmel,ncoef,what", [g + (what,) for g in MEL_GEOMETRIES for what in ("mel", "mfcc", "both")
                                                      if what != "both" or (g[0] == 2048 and g[3] <= 128)])   # (the one-pass plan: W 2048, up to 128 filters)
def test_mel(zafx, w, hop, fs, nmel, ncoef, what, layout, grid):
    run(zafx, mel_prep(zafx, w, hop, fs, nmel, ncoef, what, layout, grid), pairs(DELTAS))


# ------------------------------------------------------------------------------------------------ CQT / chromagram
@functools.lru_cache(maxsize=2)
def cqt_kernel(which):
    if which == "tiny":
        g = np.load(f"{GOLDEN}/tiny.npz")
        return 4000, 50, 12, scipy.sparse.csr_matrix(g["ck_dense"])
    return 44100, 25, 24, orc.cqtkernel(44100, 24, 55, 3520)


@functools.lru_cache(maxsize=32)
def cqt_ref(which, n, f64):
    fs, tr, res, ck = cqt_kernel(which)
    x = clips(len(which) + 70, n, np.float64 if f64 else np.float32)
    spec = [orc.cqtspectrogram(c.astype(np.float64), fs, tr, ck) for c in x]
    return x, spec, [orc.cqtchromagram(c.astype(np.float64), fs, tr, res, ck) for c in x]


def cqt_prep(zafx, which, chroma, layout, grid, f64=False):
    fs, tr, res, ck = cqt_kernel(which)
    step = round(fs / tr)
    n = 32 * step + (step + 1) * (grid == "off")
    x, spec, chrom = cqt_ref(which, n, f64)
    plan = zafx.cqt_plan(fs, tr, ck, res if chroma else None, layout=layout, f64=f64)
    assert plan.f64 == f64 and plan.out_dims(n)[1] == 32 + (grid == "off") and zafx.LAYOUT_FT == _FT
    ref = chrom if chroma else spec

    def want(di, do):
        if f64:
            return "k_cqt_ft_f64" if di % 16 == 0 else "k_cqt_f64"
        return "k_cqt"
    return Prep(plan, x, n, blocks_2d(plan, 3, n, as_tf(ref) if layout == "TF" else ref), TOL_F64 if f64 else TOL_FB, want)


@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("layout", ["FT", "TF"])
@pytest.mark.parametrize("chroma", [False, True], ids=["cqt", "chroma"])
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_cqt(zafx, which, chroma, layout, grid):
    run(zafx, cqt_prep(zafx, which, chroma, layout, grid), pairs(DELTAS))


# ------------------------------------------------------------------------------------------------ DCT / DST, LINEAR
@pytest.mark.parametrize("sine", [False, True], ids=["dct", "dst"])
@pytest.mark.parametrize("t", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [64, 1024, 100, 441])
def test_dct_dst(zafx, n, t, sine):
    x = clips(n + t, n)
    ref = [(orc.dst if sine else orc.dct)(c.astype(np.float64), t) for c in x]
    plan = zafx.dct_plan(n, t, sine)
    name = "k_dct" if zafx.dct_fft_length(n, t, sine) is not None else "k_dct_bsh" if n % 4 == 0 and t > 1 else "k_dct_bs32"
    run(zafx, Prep(plan, x, n, arena.uniform_blocks((3, n), None, ref), TOL_FFT, lambda di, do: name), pairs(DELTAS))


@pytest.mark.parametrize("rows,cols,count", [(40, 256, 3), (41, 100, 3), (16384, 32, 64)])
def test_linear(zafx, rows, cols, count):
    """y = M x per clip; 16384 x 32 on 64 clips is the smallest problem the launcher hands to k_linear128 (rows x clips >= 2^20)."""
    m = np.random.default_rng([rows, cols]).standard_normal((rows, cols)).astype(np.float32)
    x = clips(rows, cols, count=count)
    ref = list(x.astype(np.float64) @ m.astype(np.float64).T)
    plan = zafx.linear_plan(m)
    big = rows * count >= 128 * 128 * 64 and cols % 32 == 0
    run(zafx, Prep(plan, x, cols, arena.uniform_blocks((count, rows), None, ref), TOL_FFT, lambda di, do: "k_linear128" if big and di % 16 == 0 else "k_linear"),
        pairs(DELTAS))


# ------------------------------------------------------------------------------------------------ integer PCM
PCM_PAIRS = [(128, 128), (2, 128), (4, 128), (8, 128), (16, 128), (2, 8), (16, 8), (128, 4)]


def pcm_input(n, channels):
    rng = np.random.default_rng([83, channels, n])
    pcm = rng.integers(-32768, 32767, size=(3, n, channels), endpoint=True).astype(np.int16)
    pcm[0, :7], pcm[0, 7:14] = -32768, 32767
    return pcm, (pcm.astype(np.float64) / 32768.0).mean(axis=2)


def on_plain_allocation(zafx, plan, pcm, call):
    d_pcm = zafx.DeviceBuffer.from_host(pcm)
    d_out = zafx.DeviceBuffer(plan.out_shape(3, pcm.shape[1]), plan.out_dtype)
    call(d_pcm, d_out)
    out = d_out.download()
    d_pcm.free(), d_out.free()
    return out


@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("kind", ["mel", "stft", "mdct", "float"])
def test_pcm(zafx, kind, channels, grid):
    """int16 PCM at 2-, 4-, 8- and 16-byte offsets into execute_pcm (mel, STFT, MDCT at W 2048) and pcm_to_float: the oracle's numbers of
    x / 2^15 averaged over the channels (zaf.py:1202, :65), and what the same call gives on a plain allocation -- bit for bit where the offsets
    select the kernel that ran there, within 2e-6 where they select its other form (k_stft_ft16 / k_stft_ft16c).  The arena around
    the samples holds -32768; the poisoned clip too."""
    tile = 32 if kind == "mdct" else 16
    n = (2 * tile - 1) * 1024 + (grid == "off")
    pcm, x64 = pcm_input(n, channels)
    if kind == "mel":
        fb = zafx.melfilterbank(44100, 2048, 128)
        plan, tol = zafx.mel_plan(zafx.hamming(2048), 1024, fb), TOL_FB
        ref = [orc.melspectrogram(c, orc.hamming_periodic(2048), 1024, orc.melfilterbank(44100, 2048, 128)) for c in x64]
        name = lambda di, do: "k_mel2"
    elif kind == "stft":
        plan, tol = zafx.stft_plan(zafx.hamming(2048), 1024), TOL_FFT
        ref = list(orc.stft_batch(x64, orc.hamming_periodic(2048), 1024))
        name = stft_want(2048, 1024, False, "FT", ref[0].shape[1])
    elif kind == "mdct":
        plan, tol = zafx.mdct_plan(zafx.kaiser_bessel_derived(2048)), TOL_FFT
        ref = list(orc.mdct_batch(x64, orc.kbd_window(2048)))
        name = lambda di, do: "k_mdct_ft32"
    else:
        plan, tol, ref = zafx.stft_plan(zafx.hamming(2048), 1024), TOL_FFT, list(x64)
    if kind == "float":
        call = lambda d_in, d_out: (plan.pcm_to_float(d_in, d_out, 3, n, channels), plan.sync())
        blocks = arena.uniform_blocks((3, n), None, ref)
        d_pcm, d_x = zafx.DeviceBuffer.from_host(pcm), zafx.DeviceBuffer((3, n), np.float32)
        call(d_pcm, d_x)
        exact, exact_kernel = d_x.download(), None
        d_pcm.free(), d_x.free()
        name = lambda di, do: None
    else:
        call = lambda d_in, d_out: (plan.execute_pcm(d_in, d_out, 3, n, channels), plan.sync())
        blocks = blocks_2d(plan, 3, n, ref)
        exact, exact_kernel = on_plain_allocation(zafx, plan, pcm, call), plan.last_kernel
    run(zafx, Prep(plan, pcm, n, blocks, tol, name, launch=call, exact=exact, exact_kernel=exact_kernel, out_dtype=np.float32 if kind == "float" else None), PCM_PAIRS)


# ------------------------------------------------------------------------------------------------ float64
@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("w,hop", [(2048, 1024), (256, 64)])
@pytest.mark.parametrize("route", ["stft", "stft_one", "istft", "istft_one", "mdct", "imdct", "mel", "mfcc"])
def test_f64(zafx, route, w, hop, grid):
    which = pairs(DELTAS_F64)
    if route.startswith("stft"):
        prep = stft_prep(zafx, w, hop, route.endswith("one"), "FT", grid, f64=True, tile=8)
    elif route.startswith("istft"):
        prep = istft_prep(zafx, w, hop, route.endswith("one"), "FT", grid, f64=True, tile=8)
    elif route == "mdct":
        prep = mdct_prep(zafx, w, "FT", grid, f64=True, tile=16)
    elif route == "imdct":
        prep = imdct_prep(zafx, w, "FT", grid, f64=True, tile=16)
    else:
        prep = mel_prep(zafx, w, hop, 44100 if w == 2048 else 8000, 128 if w == 2048 else 26, 20 if w == 2048 else 12, route, "FT", grid, f64=True, tile=8)
    run(zafx, prep, which)


@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("chroma", [False, True], ids=["cqt", "chroma"])
def test_f64_cqt(zafx, chroma, grid):
    run(zafx, cqt_prep(zafx, "full", chroma, "FT", grid, f64=True), pairs(DELTAS_F64))


# ------------------------------------------------------------------------------------------------ center / sides
@pytest.mark.parametrize("grid", ["on", "off"])
@pytest.mark.parametrize("sides", [True, False], ids=["center_sides", "center"])
@pytest.mark.parametrize("w", [1024, 256])
def test_center(zafx, w, sides, grid):
    from test_gpu_center import oracle_center, stereo
    f, h = zafx.center_tile_frames(w), w // 2
    n = 2 * f * h + 64 + (grid == "off")
    x = np.stack([stereo(w + c, n) for c in range(3)])
    win = zafx.hamming(w)
    center = [oracle_center(c, win) for c in x]
    ref = [np.stack([c, xc.astype(np.float64) - c]) for c, xc in zip(center, x)] if sides else center
    plan = zafx.center_plan(win, sides=sides)

    def err(val, r):
        """The bounds of tests/test_gpu_center.py: the center normwise, the sides against the input's level."""
        if not sides:
            return relerr(val, r)
        level = float(np.abs(r[0] + r[1]).max())
        return max(relerr(val[0], r[0]), float(np.abs(val[1] - r[1]).max()) / level)
    run(zafx, Prep(plan, x, n, arena.uniform_blocks(plan.out_shape(3, n), None, ref), TOL_FFT, lambda di, do: "k_center", err=err), pairs(DELTAS))


# ------------------------------------------------------------------------------------------------ ragged batches
RAGGED_PAIRS = [(128, 128), (128, 8), (4, 128), (4, 8)]


@pytest.mark.parametrize("route", ["stft2048", "stft1024", "mel"])
def test_ragged(zafx, route):
    """Three lengths in one call, rows padded to whole lines: one launch at delta_out = 128, one execute per clip at 8 (the blocks' bases are off
    the line grid then).  The guards stand in for the exact-size sentinel of tests/test_gpu_ragged.py outside the whole array; the padding
    inside it is (b)'s."""
    w = 1024 if route == "stft1024" else 2048
    hop = w // 2
    lengths = np.array([37 * hop + 5, 3000, 33 * hop], np.int64)
    x = [np.random.default_rng([77, i]).standard_normal(int(n)).astype(np.float32) for i, n in enumerate(lengths)]
    in_offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    flat = np.concatenate(x)
    win = orc.hamming_periodic(w)
    if route == "mel":
        fb = zafx.melfilterbank(44100, w, 128)
        plan, tol, native = zafx.mel_plan(zafx.hamming(w), hop, fb, row_align=32), TOL_FB, "k_mel2_ragged"
        ref = [orc.melspectrogram(c.astype(np.float64), win, hop, orc.melfilterbank(44100, w, 128)) for c in x]
    else:
        plan, tol, native = zafx.stft_plan(zafx.hamming(w), hop, row_align=16), TOL_FFT, "k_stft_ft16_ragged"
        ref = [orc.stft(c.astype(np.float64), win, hop) for c in x]
    offs, frames, pitch = plan.ragged_layout(lengths)
    rows = ref[0].shape[0]
    blocks = [arena.Block(int(offs[i]), (rows, int(pitch[i])), int(frames[i]), ref[i]) for i in range(3)]
    assert int(offs[3]) == sum(rows * int(p) for p in pitch)
    poisoned = flat.copy()
    poisoned[in_offsets[1]:in_offsets[1] + lengths[1]] = np.nan
    launch = lambda d_in, d_out: (plan.execute_ragged(d_in, in_offsets, lengths, d_out), plan.sync())
    prep = Prep(plan, flat, None, blocks, tol, lambda di, do: native if do % 128 == 0 else "per-clip*", launch=launch, poisoned=poisoned, n_clips=1)
    prep.guard = arena.guard_bytes(int(lengths.max()) * 4, max(rows * int(p) for p in pitch) * plan.out_dtype.itemsize)
    run(zafx, prep, RAGGED_PAIRS)


# ------------------------------------------------------------------------------------------------ the ragged MDCT, IMDCT and center launches
INPUT_GAPS = (1, 3, 5)     # elements of poison behind clips 0, 1 and 2 of the input (the entry points take free offsets)
POISON32 = np.array([arena.poison_word(np.float32)[1]], np.uint32).view(np.float32)[0]


def with_gaps(parts, gaps, unit=1):
    """`parts` (1-D float32 arrays) laid out with gaps[i] * unit poison elements behind part i: -> (flat, offsets in elements)."""
    offsets, pieces, at = [], [], 0
    for i, a in enumerate(parts):
        offsets.append(at)
        g = np.full(gaps[i % len(gaps)] * unit, POISON32, np.float32)
        pieces += [np.ascontiguousarray(a, np.float32).reshape(-1), g]
        at += a.size + g.size
    flat = np.concatenate(pieces) if pieces else np.zeros(0, np.float32)
    return flat, np.array(offsets, np.int64)


def ragged_guard(in_elems, blocks):
    """arena.guard_bytes(longest clip's input bytes, largest block's output bytes): the harness's condition (tests/arena.py)."""
    return arena.guard_bytes(int(max(in_elems)) * 4, max(int(np.prod(b.shape, dtype=np.int64)) for b in blocks) * 4)


@pytest.mark.parametrize("form", ["edge", "aligned"])
@pytest.mark.parametrize("w", [2048, 512])
def test_mdct_ragged(zafx, w, form):
    """k_mdct_ft32_ragged: three lengths in one call at row_align = 32.  "edge": lengths off the 4-sample grid with 1, 3 and 5 poisoned samples
    behind the clips -- a clip that reads past its end (a KBD window edge of 1e-5 hides that on noise) or in front of its start reads NaN;
    "aligned": lengths that are multiples of 4 back to back -- the 16-byte-load form at delta_in = 128 and 16, the 4-byte form on a base 4
    or 8 bytes off.  One launch at delta_out = 128, one execute per clip at 8."""
    m = w // 2
    lengths = [37 * m + 5, 3000 + 1, 33 * m]
    if form == "aligned":
        lengths = [n - n % 4 for n in lengths]
    x = [np.random.default_rng([78, w, i]).standard_normal(n).astype(np.float32) for i, n in enumerate(lengths)]
    flat, in_offsets = with_gaps(x, INPUT_GAPS if form == "edge" else (0,))
    lengths = np.array(lengths, np.int64)
    assert form == "edge" or not (in_offsets % 4).any() and not (lengths % 4).any()
    win = orc.kbd_window(w)
    ref = [orc.mdct(c.astype(np.float64), win) for c in x]
    plan = zafx.mdct_plan(zafx.kaiser_bessel_derived(w), row_align=32)
    offs, frames, pitch = plan.ragged_layout(lengths)
    blocks = [arena.Block(int(offs[i]), (m, int(pitch[i])), int(frames[i]), ref[i]) for i in range(3)]
    assert int(offs[3]) == sum(m * int(p) for p in pitch) and [r.shape[1] for r in ref] == frames.tolist()
    poisoned = flat.copy()
    poisoned[in_offsets[1]:in_offsets[1] + lengths[1]] = np.nan
    launch = lambda d_in, d_out: (plan.execute_ragged(d_in, in_offsets, lengths, d_out), plan.sync())
    prep = Prep(plan, flat, None, blocks, TOL_FFT, lambda di, do: "k_mdct_ft32_ragged" if do % 128 == 0 else "per-clip*", launch=launch, poisoned=poisoned, n_clips=1)
    prep.guard = ragged_guard(lengths, blocks)
    run(zafx, prep, RAGGED_PAIRS + [(8, 128), (16, 128)])


IMDCT_RAGGED_PAIRS = [(di, do) for di in (128, 4, 8) for do in (128, 4, 8)]


def imdct_ragged_prep(zafx, w, frames, row_align, middle):
    """Blocks of `frames` frames at the plan's pitch, pad columns NaN, 1, 3 and 5 poisoned floats behind them; the clips' samples at
    caller-chosen places with 1 and 3 floats between them and 2 behind the last.  `middle`: the block the second pass poisons, or None."""
    m = w // 2
    win = orc.kbd_window(w)
    plan = zafx.mdct_plan(zafx.kaiser_bessel_derived(w), inverse=True, row_align=row_align)
    coefs, ref, packed = [], [], []
    for i, t in enumerate(frames):
        c = orc.mdct(np.random.default_rng([79, w, i]).standard_normal((t - 1) * m), win).astype(np.float32)
        assert c.shape == (m, t)
        p = plan.row_pitch(t)
        assert p % 4 == 0   # (native by the header's contract)
        rows = np.full((m, p), np.nan, np.float32)
        rows[:, :t] = c
        coefs.append(c), packed.append(rows)
        ref.append(orc.imdct(c.astype(np.float64), win) if t > 1 else np.zeros(0))
    flat, in_offsets = with_gaps(packed, INPUT_GAPS)
    blocks, out_offsets, at = [], [], 0
    for i, r in enumerate(ref):
        out_offsets.append(at)
        if len(r):
            assert len(r) == m * (frames[i] - 1) - 1
            blocks.append(arena.Block(at, (len(r),), len(r), r))
            at += len(r)
        gap = (1, 3, 2)[i]   # (a block of one frame writes nothing: its place is the gap that follows)
        blocks.append(arena.gap_block(at, gap))
        at += gap
    poisoned = None
    if middle is not None:
        poisoned = flat.copy()
        poisoned[in_offsets[middle]:in_offsets[middle] + packed[middle].size] = np.nan
    frames_a, out_a = np.array(frames, np.int64), np.array(out_offsets, np.int64)
    launch = lambda d_in, d_out: (plan.execute_imdct_ragged(d_in, in_offsets, frames_a, d_out, out_a), plan.sync())
    prep = Prep(plan, flat, None, blocks, TOL_FFT, lambda di, do: "k_imdct_ragged", launch=launch, poisoned=poisoned, n_clips=1,
                middle=None if middle is None else 2 * middle)   # (clip i is block 2 i: a gap follows every clip)
    prep.guard = ragged_guard([r.size for r in packed], blocks)
    return prep


@pytest.mark.parametrize("rows", ["padded", "compact", "one_frame"])
@pytest.mark.parametrize("w", [2048, 512])
def test_imdct_ragged(zafx, w, rows):
    """k_imdct_ragged on coefficient arrays and sample arrays 4 and 8 bytes off the grid (16-byte buffer loads "at any 4-byte alignment", pair
    stores that need their dword only: include/zafx.h).  "padded": 37, 2 and 33 frames in rows of 64, 32 and 64 with NaN pad columns;
    "compact": 36, 4 and 32 frames at a pitch of their own, every one a multiple of 4; "one_frame": the middle block is a single frame,
    which writes nothing -- its place in the output is a gap (one pass: there is no neighbour's result to compare)."""
    if rows == "padded":
        prep = imdct_ragged_prep(zafx, w, [37, 2, 33], 32, 1)
    elif rows == "compact":
        prep = imdct_ragged_prep(zafx, w, [36, 4, 32], 0, 1)
    else:
        prep = imdct_ragged_prep(zafx, w, [37, 1, 33], 32, None)
    run(zafx, prep, IMDCT_RAGGED_PAIRS)


# (4, 4), (4, 128): a base at 4 mod 8 -- k_center reads and writes a sample frame as one 8-byte piece at the clip's base plus a multiple of 8,
# and test_center runs the same loads and stores at delta = 4; include/zafx.h states the 4-byte rule for zafx_execute_center_ragged
CENTER_RAGGED_PAIRS = [(8, 8), (16, 64), (64, 128), (128, 8), (4, 4), (4, 128)]


@pytest.mark.parametrize("empty", [False, True], ids=["three", "with_empty"])
@pytest.mark.parametrize("sides", [True, False], ids=["center_sides", "center"])
@pytest.mark.parametrize("w", [256, 1024, 2048])
def test_center_ragged(zafx, w, sides, empty):
    """k_center_ragged: clips of 2 F H + 65, F H (a tile's end exactly) and 3 F H - 1 sample frames with 1, 3 and 5 poisoned sample frames
    behind them, their results at caller-chosen places with 1 and 3 sample frames between the blocks; "with_empty": a fourth clip of length
    0, of which nothing is written.  test_center's error function (center normwise, sides against the input's level)."""
    from center_oracle import oracle_center
    from test_gpu_center import stereo
    f, h = zafx.center_tile_frames(w), w // 2
    lengths = [2 * f * h + 65, f * h, 3 * f * h - 1] + ([0] if empty else [])
    x = [stereo(3 * w + c, n) for c, n in enumerate(lengths)]
    flat, in_floats = with_gaps(x, INPUT_GAPS, unit=2)
    win = zafx.hamming(w)
    center = [oracle_center(c, win) for c in x[:3]]
    ref = [np.stack([c, xc.astype(np.float64) - c]) for c, xc in zip(center, x)] if sides else center
    per = 2 if sides else 1
    blocks, out_offsets, at = [], [], 0   # (in sample frames)
    for i, n in enumerate(lengths):
        out_offsets.append(at)
        if n:
            blocks.append(arena.Block(2 * at, ref[i].shape, 2, ref[i]))
            at += per * n
        gap = (1, 3, 2, 4)[i]   # (the empty clip's place is a gap)
        blocks.append(arena.gap_block(2 * at, 2 * gap))
        at += gap
    plan = zafx.center_plan(win, sides=sides)
    in_offsets, lens, outs = in_floats // 2, np.array(lengths, np.int64), np.array(out_offsets, np.int64)
    poisoned = flat.copy()
    poisoned[in_floats[1]:in_floats[1] + 2 * lengths[1]] = np.nan

    def err(val, r):
        if not sides:
            return relerr(val, r)
        level = float(np.abs(r[0] + r[1]).max())
        return max(relerr(val[0], r[0]), float(np.abs(val[1] - r[1]).max()) / level)

    launch = lambda d_in, d_out: (plan.execute_center_ragged(d_in, in_offsets, lens, d_out, outs), plan.sync())
    prep = Prep(plan, flat, None, blocks, TOL_FFT, lambda di, do: "k_center_ragged", err=err, launch=launch, poisoned=poisoned, n_clips=1, middle=2)
    prep.guard = ragged_guard([2 * n for n in lengths], blocks)
    run(zafx, prep, CENTER_RAGGED_PAIRS)
