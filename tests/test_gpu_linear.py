"""The two matrix-core kernels of zafx_linear.hip at their tile edges, and the dense dct / dst route that rides on them (-m gpu).

The cases and what each is there for: tests/linear_cases.py.  Three groups:

  arena      every case but the long-row one on views off the allocation grid (tests/arena.py, as tests/test_gpu_arena.py::test_linear does):
             guards intact, every element written, the float64 product within TOL_FFT, every other clip bit-identical with clip 1 poisoned,
             and the kernel the launcher's rule gives for the pair -- a k_linear128 case falls to k_linear where the clips start off the
             16-byte grid; an output 4 or 8 bytes off it takes the scalar stores of k_linear128 whatever rows % 4 is;
  identity   the two k_linear128 cases give the same BITS at every offset pair, whichever kernel the pair reaches: both kernels feed
             v_mfma_f32_16x16x4_f32 the same groups of four k in the same order from a zero accumulator, and with cols % 32 == 0 k_linear
             pads nothing;
  dense dct  zafx.dct_batch / dst_batch / dct at the lengths core._transform_batch still serves by an N x N matrix: 8192 < N <= 16384 off
             the power-of-two grid (8224 on k_linear128 with 257 K tiles, 8194 on k_linear) and one sample."""
import numpy as np
import pytest

import arena
import linear_cases as lc
from conftest import relerr
from oracle import zaf_oracle as orc

pytestmark = pytest.mark.gpu

TOL_FFT = 1e-5
DELTAS = (4, 8, 16, 64)

_DEVICE_ERROR = []


def pairs(deltas):
    out = [(128, 128)]
    for d in deltas:
        out += [(d, d), (128, d), (d, 128)]
    return out


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    z.set_row_padding("compact")
    yield z
    z.set_row_padding("auto")
    z.clear_plan_cache()


class Case:
    """One case, ready to run at any offset pair."""

    def __init__(self, zafx, rows, cols, count):
        self.shape = (rows, cols, count)
        m = lc.matrix(rows, cols)
        self.x = lc.clips(rows, cols, count)
        self.blocks = arena.uniform_blocks((count, rows), None, list(lc.reference(self.x, m)))
        self.plan = zafx.linear_plan(m)
        self.guard = arena.guard_bytes(cols * 4, rows * 4)
        self.middle = 1 if count >= 3 else None   # (a single clip has no neighbour to poison)

    def launch(self, d_in, d_out):
        self.plan.execute(d_in, d_out, self.shape[2], self.shape[1])
        self.plan.sync()

    def run(self, zafx, pair, exact=None, middle=None):
        """arena.run_case at one pair -> (the whole result as one array, the kernel that ran).  A device error ends the module."""
        if _DEVICE_ERROR:
            pytest.fail(f"not run: an earlier case met a device error ({_DEVICE_ERROR[0]})")
        try:
            got = arena.run_case(zafx, self.x, np.float32, self.blocks, self.guard, pair, self.launch, TOL_FFT, relerr, exact=exact, exact_tol=0.0,
                                 middle=middle)
        except zafx.ZafxError as exc:
            _DEVICE_ERROR.append(f"{self.shape} {pair}: {exc}")
            raise
        return np.stack(got), self.plan.last_kernel


@pytest.mark.parametrize("rows,cols,count", lc.ARENA_CASES, ids=[lc.name_of(c) for c in lc.ARENA_CASES])
def test_linear_at_its_tile_edges(zafx, rows, cols, count):
    case = Case(zafx, rows, cols, count)
    failures, seen = [], []
    for pair in pairs(DELTAS):
        try:
            kernel = case.run(zafx, pair, middle=case.middle)[1]
        except AssertionError as exc:
            failures.append(f"{pair}: {exc}")
            kernel = case.plan.last_kernel
        want = lc.kernel(rows, cols, count, pair[0])
        seen.append(f"{pair}: {kernel}")
        if kernel != want:
            failures.append(f"{pair}: ran {kernel}, the launcher's rule says {want}")
    print("; ".join(seen))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("rows,cols,count", lc.BIG_ARENA_CASES, ids=[lc.name_of(c) for c in lc.BIG_ARENA_CASES])
def test_both_kernels_give_the_same_bits(zafx, rows, cols, count):
    case = Case(zafx, rows, cols, count)
    exact, kernel = case.run(zafx, (128, 128))
    assert kernel == "k_linear128"
    failures, reached = [], set()
    for pair in pairs(DELTAS)[1:]:
        try:
            reached.add(case.run(zafx, pair, exact=exact)[1])
        except AssertionError as exc:
            failures.append(f"{pair} ({case.plan.last_kernel}): {exc}")
    assert reached == {"k_linear", "k_linear128"}, reached
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ dense dct / dst
def dense_plan(zafx, builder, kind, n):
    """The plan core._transform_batch keeps for a dense transform."""
    from zafx import core
    return core._cache[(builder, kind, n, 0)]


def test_dense_dct_on_k_linear128(zafx):
    """dct-II at N = 8224 = 32 * 257 (N / 2 no power of two, above the chirp-z form's 8192): 130 clips make rows x clips >= 2^20, so
    k_linear128 with 257 K tiles, a last row tile of 32 rows and a second clip tile of 2 clips.  16 distinct vectors, replicated.
    The loop is closed by dct-III (the transposed matrix) to the bound of test_gpu_parity.py::test_dct_dst_of_any_length."""
    n = lc.DCT_N
    x = lc.dct_clips()
    got = zafx.dct_batch(x, 2)
    assert dense_plan(zafx, "dct_matrix", 2, n).last_kernel == "k_linear128"
    assert got.shape == x.shape and got.dtype == np.float32
    errs = [relerr(got[c], orc.dct(x[c].astype(np.float64), 2)) for c in range(lc.DCT_DISTINCT)]
    print("dct2_8224 against the oracle:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= TOL_FFT, errs
    assert np.array_equal(got[16:32], got[:16]) and np.array_equal(got[128:130], got[0:2])   # replicas in other tiles
    back = zafx.dct_batch(got[:3], 3)
    assert dense_plan(zafx, "dct_matrix", 3, n).last_kernel == "k_linear"
    print("dct3(dct2(x)) - x:", float(np.max(np.abs(back - x[:3]))))
    assert np.max(np.abs(back - x[:3])) < 3e-5


def test_dense_dst_on_k_linear(zafx):
    """dst-III at N = 8194: cols % 32 != 0, so k_linear, whose last K tile holds 2 columns; the matrix is the transposed one of dst-II."""
    n = 8194
    x = lc.dct_clips(n, 5, 5)
    got = zafx.dst_batch(x, 3)
    assert dense_plan(zafx, "dst_matrix", 3, n).last_kernel == "k_linear"
    assert got.shape == x.shape and got.dtype == np.float32
    errs = [relerr(got[c], orc.dst(x[c].astype(np.float64), 3)) for c in range(5)]
    print("dst3_8194 against the oracle:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= TOL_FFT, errs


def test_dct_dst_of_one_sample(zafx):
    """N = 1 is a 1 x 1 matrix on k_linear (65 clips: two clip tiles); dct-I divides by N - 1 and is refused."""
    x = lc.dct_clips(1, 65, 65)
    for sine, batch, one, kinds in ((False, zafx.dct_batch, orc.dct, (2, 3, 4)), (True, zafx.dst_batch, orc.dst, (1, 2, 3, 4))):
        for t in kinds:
            got = batch(x, t)
            assert dense_plan(zafx, "dst_matrix" if sine else "dct_matrix", t, 1).last_kernel == "k_linear"
            assert got.shape == x.shape and got.dtype == np.float32
            ref = np.stack([one(v.astype(np.float64), t) for v in x])
            assert relerr(got, ref) <= TOL_FFT, (sine, t)
    y = zafx.dct(x[0], 2)
    assert y.shape == (1,) and y.dtype == np.float64 and relerr(y, orc.dct(x[0].astype(np.float64), 2)) <= TOL_FFT
    with pytest.raises(ValueError):
        zafx.dct_batch(x, 1)
    with pytest.raises(ValueError):
        zafx.dct(x[0], 1)
