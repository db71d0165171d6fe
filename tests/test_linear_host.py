"""tests/linear_cases.py held to account on the CPU (no GPU): the table reaches the branches it is there for, the yardstick of its accuracy
lines (tests/plain.py linear_chain) is a correct product and sits where a fused chain -- the matrix core's arithmetic -- can meet the family
factors, and the matrix builders of the dense dct / dst route are right at the lengths that route serves.

Left out here: the dct-II line at N = 8224.  Its chain loop and the two 8224 x 8224 builds it needs take about ten seconds; the fused chain
is held to the yardstick at 4096 columns below, and tests/test_gpu_accuracy.py measures the yardstick at 8224 next to the kernel."""
import numpy as np
import pytest

import accuracy as acc
import accuracy_cases as ac
import linear_cases as lc
import plain
from conftest import relerr
from oracle import zaf_oracle as orc

HEADROOM = 1.5   # the emulated chain stays this far inside the family factors: what is left is for whatever the emulation does not know


def test_expected_kernels_follow_the_launchers_rule():
    for rows, cols, count in lc.CASES:
        big = cols % 32 == 0 and rows * count >= 1 << 20
        assert lc.kernel(rows, cols, count) == ("k_linear128" if big else "k_linear")
        for d_in in (4, 8, 16, 64, 128):
            assert lc.kernel(rows, cols, count, d_in) == ("k_linear128" if big and d_in % 16 == 0 else "k_linear")
        assert 1 <= rows <= 16384 and 1 <= cols <= 16384   # what zafx.linear_plan takes
    assert [lc.kernel(*c) for c in lc.CASES] == ["k_linear"] * 4 + ["k_linear128"] * 3
    assert lc.kernel(lc.DCT_N, lc.DCT_N, lc.DCT_CLIPS) == "k_linear128" and lc.kernel(lc.DCT_N, lc.DCT_N, 3) == "k_linear"
    assert lc.kernel(8194, 8194, 5) == "k_linear" and lc.kernel(1, 1, 65) == "k_linear"
    assert set(lc.BIG_ARENA_CASES) <= set(lc.ARENA_CASES) and lc.LONG_ROWS not in lc.ARENA_CASES


def test_every_branch_has_a_case():
    geo = {c: lc.geometry(*c) for c in lc.ARENA_CASES}
    big = [g for g in geo.values() if g["kernel"] == "k_linear128"]
    small = [g for g in geo.values() if g["kernel"] == "k_linear"]
    assert len(big) == len(lc.BIG_ARENA_CASES) == 2
    # k_linear128: the double buffer (2 K tiles: the second buffer; >= 3: buffer 0 again), both store forms, partial row and clip tiles
    assert {g["k_tiles"] for g in big} >= {2, 3}
    assert {g["float4_stores"] for g in big} == {True, False}
    assert any(0 < g["last_row_tile"] < 128 and g["last_row_tile"] % 4 for g in big)       # a partial tile that ends inside a float4 group
    assert any(g["last_row_tile"] == 4 and g["float4_stores"] for g in big)                # exactly one float4 group
    assert any(g["clip_tiles"] == 2 and g["last_clip_tile"] == 1 for g in big)             # one valid clip, 127 clamped reads behind it
    assert any(g["clip_tiles"] == 2 and g["last_clip_tile"] == 128 for g in big)
    assert all(not lc.geometry(*c, y_offset=d)["float4_stores"] for c in lc.BIG_ARENA_CASES for d in (4, 8))   # the unaligned-y branch
    assert all(lc.geometry(4100, 64, 256, y_offset=d)["float4_stores"] for d in (16, 64, 128))
    assert all(lc.geometry(*c, x_offset=d)["kernel"] == "k_linear" for c in lc.BIG_ARENA_CASES for d in (4, 8))
    # k_linear: a side of 1, one past and one short of a tile on every side, columns off the 4-float pieces, more than one clip tile
    assert geo[(1, 1, 1)] == dict(geo[(1, 1, 1)], row_tiles=1, k_tiles=1, clip_tiles=1, last_row_tile=1, last_k_tile=1, last_clip_tile=1)
    g = geo[(65, 33, 65)]
    assert (g["row_tiles"], g["last_row_tile"], g["k_tiles"], g["last_k_tile"], g["clip_tiles"], g["last_clip_tile"]) == (2, 1, 2, 1, 2, 1)
    g = geo[(63, 31, 130)]
    assert (g["row_tiles"], g["last_row_tile"], g["k_tiles"], g["last_k_tile"], g["clip_tiles"], g["last_clip_tile"]) == (1, 63, 1, 31, 3, 2)
    assert any(g["row_tiles"] == 3 and g["last_k_tile"] == 32 for g in small)
    assert any(c[1] % 4 for c in geo if geo[c]["kernel"] == "k_linear")
    # the long rows and the dense dct
    assert lc.geometry(*lc.LONG_ROWS)["k_tiles"] == 128
    g = lc.geometry(lc.DCT_N, lc.DCT_N, lc.DCT_CLIPS)
    assert (g["k_tiles"], g["last_row_tile"], g["clip_tiles"], g["last_clip_tile"]) == (257, 32, 2, 2)
    assert lc.DCT_N // 2 & (lc.DCT_N // 2 - 1) and lc.DCT_N > 8192                          # off k_dct's grid, above the chirp-z form


def test_judged_clips():
    assert list(lc.judged(1)) == [0] and list(lc.judged(16)) == list(range(16))
    assert list(lc.judged(130)) == list(range(8)) + list(range(122, 130))
    x = lc.dct_clips(8, 35, 16)
    assert np.array_equal(x[16:32], x[:16]) and np.array_equal(x[32:35], x[:3]) and len({v.tobytes() for v in x[:16]}) == 16


def test_the_chain_is_the_product():
    """linear_chain restates x @ m.T (float64 <= 1e-12 of it; long double no further from float64 than a sum's rounding), returns the
    precision asked for, and at float32 is a single-precision computation: its error grows with the columns, as sqrt(cols)."""
    rng = np.random.default_rng(5)
    m, x = rng.standard_normal((37, 300)), rng.standard_normal((5, 300))
    ref = x @ m.T
    for dtype in plain.DTYPES:
        out = plain.linear_chain(x, m, dtype)
        assert out.dtype == np.dtype(dtype) and out.shape == (5, 37)
    assert relerr(plain.linear_chain(x, m, np.float64), ref) <= 1e-12
    assert relerr(plain.linear_chain(x, m, np.longdouble).astype(np.float64), ref) <= 1e-12
    # the same bits as a scalar loop
    want = np.zeros((5, 37), np.float32)
    x32, m32 = x.astype(np.float32), m.astype(np.float32)
    for b in range(5):
        for r in range(37):
            a = np.float32(0)
            for k in range(300):
                a = np.float32(a + np.float32(x32[b, k] * m32[r, k]))
            want[b, r] = a
    assert np.array_equal(plain.linear_chain(x, m, np.float32), want)
    errs = []
    for cols in (64, 1024):
        m, x = rng.standard_normal((200, cols)).astype(np.float32), rng.standard_normal((16, cols)).astype(np.float32)
        errs.append(acc.measure([plain.linear_chain(x, m, np.float32)], [lc.reference(x, m)])["e_rms"])
    assert 2.0 <= errs[1] / errs[0] <= 8.0, errs   # sqrt(1024 / 64) = 4


@pytest.mark.parametrize("case", lc.CASES, ids=lc.name_of)
def test_a_fused_chain_meets_the_family_factors(case):
    """The matrix core's arithmetic, emulated (linear_cases.fused_chain), against the yardstick on the case's own inputs and judged clips:
    inside the family factors of tests/accuracy.py with HEADROOM to spare, so that a kernel which is such a chain passes
    tests/test_gpu_accuracy.py without a factor of its own."""
    rows, cols, count = case
    assert "linear/" + lc.name_of(case) not in ac.OWN_FACTORS
    m = lc.matrix(rows, cols)
    x = lc.clips(rows, cols, count)[lc.judged(count)]
    ref = lc.reference(x, m)
    wide = lambda v: ac.as_measured("LINEAR", list(v))
    k, y = acc.measure(wide(lc.fused_chain(x, m)), wide(ref)), acc.measure(wide(plain.linear_chain(x, m, np.float32)), wide(ref))
    print(acc.line("linear/" + lc.name_of(case), "fused chain", k, y))
    assert relerr(plain.linear_chain(x, m, np.float32), ref) <= 1e-5     # the contract bound holds for the yardstick itself
    tight = {name: f / HEADROOM for name, f in acc.factors().items()}
    assert not acc.over(k, y, tight), (acc.ratios(k, y), tight)


def test_dense_matrices_at_the_lengths_of_the_dense_route():
    """constants.dct_matrix / dst_matrix times a vector against the oracle, as tests/test_host_logic.py does at the golden lengths: at one
    sample (every type; dct-I is refused) and at 8194, above every length an FFT form serves (dct-II and dst-III: a plain and a transposed build)."""
    import zafx
    x1 = np.array([0.75])
    for t in (1, 2, 3, 4):
        assert relerr(zafx.dst_matrix(1, t) @ x1, orc.dst(x1, t)) <= 1e-11
        if t > 1:
            assert relerr(zafx.dct_matrix(1, t) @ x1, orc.dct(x1, t)) <= 1e-11
    with pytest.raises(ValueError):
        zafx.dct_matrix(1, 1)
    n = 8194
    x = np.random.default_rng(n).standard_normal(n)
    m = zafx.dct_matrix(n, 2)
    assert m.shape == (n, n) and relerr(m @ x, orc.dct(x, 2)) <= 1e-11
    del m
    m = zafx.dst_matrix(n, 3)
    assert m.shape == (n, n) and relerr(m @ x, orc.dst(x, 3)) <= 1e-11
