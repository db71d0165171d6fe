"""Every kernel route held to the accuracy of a plain transform of its own precision (-m gpu).

The contract bounds of the parity tests (1e-5, 1e-4, 1e-12 / 1e-10 normwise) leave a kernel a factor of 20 ... 60 (float32) or several
thousand (float64) above what it achieves, and the byte hashes of tests/golden say "changed", never "worse".  Here every case runs once,
its result and the yardstick's -- tests/plain.py at float32 or float64 on the same input and constants -- are measured against the same
reference (the pinned float64 oracle; tests/plain.py at long double for a float64 kernel) with the four metrics of tests/accuracy.py, and
the kernel must stay within K times the yardstick in each: 2 for e_rms, 3 for e_max, e_row, e_col, twice that for a Bluestein route, a
per-case factor with its cause in tests/accuracy_cases.OWN_FACTORS.  The contract bound holds on top, unchanged.

The cases: constants A of every route of tests/const_probe.py but the center mask; the 92 calls of tests/route_cases.py on the very inputs
its hashes were recorded with (kernel names held to tests/golden/call_routes.json); float64 Bluestein STFT and MDCT at W = 1000 (the only
device-side trigonometry), k_mel's melspectrogram at W = 1024, and dct / dst of types 1-4 at 64, 1024 (k_dct), 100, 132 (k_dct_bsh) and 134 (k_dct_bs32), 8 rows each; k_linear and k_linear128 at the shapes of tests/linear_cases.py and the dense dct-II at
N = 8224, 16 clips each, whose yardstick is one k-ordered float32 chain per output (plain.linear_chain: what the matrix core computes; BLAS is
4 ... 9 times below any single chain at thousands of columns); the eight fused float32 mask-filter kernels at the 112 cases of
tests/maskfilter_cases.py (real masks in three layouts, three stems, complex masks, interleaved stereo under one mask and under one per
channel; W = 256 ... 2048; T = 62 and 63; with and without the rest), each through its equal-length and its ragged launch, whose shared clips
must agree bit for bit, against plain.maskfilter* -- unpacked, one frame and one channel per transform.  (The four PCM kernels' float32
output is held to the float kernels' bits in tests/test_gpu_maskfilter_pcm.py and tests/test_gpu_windows.py, which carries the judgment over.)

One line per case: kernel, the eight numbers, the four ratios.  ZAFX_ACCURACY_REPORT=path writes them as JSON (profiles/accuracy_ratios.json)."""
import json
import os

import numpy as np
import pytest

import accuracy as acc
import accuracy_cases as ac
import const_probe as cp
import maskfilter_cases as mc
import maskfilter_run as mr
import plain
import route_cases as rc
from conftest import GOLDEN, relerr

pytestmark = pytest.mark.gpu

_report = {}


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    if z.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    yield z
    z.clear_plan_cache()
    path = os.environ.get("ZAFX_ACCURACY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_report, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def routes():
    with open(os.path.join(GOLDEN, "call_routes.json")) as f:
        return json.load(f)


def judge(name, kernel_name, kind, got, ref, yard, hop, window_length=0):
    """Measures, prints, records; then asserts the factors."""
    wide = lambda v: [np.asarray(a) for a in ac.as_measured(kind, v)]
    k, y = acc.measure(wide(got), wide(ref), hop), acc.measure(wide(yard), wide(ref), hop)
    own = ac.OWN_FACTORS.get(name)
    factors = acc.factors(ac.bluestein(kernel_name, window_length), own[0] if own else None)
    print(acc.line(name, kernel_name, k, y))
    _report[name] = acc.record(kernel_name, k, y, factors)
    assert all(np.isfinite(v) for v in k.values()), (name, k)
    missed = acc.over(k, y, factors)
    assert not missed, (name, kernel_name, missed, acc.ratios(k, y), factors)


def run_probe(zafx, case):
    """One execute of a tests/const_probe.py case under constants A into a NaN-filled buffer -> the clips' results."""
    plan = case.make()
    d_in = d_out = None
    try:
        bound = case.bind(plan)
        d_in = zafx.DeviceBuffer.from_host(bound["x"])
        d_out = zafx.DeviceBuffer(bound["out_shape"], plan.out_dtype)
        d_out.upload(cp.nan_filled(bound["out_shape"], plan.out_dtype))
        bound["launch"](plan, d_in, d_out)
        plan.sync()
        out = d_out.download()
        assert plan.last_kernel == case.kernel, (plan.last_kernel, case.kernel)
        return [np.array(g) for g in bound["split"](out)]
    finally:
        for d in (d_in, d_out):
            if d is not None:
                d.free()
        plan.destroy()


def probe(zafx, name, case):
    got = run_probe(zafx, case)
    contract = case.refs(None)
    assert max(case.err(np.asarray(g, r.dtype), r) for g, r in zip(got, contract)) <= case.tol, name   # the old bound, on top
    judge(f"const/{name}", case.kernel, case.kind, got, ac.probe_reference(case), ac.probe_yardstick(case), ac.probe_hop(case), ac.probe_window(case))


@pytest.mark.parametrize("route", ac.PROBE_ROUTES)
def test_route_is_as_accurate_as_a_plain_transform(zafx, route):
    probe(zafx, route, cp.case(route))


@pytest.mark.parametrize("route", sorted(ac.ADDED_PROBES))
def test_added_case_is_as_accurate_as_a_plain_transform(zafx, route):
    """W = 1000 in float64 (the chirps come from sincospi on the device) and k_mel's melspectrogram."""
    probe(zafx, route, ac.ADDED_PROBES[route]())


@pytest.mark.parametrize("name", list(rc.CASES))
def test_call_is_as_accurate_as_a_plain_transform(zafx, routes, name):
    c = rc.CASES[name]
    keep = {}
    kernel, digest = rc.record(name, keep)
    assert kernel == routes[name][0], (name, kernel, digest)
    x = ac.route_input(c, keep["x"], keep["n_in"], keep["pitch"])
    got = ac.route_output(c, keep)
    consts = ac.route_consts(c)
    ref = ac.route_reference(c, x, consts)
    tol = cp.TOL_FB if c["family"] in ("mel", "mfcc") else cp.TOL_FFT
    assert max(relerr(np.asarray(g, r.dtype), r) for g, r in zip(got, ref)) <= tol, name
    judge(f"call/{name}", kernel, c["family"], got, ref, ac.route_plain(c, x, np.float32, consts), ac.route_hop(c), c["W"])


@pytest.mark.parametrize("name", list(ac.DCT_CASES))
def test_dct_dst_are_as_accurate_as_a_plain_transform(zafx, name):
    n, t, sine, kernel = ac.DCT_CASES[name]
    x = ac.dct_input(n)
    plan = zafx.dct_plan(n, t, sine)
    got = plan.run_host(x, n)
    assert plan.last_kernel == kernel and got.shape == x.shape and got.dtype == np.float32, (plan.last_kernel, kernel)
    ref = ac.dct_reference(x, t, sine)
    assert max(relerr(g.astype(np.float64), r) for g, r in zip(got, ref)) <= cp.TOL_FFT
    judge(f"dct/{name}", kernel, "DCT", list(got), ref, ac.dct_plain(x, t, sine, np.float32), None)


@pytest.mark.parametrize("name", ac.MASKFILTER_NAMES)
def test_maskfilter_is_as_accurate_as_a_plain_chain(zafx, name):
    """The eight fused float32 mask-filter kernels (tests/maskfilter_cases.py): each case through its equal-length launch and, with four short
    clips between the same three, through its ragged one; the ragged launch must give every shared clip the bits of the equal-length one.  A
    stereo form's rows are its channels, and the level of the old bound is taken over both."""
    form, wl, rest, b, twin, where = ac.maskfilter_case(name)
    kernels = mc.KERNELS[mc.family_of(form)]
    tail = mc.rest_rows(form)
    got = mr.run(form, b["w"], b["clips"], b["masks"], rest, ragged=False)
    rag = mr.run(form, twin["w"], twin["clips"], twin["masks"], rest, ragged=True)
    for k, i in enumerate(where):
        assert np.array_equal(mr.bits(rag[i]), mr.bits(got[k])), (name, "ragged clip", i, "equal-length clip", k)
    for tag, kernel, res, case in ((name, kernels[0], got, b), (name + "/ragged", kernels[1], rag, twin)):
        for r, ref, x in zip(res, case["refs"], case["clips"]):   # the old bound, on top: every stem and the rest
            assert np.isfinite(r).all(), (tag, "the output was not written everywhere")
            for j in range(len(r)):
                err = mc.mask_error(r[j], ref[j], mc.row_level(ref, x, j, tail))   # (the references' rows: the stems, then the rest)
                assert err <= mc.TOL_FFT, (tag, len(x), j, err)
        judge(f"maskfilter/{tag}", kernel, "MASKFILTER", mc.all_rows(res), mc.rows_of(case["refs"], rest, tail), mc.rows_of(case["yard"], rest, tail), wl // 2)


@pytest.mark.parametrize("name", ac.LINEAR_NAMES)
def test_linear_is_as_accurate_as_a_single_chain(zafx, name):
    """Both kernels of zafx_linear.hip at the shapes of tests/linear_cases.py -- 1 to 128 K tiles -- and the dense dct-II at N = 8224 (257 K
    tiles through zafx.dct_batch), the judged clips against plain.linear_chain at float32."""
    from zafx import core
    x, m, pick, ref, kernel = ac.linear_case(name)
    if name == ac.DCT2_DENSE:
        got = zafx.dct_batch(x, 2)
        plan = core._cache[("dct_matrix", 2, x.shape[1], 0)]
    else:
        plan = zafx.linear_plan(m)
        got = plan.run_host(x, x.shape[1])
    assert plan.last_kernel == kernel and got.shape == (len(x), len(m)) and got.dtype == np.float32, (plan.last_kernel, kernel)
    got = got[pick]
    assert max(relerr(g.astype(np.float64), r) for g, r in zip(got, ref)) <= cp.TOL_FFT
    judge(f"linear/{name}", kernel, "LINEAR", list(got), list(ref), list(plain.linear_chain(x[pick], m, np.float32)), None)
