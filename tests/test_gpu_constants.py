"""A plan whose constants are replaced after it has run (-m gpu): zafx_plan_set_constant on a plan that is in use.

The C-ABI lets a caller upload a constant at any time; everything derived from it (the COLA gain, the MDCT's folded window, the packed
filterbank and DCT fragments and the route they select, k_cqt's packed tables and their form) is rebuilt by finalize_constant in
zafx_capi.cpp.  The Python factories never reach that path (their cache keys on a digest of the constants), a C caller that keeps one plan
and swaps its window or filterbank does.  Every case here (tests/const_probe.py) runs one route on a private plan:

  step 1  constants A: execute into a NaN-filled buffer, against the float64 oracle on A;
  step 2  constants B uploaded over A on the same plan: against the oracle on B, and bit for bit -- the whole buffer, pad columns included --
          what a fresh plan made with B gives; last_kernel and zafx_plan_kernel_name are the fresh plan's; no NaN inside a clip's result,
          nothing but NaN in the padding;
  step 3  A again: step 1's bits.

Before any GPU work a case asserts on the host that B's reference differs from A's by MIN_CHANGE = 0.1 or more in every clip, so it cannot
pass by ignoring the upload.  The bounds are the project's: TOL_FFT 1e-5, TOL_FB 1e-4, float64 1e-12 (MFCC 1e-10), tests/center_oracle.py's
for the center; the bit comparisons take none.  One case per family (const_probe.ASYNC) makes step 2's upload while step 1's execute is
still in the stream, before its result is downloaded: zafx_plan_set_constant waits for the plan's stream before it frees anything, so step 1's
result is still A's.

The fused mask-filter kernels take a second device input, the masks, which the Case machinery of tests/const_probe.py has no place for: their
A -> B -> A -> zero gain -> A runs through tests/maskfilter_run.py on a private plan (test_maskfilter_window_replaced_on_a_used_plan, at the end).

k_cqt's two forms (matrix-core for a numerically real matrix, lane reduction otherwise) share the name k_cqt; zafx_plan_cqt_form
(Plan.cqt_form) tells which one a launch took, and every float32 CQT case holds it to the fresh plan's and, after A again, to step 1's."""
import numpy as np
import pytest

import const_probe as cp
from conftest import excess, relerr, synth_clip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    if z.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return z


def run(z, plan, bound, d_in, before_download=None):
    """One execute into a fresh NaN-filled buffer; `before_download` runs between the enqueue and the download."""
    d_out = z.DeviceBuffer(bound["out_shape"], plan.out_dtype)
    try:
        d_out.upload(cp.nan_filled(bound["out_shape"], plan.out_dtype))
        bound["launch"](plan, d_in, d_out)
        if before_download is not None:
            before_download()
        plan.sync()
        return d_out.download()
    finally:
        d_out.free()


def refused(z, plan, bound, d_in):
    """The message with which the plan refuses to execute (None: it ran), and whether the NaN-filled output stayed untouched."""
    d_out = z.DeviceBuffer(bound["out_shape"], plan.out_dtype)
    try:
        d_out.upload(cp.nan_filled(bound["out_shape"], plan.out_dtype))
        try:
            bound["launch"](plan, d_in, d_out)
        except z.ZafxError as e:
            plan.sync()
            return str(e), bool(np.isnan(cp.scalars_of(d_out.download())).all())
        plan.sync()
        return None, False
    finally:
        d_out.free()


def check(case, bound, out, refs, tag, rows=None):
    """The clips' results (their leading `rows` rows; None: all) against the oracle; NaN nowhere inside them and everywhere in the padding."""
    got = bound["split"](out)
    assert len(got) == len(refs)
    got = [np.asarray(g, np.complex128 if np.iscomplexobj(g) else np.float64) for g in got]
    if any(g.shape != r.shape for g, r in zip(got, refs)):
        errs = [float("inf")]
    elif rows is not None:
        errs = [relerr(g[:rows], r[:rows]) if rows else 0.0 for g, r in zip(got, refs)]
    else:
        errs = [case.err(g, r) for g, r in zip(got, refs)]
    print(f"{tag}: worst normwise error {max(errs):.3g} (bound {case.tol:g})")
    scalars, keep = cp.scalars_of(out), bound["keep"]
    if keep is None:
        assert np.isfinite(scalars).all(), (tag, "NaN inside a result")
    else:
        per = scalars.size // keep.size
        assert np.isfinite(scalars.reshape(-1, per)[keep.reshape(-1)]).all(), (tag, "NaN inside a result")
        assert np.isnan(scalars.reshape(-1, per)[~keep.reshape(-1)]).all(), (tag, "the padding was written")
    assert max(errs) <= case.tol, (tag, errs)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(cp.as_bytes(a), cp.as_bytes(b)))


def teeth(case, variant):
    ref_a, ref_b = case.refs(None), case.refs(variant)
    change = min(case.err(b, a) for a, b in zip(ref_a, ref_b))
    assert change >= cp.MIN_CHANGE, (variant, change)
    return ref_a, ref_b


def swap(zafx, route, variant, overlapped):
    case = cp.case(route)
    steps = case.variants[variant]
    ref_a, ref_b = teeth(case, variant)   # host arithmetic, before any GPU work
    fresh = case.make(case.after(steps))
    plan = case.make()
    d_in = None
    try:
        bound = case.bind(plan)
        d_in = zafx.DeviceBuffer.from_host(bound["x"])
        # the fresh plan with B: its result -- or, for the one-pass mel + mfcc plan alone, the words of its refusal (a filterbank its one
        # kernel does not take)
        try:
            out_f, message = run(zafx, fresh, bound, d_in), None
        except zafx.ZafxError as e:
            if route != "mel2_both":
                raise
            out_f, message = None, str(e)
        cqt32 = case.kind in ("CQT", "CHROMA") and not case.kw["f64"]
        # step 1
        out_1 = run(zafx, plan, bound, d_in, (lambda: cp.upload(plan, steps)) if overlapped else None)
        assert plan.last_kernel == case.kernel, (route, plan.last_kernel)
        check(case, bound, out_1, ref_a, f"{route} A")
        form_1 = plan.cqt_form
        assert (form_1 is not None) == cqt32
        # step 2
        if not overlapped:
            cp.upload(plan, steps)
        if message is not None:
            again, untouched = refused(zafx, plan, bound, d_in)
            assert again == message and untouched, (again, message, untouched)
        else:
            out_2 = run(zafx, plan, bound, d_in)
            check(case, bound, out_2, ref_b, f"{route} {variant}", case.oracle_rows.get(variant))
            assert same_bits(out_2, out_f), (route, variant, "the reused plan's result is not the fresh plan's")
            assert (plan.last_kernel, plan.kernel_name, plan.cqt_form) == (fresh.last_kernel, fresh.kernel_name, fresh.cqt_form)
            if variant == "values_complex":
                assert plan.cqt_form == "lane-reduction"
        # step 3
        cp.upload(plan, case.restore(steps))
        out_3 = run(zafx, plan, bound, d_in)
        assert same_bits(out_3, out_1), (route, variant, "A again does not give step 1's bits")
        assert plan.last_kernel == case.kernel and plan.cqt_form == form_1
    finally:
        if d_in is not None:
            d_in.free()
        plan.destroy()
        fresh.destroy()


@pytest.mark.parametrize("route,variant", cp.pairs(), ids=lambda v: v)
def test_constants_replaced(zafx, route, variant):
    swap(zafx, route, variant, False)


@pytest.mark.parametrize("route", sorted(cp.ASYNC))
def test_upload_behind_a_running_execute(zafx, route):
    """Step 2's set_* call is made while step 1's execute is still in the plan's stream: step 1's result is A's all the same."""
    swap(zafx, route, cp.ASYNC[route], True)


CQT32 = ("cqt_tiny", "cqt_8192", "chroma_8192", "cqt_split", "chroma_split", "cqt_65536")


def test_a_cqt_case_runs_the_matrix_core_form(zafx):
    """Both forms of k_cqt carry its name; Plan.cqt_form (zafx_plan_cqt_form) tells which one the last launch took.  Through fresh plans: at
    least one float32 case runs the matrix-core form under A, and every one that does runs the lane reduction under B2 -- so the B2 cases of
    test_constants_replaced, which hold the reused plan to (A's form, the fresh B2 plan's, A's again), see the form switch off and come back."""
    forms = {}
    for route in CQT32:
        case = cp.case(route)
        for name in (None, "values_complex"):
            if name is not None and name not in case.variants:
                continue
            plan = case.make(None if name is None else case.after(case.variants[name]))
            d_in = None
            try:
                assert plan.cqt_form is None
                bound = case.bind(plan)
                d_in = zafx.DeviceBuffer.from_host(bound["x"])
                run(zafx, plan, bound, d_in)
                forms[route, name] = plan.cqt_form
            finally:
                if d_in is not None:
                    d_in.free()
                plan.destroy()
    print(forms)
    matrix_core = [r for r in CQT32 if forms[r, None] == "matrix-core"]
    assert any((r, "values_complex") in forms for r in matrix_core), forms
    assert all(forms[r, "values_complex"] == "lane-reduction" for r in CQT32 if (r, "values_complex") in forms), forms


# ------------------------------------------------------------------------------------------------ a window whose COLA sum is zero
@pytest.mark.parametrize("route", ["istft_ft16", "center_sides_2048"])
def test_zero_gain_refused(zafx, route):
    """B0 = A with B0[0] = -B0[hop]: execute refuses with the reference's division by zero in words and writes nothing; A again: step 1's bits."""
    case = cp.case(route)
    steps = case.variants["zero_gain"]
    plan = case.make()
    d_in = None
    try:
        bound = case.bind(plan)
        d_in = zafx.DeviceBuffer.from_host(bound["x"])
        out_1 = run(zafx, plan, bound, d_in)
        check(case, bound, out_1, case.refs(None), f"{route} A")
        cp.upload(plan, steps)
        message, untouched = refused(zafx, plan, bound, d_in)
        assert message is not None and "sum(window[0:W:H]) is zero" in message, message
        assert untouched
        cp.upload(plan, case.restore(steps))
        assert same_bits(run(zafx, plan, bound, d_in), out_1)
    finally:
        if d_in is not None:
            d_in.free()
        plan.destroy()


# ------------------------------------------------------------------------------------------------ the ragged entry points on a reused plan
LENGTHS = (0, 1, 3072, 16 * 1024 + 3)
FRAMES = (1, 2, 4, 18)   # the frame counts of LENGTHS at W = 2048, hop 1024 (STFT and MDCT alike)
GAPS = (1, 3, 5)


def with_gaps(parts, dtype, unit=1, gaps=GAPS, fill=np.nan):
    offsets, pieces, at = [], [], 0
    for i, a in enumerate(parts):
        offsets.append(at)
        g = np.full(gaps[i % len(gaps)] * unit, fill, dtype)
        pieces += [np.ascontiguousarray(a, dtype).reshape(-1), g]
        at += a.size + g.size
    return np.concatenate(pieces), np.array(offsets, np.int64)


def out_places(sizes):
    offs, at = [], 5
    for i, n in enumerate(sizes):
        offs.append(at)
        at += n + GAPS[i % len(GAPS)]
    return np.array(offs, np.int64), at


def ragged_forward(kind, f64=False, pcm=False):
    """execute_ragged (execute_ragged_pcm on int16 mono) of a mel or MDCT plan at W = 2048 whose rows are whole lines."""
    from oracle import zaf_oracle as orc
    w, hop = 2048, 1024
    dtype = np.float64 if f64 else np.float32
    lens = np.array(LENGTHS, np.int64)
    if pcm:
        xs = [np.round(synth_clip(93, i, n) * 8000.0).clip(-32768, 32767).astype(np.int16) for i, n in enumerate(LENGTHS)]
        even = [x if len(x) % 2 == 0 else np.append(x, np.iinfo(np.int16).min) for x in xs]    # (even offsets: the kernel's own loads)
        flat, in_offsets = with_gaps(even, np.int16, gaps=(2, 4, 6), fill=np.iinfo(np.int16).min)
        assert not (in_offsets % 2).any()
        x64 = [x.astype(np.float64) / 32768.0 for x in xs]
    else:
        xs = [synth_clip(92, i, n).astype(dtype) for i, n in enumerate(LENGTHS)]
        flat, in_offsets = with_gaps(xs, dtype)
        x64 = [x.astype(np.float64) for x in xs]
    if kind == "mel":
        consts = {"window": cp.window_a(w), "fb": cp.fb_mel(cp.FS, w, 128)}
        steps = [("window", cp.win.skew(w)), ("fb", cp.fb_mel(16000, w, 128))]
        ref = lambda c: [c["fb"] @ np.abs(orc.stft(x, c["window"], hop)[1:w // 2 + 1]) for x in x64]
        case = cp.Case("MEL", dict(window_length=w, step_length=hop, n_filters=128, row_align=32), consts, ref, None, cp.TOL_FB, "k_mel2_ragged", {"b": steps})
    else:
        consts = {"window": cp.window_a(w, True)}
        ref = lambda c: [orc.mdct(x, c["window"]) for x in x64]
        case = cp.Case("MDCT", dict(window_length=w, row_align=16 if f64 else 32, f64=f64), consts, ref, None, cp.TOL_F64 if f64 else cp.TOL_FFT,
                       "k_mdct_ft16_f64_ragged" if f64 else "k_mdct_ft32_ragged", {"b": [("window", cp.win.skew(w))]})

    def bind(plan):
        offs, frames, pitch = plan.ragged_layout(lens)
        assert tuple(frames.tolist()) == FRAMES
        rows = plan.out_dims(int(lens[-1]))[0]
        keep = np.zeros(int(offs[-1]), bool)
        block = lambda a, i: a[int(offs[i]):int(offs[i]) + rows * int(pitch[i])].reshape(rows, int(pitch[i]))[:, :int(frames[i])]
        for i in range(len(lens)):
            block(keep, i)[:] = True
        launch = (lambda p, d_in, d_out: p.execute_ragged_pcm(d_in, in_offsets, lens, d_out, 1)) if pcm else \
                 (lambda p, d_in, d_out: p.execute_ragged(d_in, in_offsets, lens, d_out))
        return dict(x=flat, out_shape=(int(offs[-1]),), launch=launch, split=lambda out: [block(out, i) for i in range(len(lens))], keep=keep)
    case.bind = bind
    return case


def ragged_inverse(kind):
    """execute_imdct_ragged / execute_istft_ragged at W = 2048: blocks at the plan's pitch with NaN pad columns and gaps behind them."""
    from oracle import zaf_oracle as orc
    w, hop = 2048, 1024
    if kind == "imdct":
        a = cp.window_a(w, True)
        blocks = [orc.mdct(synth_clip(94, i, (t - 1) * hop).astype(np.float64), a).astype(np.float32) for i, t in enumerate(FRAMES)]
        ref = lambda c: [orc.imdct(b.astype(np.float64), c["window"]) if t > 1 else np.zeros(0) for b, t in zip(blocks, FRAMES)]
        sizes = [max(hop * (t - 1) - 1, 0) for t in FRAMES]
        plan_kind, kw, dtype, name, kernel = "IMDCT", dict(window_length=w, row_align=32), np.float32, "execute_imdct_ragged", "k_imdct_ragged"
    else:
        a = cp.window_a(w)
        blocks = [orc.stft(synth_clip(95, i, cp.stft_n(w, hop, t) if t > 1 else 0).astype(np.float64), a, hop).astype(np.complex64) for i, t in enumerate(FRAMES)]
        ref = lambda c: [orc.istft(b.astype(np.complex128), c["window"], hop) for b in blocks]
        sizes = [max(t * hop - (w - hop), 0) for t in FRAMES]
        plan_kind, kw, dtype, name, kernel = "ISTFT", dict(window_length=w, step_length=hop, row_align=16), np.complex64, "execute_istft_ragged", "k_istft_ragged"
    assert [b.shape[1] for b in blocks] == list(FRAMES)
    out_off, total = out_places(sizes)
    frames_a = np.array(FRAMES, np.int64)

    def bind(plan):
        packed = [cp.rows_with_nan_pads(b[None], plan.row_pitch(t), dtype)[0] for b, t in zip(blocks, FRAMES)]
        flat, in_off = with_gaps(packed, dtype)
        keep = np.zeros(total, bool)
        for o, n in zip(out_off.tolist(), sizes):
            keep[o:o + n] = True
        return dict(x=flat, out_shape=(total,), launch=lambda p, d_in, d_out: getattr(p, name)(d_in, in_off, frames_a, d_out, out_off),
                    split=lambda out: [out[o:o + n] for o, n in zip(out_off.tolist(), sizes)], keep=keep)
    return cp.Case(plan_kind, kw, {"window": a}, ref, bind, cp.TOL_FFT, kernel, {"b": [("window", cp.win.skew(w))]})


def ragged_center():
    """execute_center_ragged at W = 2048: stereo clips of LENGTHS sample frames, center and sides."""
    w = 2048
    xs = [cp.stereo(3 * w + c, n) for c, n in enumerate(LENGTHS)]
    flat, in_floats = with_gaps(xs, np.float32, unit=2)
    out_off, total = out_places([2 * n for n in LENGTHS])
    lens = np.array(LENGTHS, np.int64)

    def bind(plan):
        keep = np.zeros((total, 2), bool)
        for o, n in zip(out_off.tolist(), LENGTHS):
            keep[o:o + 2 * n] = True
        return dict(x=flat, out_shape=(total, 2), launch=lambda p, d_in, d_out: p.execute_center_ragged(d_in, in_floats // 2, lens, d_out, out_off),
                    split=lambda out: [out[o:o + 2 * n].reshape(2, n, 2) for o, n in zip(out_off.tolist(), LENGTHS)], keep=keep)
    from center_oracle import TOL_CENTER
    return cp.Case("CENTER_SIDES", dict(window_length=w, step_length=w // 2), {"window": cp.window_a(w)}, lambda c: cp.center_refs(xs, c["window"], True), bind,
                   TOL_CENTER, "k_center_ragged", {"b": [("window", cp.win.skew(w))]}, err=cp.center_err(True))


RAGGED = {
    "mel_execute_ragged": lambda: ragged_forward("mel"),
    "mdct_execute_ragged": lambda: ragged_forward("mdct"),
    "imdct_ragged": lambda: ragged_inverse("imdct"),
    "istft_ragged": lambda: ragged_inverse("istft"),
    "center_ragged": ragged_center,
    "mel_execute_ragged_pcm": lambda: ragged_forward("mel", pcm=True),
    "mdct_f64_execute_ragged": lambda: ragged_forward("mdct", f64=True),
}


@pytest.mark.parametrize("entry", sorted(RAGGED))
def test_ragged_entry_points_on_a_reused_plan(zafx, entry):
    """Clips of 0, 1, 3072 and 16 x 1024 + 3 samples (or the matching frame counts) through a ragged entry point after the plan's constants
    were replaced: the oracle's results on B, the bits of the same call on a fresh plan, the same kernel; A again: step 1's bits."""
    case = RAGGED[entry]()
    steps = case.variants["b"]
    ref_a, ref_b = case.refs(None), case.refs("b")
    # (the two long clips: an empty clip has nothing to change, and the center of a one-sample clip is x (w[0] + w[H]) / gain = x under any window)
    change = min(case.err(b, a) for a, b in list(zip(ref_a, ref_b))[2:])
    assert change >= cp.MIN_CHANGE, change
    plan, fresh = case.make(), case.make(case.after(steps))
    d_in = None
    try:
        bound = case.bind(plan)
        d_in = zafx.DeviceBuffer.from_host(bound["x"])
        out_1 = run(zafx, plan, bound, d_in)
        assert plan.last_kernel == case.kernel, plan.last_kernel
        check(case, bound, out_1, ref_a, f"{entry} A")
        cp.upload(plan, steps)
        out_2 = run(zafx, plan, bound, d_in)
        check(case, bound, out_2, ref_b, f"{entry} B")
        assert same_bits(out_2, run(zafx, fresh, bound, d_in))
        assert plan.last_kernel == fresh.last_kernel == case.kernel
        cp.upload(plan, case.restore(steps))
        assert same_bits(run(zafx, plan, bound, d_in), out_1), "A again does not give step 1's bits"
    finally:
        if d_in is not None:
            d_in.free()
        plan.destroy()
        fresh.destroy()


# ------------------------------------------------------------------------------------------------ refused uploads
def expect_refusal(zafx, plan, which, array, dtype):
    with pytest.raises(zafx.ZafxError) as e:
        plan._set(which, array, dtype)
    assert len(str(e.value)) > len("zafx_plan_set_constant"), "a refusal says why"


@pytest.mark.parametrize("route", ["mel2_mfcc", "mfcc_f64", "mdct_ft32", "linear"])
def test_refused_uploads_leave_the_plan_as_it_was(zafx, route):
    """A plan that has run refuses a buffer one element short for every constant it takes and every constant id it does not take, each with
    a message; after each refusal execute gives step 1's bits."""
    L = cp.lib()
    case = cp.case(route)
    plan = case.make()
    real = np.float64 if plan.f64 else np.float32
    ids = {"window": L.CONST_WINDOW, "fb": L.CONST_MEL_FB, "dct": L.CONST_DCT, "matrix": L.CONST_MATRIX}
    d_in = None
    try:
        bound = case.bind(plan)
        d_in = zafx.DeviceBuffer.from_host(bound["x"])
        out_1 = run(zafx, plan, bound, d_in)
        for key, value in case.consts.items():
            expect_refusal(zafx, plan, ids[key], np.asarray(value).reshape(-1)[:-1], real)
            assert same_bits(run(zafx, plan, bound, d_in), out_1), key
        for which in (L.CONST_WINDOW, L.CONST_MEL_FB, L.CONST_DCT, L.CONST_MATRIX, L.CONST_CQT_INDPTR, L.CONST_CQT_INDICES, L.CONST_CQT_VALUES):
            if which in [ids[k] for k in case.consts]:
                continue
            expect_refusal(zafx, plan, which, np.zeros(16, np.float32), np.float32)
            assert same_bits(run(zafx, plan, bound, d_in), out_1), which
        expect_refusal(zafx, plan, 99, np.zeros(16, np.float32), np.float32)
        assert same_bits(run(zafx, plan, bound, d_in), out_1)
    finally:
        if d_in is not None:
            d_in.free()
        plan.destroy()


@pytest.mark.parametrize("route", ["cqt_8192", "cqt_f64"])
def test_refused_cqt_uploads_leave_the_plan_as_it_was(zafx, route):
    """The CQT kernel's three arrays on a plan that has run.  indptr has a fixed length (n_bins + 1): one element short is refused.  indices
    and values have the length the three arrays agree on, which an upload of one of them cannot know (a kernel of another nnz arrives array by
    array), so a buffer one element short is refused where the disagreement shows: execute says the CSR arrays are inconsistent and writes
    nothing, and the plan takes the whole array again.  An indices array with one column equal to fft_length is refused at the upload and
    changes nothing.  A good values upload afterwards -- one that marks the packed tables for rebuild -- matches a fresh plan."""
    L = cp.lib()
    case = cp.case(route)
    ck = case.consts["cqt"]
    cplx = np.complex128 if case.kw["f64"] else np.complex64
    plan = case.make()
    d_in = None
    try:
        bound = case.bind(plan)
        d_in = zafx.DeviceBuffer.from_host(bound["x"])
        out_1 = run(zafx, plan, bound, d_in)
        check(case, bound, out_1, case.refs(None), f"{route} A")
        expect_refusal(zafx, plan, L.CONST_CQT_INDPTR, ck.indptr[:-1], np.int32)
        assert same_bits(run(zafx, plan, bound, d_in), out_1)
        bad = ck.indices.copy()
        bad[len(bad) // 2] = ck.shape[1]
        expect_refusal(zafx, plan, L.CONST_CQT_INDICES, bad, np.int32)
        assert same_bits(run(zafx, plan, bound, d_in), out_1)
        for which in (L.CONST_WINDOW, L.CONST_MEL_FB, L.CONST_DCT, L.CONST_MATRIX, 99):
            expect_refusal(zafx, plan, which, np.zeros(16, np.float32), np.float32)
        assert same_bits(run(zafx, plan, bound, d_in), out_1)
        for which, whole, dtype in ((L.CONST_CQT_INDICES, ck.indices, np.int32), (L.CONST_CQT_VALUES, ck.data, cplx)):
            plan._set(which, whole[:-1], dtype)
            message, untouched = refused(zafx, plan, bound, d_in)
            assert message is not None and "inconsistent" in message and untouched, (which, message, untouched)
            plan._set(which, whole, dtype)
            assert same_bits(run(zafx, plan, bound, d_in), out_1), which
        steps = case.variants["values"]
        cp.upload(plan, steps)
        fresh = case.make(case.after(steps))
        try:
            out_2 = run(zafx, plan, bound, d_in)
            check(case, bound, out_2, case.refs("values"), f"{route} values")
            assert same_bits(out_2, run(zafx, fresh, bound, d_in))
        finally:
            fresh.destroy()
    finally:
        if d_in is not None:
            d_in.free()
        plan.destroy()


# ------------------------------------------------------------------------------------------------ the fused mask filters on a reused plan
# Every mask-filter kernel whose own module has no A -> B -> A (k_maskfilter and k_maskfilter_stems have:
# test_window_replaced_on_a_used_plan): they share check_window_gain and the plan's cola_gain through zafx_overlap_walk.hpp, and each reads
# the window on its own.  (form of tests/maskfilter_cases.py, ragged, the PCM entry points' output type or None for the float32 ones)
MASKFILTER_SWAPS = [("tf", True, None), ("stems", True, None), ("complex", False, None), ("complex", True, None),
                    ("stereo1", False, None), ("stereo1", True, None), ("stereo2", False, None), ("stereo2", True, None)]
MASKFILTER_SWAPS += [(form, ragged, out) for form in ("tf", "stereo1", "stereo2") for ragged in (False, True) for out in (np.int16, np.float32)]
PCM_SCALE = 4096   # unit noise as int16 with peaks near 18000: under masks in [0, 1] the reference stays inside the int16 range (asserted)


def _swap_id(v):
    form, ragged, out = v
    return f"{form}{'_pcm_' + np.dtype(out).name if out else ''}{'_ragged' if ragged else ''}"


@pytest.mark.parametrize("wl", [2048, 256])
@pytest.mark.parametrize("swap_case", MASKFILTER_SWAPS, ids=_swap_id)
def test_maskfilter_window_replaced_on_a_used_plan(zafx, swap_case, wl):
    """A = periodic Hamming, B = tests/windows.py's skew, on a private MASKFILTER_REST plan, three clips of 9 H + 3 under "unit" / "disc" masks:
    every step against the float64 oracle under its window (mask_error <= TOL_FFT, a stereo form's level over both channels; an int16 output
    within 0.5 LSB + 32768 x the per-hop bound, its rest clip(x - y_q) in integers); B has the bits and the last_kernel of a fresh plan made
    with B; A again has step 1's bits; then A with w[0] = -w[H] is refused in the reference's words and leaves the filled output as it was,
    and A once more has step 1's bits.  Before any launch: B's reference differs from A's by MIN_CHANGE or more in every row of every clip."""
    import maskfilter_cases as mc
    import maskfilter_run as mr
    import windows as win
    from test_gpu_maskfilter_pcm import int_rest
    form, ragged, out = swap_case
    h = wl // 2
    n = 9 * h + 3
    data, tail = mc.data_of(form), mc.rest_rows(form)
    windows = {"a": cp.window_a(wl), "b": win.skew(wl)}
    batches = {tag: mc.batch(data, wl, n, name, "unit") for tag, name in (("a", "hamming"), ("b", "skew"))}
    clips, masks = batches["a"]["clips"], batches["a"]["masks"]
    assert all(np.array_equal(x, y) for x, y in zip(clips, batches["b"]["clips"])) and len(clips) == 3
    if out is None:
        refs = {tag: batches[tag]["refs"] for tag in windows}
    else:
        pcm = [mc.to_int16(x, PCM_SCALE) for x in clips]
        clips = [mc.normalised(q) for q in pcm]
        refs = {tag: [mc.reference(data, xn, w, m) for xn, m in zip(clips, masks)] for tag, w in windows.items()}
    for ra, rb in zip(refs["a"], refs["b"]):   # teeth, on the host
        change = min(relerr(rb[j], ra[j]) for j in range(len(ra)))
        assert change >= cp.MIN_CHANGE, (form, wl, change)
    bounds = None
    if out == np.int16:
        bounds = {tag: [mc.int16_bound(r[:tail], xn, h) for r, xn in zip(refs[tag], clips)] for tag in windows}
        for tag in windows:
            for r, b in zip(refs[tag], bounds[tag]):
                assert (np.abs(32768.0 * r[:tail]) + b < 32767).all(), (form, wl, tag, "the reference leaves the int16 range")

    def make(w):
        p = zafx.Plan(zafx.MASKFILTER_REST, window_length=wl, step_length=h, layout="TF")
        p.set_window(w)
        return p

    def go(plan, refusal=None):
        if out is None:
            return mr.run(form, None, clips, masks, True, ragged, plan=plan, refusal=refusal)
        return mr.run_pcm(form, None, pcm, masks, True, ragged, out, plan=plan, refusal=refusal)

    def held(res, tag):
        worst = 0.0
        for i, (r, ref, x) in enumerate(zip(res, refs[tag], clips)):
            assert r.shape == ref.shape and np.isfinite(r).all(), (form, wl, tag, i)
            if out == np.int16:
                share = excess(r[:tail].astype(np.float64), 32768.0 * ref[:tail], bounds[tag][i])
                assert share <= 1.0, (form, wl, tag, i, "int16 out against the oracle", share)
                planar = pcm[i].T if pcm[i].ndim == 2 else pcm[i][None]
                assert np.array_equal(r[tail:], int_rest(planar, r[:tail])), (form, wl, tag, i, "rest")
                worst = max(worst, share)
            else:
                for j in range(len(r)):
                    err = mc.mask_error(r[j], ref[j], mc.row_level(ref, x, j, tail))
                    assert err <= cp.TOL_FFT, (form, wl, tag, i, j, err)
                    worst = max(worst, err)
        print(f"{_swap_id(swap_case)} W={wl} {tag.upper()}: worst {'share of the int16 bound' if out == np.int16 else 'mask_error'} {worst:.3g}")

    same = lambda p, q: len(p) == len(q) and all(same_bits(a, b) for a, b in zip(p, q))   # noqa: E731
    fresh = make(windows["b"])
    used = make(windows["a"])
    try:
        out_f, kernel_f = go(fresh), fresh.last_kernel
        out_1 = go(used)
        held(out_1, "a")
        used.set_window(windows["b"])
        out_2 = go(used)
        held(out_2, "b")
        assert same(out_2, out_f) and used.last_kernel == kernel_f and not same(out_2, out_1), (form, wl, used.last_kernel, kernel_f)
        used.set_window(windows["a"])
        assert same(go(used), out_1), (form, wl, "A again")
        used.set_window(cp.window_zero_gain(wl, h))
        assert go(used, refusal="sum(window[0:W:H]) is zero") is None
        used.set_window(windows["a"])
        assert same(go(used), out_1), (form, wl, "A after the refused window")
    finally:
        fresh.destroy()
        used.destroy()
