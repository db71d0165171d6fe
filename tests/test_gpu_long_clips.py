"""Every launcher route at and beyond its long-clip bound (-m gpu): one clip just below and one just above each record of
long_clips.BOUNDS -- the lengths at which a launcher leaves the kernel that addresses a clip with 32-bit byte offsets for another kernel,
another instantiation, or a refusal.

The clip is periodic (long_clips.period_block: noise plus a tone, period 7 hops) and built on the device; the float64 oracle of the whole
result is long_clips.periodic_reference -- three short oracle results and an index, which tests/test_long_clips_host.py holds to the plain
oracle.  Every call's kernel is asserted by name (the table is read off the dispatch code, not off last_kernel), the output is prefilled with
the arena's fill, and EVERY output element is compared: each frame (hop of samples) against a bound of its own, tol max|ref frame| +
C eps32 max|ref| (long_clips: tol 1e-5 for the transforms, 1e-4 for filterbanks and CQT), fill left inside or padding written fail at their
index.  A refusal must raise ZafxError, name its limit, and leave every word of the output at the fill.

Sizes are intrinsic -- 2^31 bytes is the smallest clip in which a signed 32-bit byte offset can wrap --, everything else is small: one clip, a
period of 28 KB, the oracle on some twenty frames.  Every case frees its buffers; the largest hold 8.6 GB on the device at their peak (two arrays of 4.3 GB: the IMDCT at W = 2048, the float64 MDCT / IMDCT and mel cases).  A case over 10 s is split by kind.  The wall time of
each case, measured once, is in profiles/long_clips_times.json (ZAFX_LONG_CLIPS_TIMES=<path> writes it)."""
import ctypes
import json
import os
import time

import numpy as np
import pytest

import long_clips as lc
from center_oracle import C_CENTER

pytestmark = pytest.mark.gpu

_times = {}


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    yield z
    z.DeviceBuffer.drain_pool()
    path = os.environ.get("ZAFX_LONG_CLIPS_TIMES")
    if path:
        known = {}
        if os.path.exists(path):
            with open(path) as f:
                known = json.load(f)
        known.update(_times)
        with open(path, "w") as f:
            json.dump(known, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def consts(zafx):
    c = dict(ck=zafx.cqtkernel(lc.FS, 24, 55, 3520))
    c["fb", 2048], c["fb", 4096] = zafx.melfilterbank(lc.FS, 2048, 128), zafx.melfilterbank(lc.FS, 4096, 128)
    for w in (2048, 4096, 8192):
        c["ham", w], c["kbd", w] = zafx.hamming(w), zafx.kaiser_bessel_derived(w)
    return c


@pytest.fixture
def timed(request):
    t0 = time.perf_counter()
    yield
    _times[request.node.name] = round(time.perf_counter() - t0, 2)


def parameters(b, c):
    """(oracle parameters, period step, channels) of a BOUNDS record."""
    kind = b["kind"]
    if kind in ("cqt", "chroma"):
        return dict(fs=lc.FS, tr=25, ck=c["ck"], octave=24), b["hop"], 1
    if kind in ("mdct", "imdct"):
        return dict(w=c["kbd", b["W"]]), b["hop"], 1
    prm = dict(w=c["ham", b["W"]], hop=b["hop"])
    if kind in ("mel", "mfcc", "mel_mfcc"):
        prm.update(fb=c["fb", b["W"]], ncoef=20)
    return prm, b["hop"], 2 if kind == "center" else 1


def forward_plan(zafx, b, c):
    kind, hop, a = b["kind"], b["hop"], b["options"].get("row_align", 0)
    spectrum = {"stft": False, "istft": False, "stft_one_sided": True, "istft_one_sided": True, "magnitude": "magnitude", "power": "power"}
    if kind in spectrum:
        return zafx.stft_plan(c["ham", b["W"]], hop, onesided=spectrum[kind], row_align=a)
    if kind in ("mdct", "imdct"):
        return zafx.mdct_plan(c["kbd", b["W"]], row_align=a)
    if kind in ("mel", "mfcc", "mel_mfcc"):
        return zafx.mel_plan(c["ham", b["W"]], hop, c["fb", b["W"]], None if kind == "mel" else 20, also_mel=kind == "mel_mfcc")
    if kind in ("cqt", "chroma"):
        return zafx.cqt_plan(lc.FS, 25, c["ck"], octave_resolution=24 if kind == "chroma" else None)
    return zafx.center_plan(c["ham", b["W"]], sides=b["options"]["sides"])


def inverse_plan(zafx, b, c):
    a = b["options"].get("row_align", 0)
    if b["kind"] == "imdct":
        return zafx.mdct_plan(c["kbd", b["W"]], inverse=True, row_align=a)
    return zafx.istft_plan(c["ham", b["W"]], b["hop"], onesided=b["kind"] == "istft_one_sided", row_align=a)


def row_parts(kind, rows):
    """The rows that share a per-frame bound: mel bands and coefficients of the one-pass plan are held to their own levels."""
    return [(0, 128), (128, rows)] if kind == "mel_mfcc" else [(0, rows)]


def check_forward(zafx, plan, d_x, n, kind, ref, want_kernel, tag, pcm=False):
    """execute (execute_pcm on int16 mono) on a prefilled output, the kernel's name, every element: -> the output buffer (the caller frees it)."""
    _, rows, pitch = plan.out_shape(1, n)
    assert (rows, plan.out_dims(n)[1]) == (ref.rows, ref.frames), (tag, rows, plan.out_dims(n), ref.rows, ref.frames)
    d_out = lc.device_filled(zafx, (1, rows, pitch), plan.out_dtype)
    try:
        if pcm:
            plan.execute_pcm(d_x, d_out, 1, n, 1)
        else:
            plan.execute(d_x, d_out, 1, n)
        plan.sync()
        assert plan.last_kernel == want_kernel, (tag, plan.last_kernel, want_kernel)
        for r0, r1 in row_parts(kind, rows):
            part = lc.PeriodicRef(ref.small[r0:r1], ref.idx, ref.first, ref.last, ref.q)
            worst = lc.walk_frames(zafx, d_out, rows, pitch, part, lc.TOL[kind], lc.floor_of(kind, part), part=(r0, r1))
            print(f"{tag}: rows {r0}:{r1} of {rows} x {ref.frames} (pitch {pitch}), {plan.last_kernel}, worst frame at {worst:.3f} of its bound")
    except BaseException:
        d_out.free()
        raise
    return d_out


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("name", lc.BOUND_NAMES)
def test_bound(zafx, consts, timed, name, side):
    run_bound(zafx, consts, name, side)


SPLIT = [b["name"] for b in lc.BOUNDS if b["options"].get("split")]


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("name", SPLIT)
def test_bound_input(zafx, consts, timed, name, side):
    """The records whose case would take more than 10 s, split by kind: the forward launch that makes the inverse's input, checked here alone
    (4 GiB of coefficients); test_bound takes the same launch's result unchecked and checks the inverse."""
    run_bound(zafx, consts, name, side, input_only=True)


def run_bound(zafx, consts, name, side, input_only=False):
    b = lc.bound(name)
    kind = b["kind"]
    n = b["n_below"] if side == "below" else b["n_above"]
    want = b["kernel_below"] if side == "below" else b["above"]
    tag = f"{name}.{side}"
    prm, step, channels = parameters(b, consts)
    pcm = bool(b["options"].get("pcm"))
    p = lc.period_block(step, channels=channels, dtype=np.int16 if pcm else np.float32)
    plan = forward_plan(zafx, b, consts)
    d_x = lc.device_clip(zafx, p, n)
    d_mid = d_out = None
    try:
        if want == "refused":
            d_out = lc.device_filled(zafx, plan.out_shape(1, n), plan.out_dtype)
            with pytest.raises(zafx.ZafxError) as e:
                plan.execute(d_x, d_out, 1, n)
                plan.sync()
            assert {"cqt": "2^29", "chroma": "2^29", "center": "2^28"}[kind] in str(e.value), str(e.value)
            plan.sync()
            lc.assert_untouched(zafx, d_out)
            return
        if kind == "center":
            sides = b["options"]["sides"]
            d_out = lc.device_filled(zafx, plan.out_shape(1, n), np.float32)
            plan.execute(d_x, d_out, 1, n)
            plan.sync()
            assert plan.last_kernel == want, (tag, plan.last_kernel)
            floor = C_CENTER * lc.EPS32 * float(np.abs(p).max())
            for block, what in enumerate(("center", "sides")[:2 if sides else 1]):   # (ZAFX_CENTER_SIDES: the sides' block directly behind the center's)
                ref = lc.periodic_reference(kind, p.astype(np.float64), n, sides=block == 1, **prm)
                worst = lc.walk_hops(zafx, d_out, 2 * n, ref, lc.TOL[kind], floor, offset=block * 2 * n)
                print(f"{tag}: {what}, {ref.frames} hops, {plan.last_kernel}, worst hop at {worst:.3f} of its bound")
            return
        if kind in lc.FRAMED:
            ref = lc.periodic_reference(kind, p / 32768.0 if pcm else p, n, **prm)   # (wavread's normalisation, zaf.py:1202)
            d_out = check_forward(zafx, plan, d_x, n, kind, ref, want, tag, pcm)
            return
        # the inverse transforms: the spectrum of the periodic clip from a forward launch (checked first), then the inverse of that
        fkind = {"istft": "stft", "istft_one_sided": "stft_one_sided", "imdct": "mdct"}[kind]
        spectrum = lc.periodic_reference(fkind, p, n, **prm)
        _, rows, pitch = plan.out_shape(1, n)
        d_mid = lc.device_filled(zafx, (1, rows, pitch), plan.out_dtype)
        plan.execute(d_x, d_mid, 1, n)
        plan.sync()
        d_x.free()
        if input_only or not b["options"].get("split"):   # (a record split by kind: test_bound_input checks this launch's result)
            worst = lc.walk_frames(zafx, d_mid, rows, pitch, spectrum, lc.TOL[fkind], lc.floor_of(fkind, spectrum))
            print(f"{tag}: the input, {rows} x {spectrum.frames} (pitch {pitch}) from {plan.last_kernel}, worst frame at {worst:.3f} of its bound")
        if input_only:
            return
        # (the row padding of the input keeps the fill, a NaN: the 16-byte gather may read it and must not use it)
        ref = lc.inverse_reference(kind, spectrum, **prm)
        inv = inverse_plan(zafx, b, consts)
        assert inv.row_pitch(spectrum.frames) == pitch and inv.out_shape(1, spectrum.frames) == (1, ref.n_out)
        d_out = lc.device_filled(zafx, (1, ref.n_out), np.float32)
        inv.execute(d_mid, d_out, 1, spectrum.frames)
        inv.sync()
        assert inv.last_kernel == want, (tag, inv.last_kernel, want)
        worst = lc.walk_hops(zafx, d_out, ref.n_out, ref, lc.TOL[kind], lc.floor_of(kind, ref))
        print(f"{tag}: {ref.n_out} samples in {ref.frames} hops, {inv.last_kernel}, worst hop at {worst:.3f} of its bound")
    finally:
        for buf in (d_x, d_mid, d_out):
            if buf is not None:
                buf.free()


# ------------------------------------------------------------------------------------------------------------ ragged batches
# A batch of three clips: the middle one just below, then just above, the length at which the ragged entry point leaves its one launch
# (zafx_capi.cpp:execute_ragged_checked, zafx_execute_center_ragged); the two neighbours are short and must have, bit for bit, what the
# equal-length launch gives each of them alone.  (name, kind, W, hop, n_below, n_above, kernel_below, above)
RAGGED = [
    ("stft_ragged_magnitude", "magnitude", 2048, 2048, (1 << 29) - 2, 1 << 29, "k_mel2_ragged", "per-clip k_mel2"),   # lengths[i] < 2^29 (k_mel2's descriptor)
    # int16 mono (zafx_execute_ragged_pcm): the integers in k_mel2_ragged's loads below; above, the clips are converted group by group into the
    # plan's staging array (rg_pcm_groups: a group stays within the scratch budget, so the long clip is a group of its own) and each group runs
    # zafx_execute_ragged -- the last group is the short last clip, one launch of k_mel2_ragged, which is what last_kernel names
    ("stft_pcm16_ragged_magnitude", "magnitude", 2048, 2048, (1 << 29) - 2, 1 << 29, "k_mel2_ragged", "k_mel2_ragged"),
    ("mdct_ragged", "mdct", 2048, 1024, (1 << 28) - 4, 1 << 28, "k_mdct_ft32_ragged", "per-clip k_mdct_ft32"),       # n_samples < 2^28, multiples of 4
    ("centersides_ragged", "center", 2048, 1024, (1 << 28) - 1, 1 << 28, "k_center_ragged", "refused"),              # lengths[i] < 2^28 sample frames
]
SHORT = (3 * 1024 + 8, 70 * 1024 + 300)   # the neighbours: 4 frames; several tiles and an edge tile


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("case", RAGGED, ids=[r[0] for r in RAGGED])
def test_ragged_middle_clip(zafx, consts, timed, case, side):
    name, kind, w, hop, n_below, n_above, kernel_below, above = case
    n = n_below if side == "below" else n_above
    want = kernel_below if side == "below" else above
    tag = f"{name}.{side}"
    stereo, pcm = kind == "center", "pcm16" in name
    dtype = np.int16 if pcm else np.float32
    p = lc.period_block(hop, channels=2 if stereo else 1, dtype=dtype)
    shorts = [np.ascontiguousarray(lc.periodic_clip(lc.period_block(hop, seed=s, channels=2 if stereo else 1, dtype=dtype), k)) for s, k in zip((1, 2), SHORT)]
    scale = 1.0 / 32768.0 if pcm else 1.0   # (wavread's normalisation, zaf.py:1202)
    if kind == "magnitude":
        plan, prm = zafx.stft_plan(consts["ham", w], hop, onesided="magnitude", row_align=32), dict(w=consts["ham", w], hop=hop)
    elif kind == "mdct":
        plan, prm = zafx.mdct_plan(consts["kbd", w], row_align=32), dict(w=consts["kbd", w])
    else:
        plan, prm = zafx.center_plan(consts["ham", w], sides=False), dict(w=consts["ham", w])
    d_in, in_off, lengths = lc.device_ragged(zafx, [shorts[0], (p, n), shorts[1]])
    d_out = None
    try:
        if stereo:
            out_off = in_off.copy()   # (the center of a clip is as long as the clip: the same slots)
            d_out = lc.device_filled(zafx, d_in.shape, np.float32)
            launch = lambda: plan.execute_center_ragged(d_in, in_off, lengths, d_out, out_off)
            blocks = [((int(k), 2), int(o) * 2) for k, o in zip(lengths, out_off)]
        else:
            offs, frames, pitch = plan.ragged_layout(lengths)
            rows = plan.out_dims(int(lengths[0]))[0]
            d_out = lc.device_filled(zafx, (int(offs[-1]),), plan.out_dtype)
            launch = (lambda: plan.execute_ragged_pcm(d_in, in_off, lengths, d_out, 1)) if pcm else (lambda: plan.execute_ragged(d_in, in_off, lengths, d_out))
            blocks = [((rows, int(tp)), int(o)) for tp, o in zip(pitch, offs)]
        if want == "refused":
            with pytest.raises(zafx.ZafxError) as e:
                launch()
            assert "2^28" in str(e.value), str(e.value)
            plan.sync()
            lc.assert_untouched(zafx, d_out)
            return
        launch()
        plan.sync()
        assert plan.last_kernel == want, (tag, plan.last_kernel, want)
        # the middle clip: every element
        ref = lc.periodic_reference(kind, p.astype(np.float64) * scale, n, **prm)
        if stereo:
            worst = lc.walk_hops(zafx, d_out, 2 * n, ref, lc.TOL[kind], C_CENTER * lc.EPS32 * float(np.abs(p).max()), offset=blocks[1][1])
        else:
            assert int(frames[1]) == ref.frames and blocks[1][0][0] == ref.rows
            worst = lc.walk_frames(zafx, d_out, ref.rows, blocks[1][0][1], ref, lc.TOL[kind], lc.floor_of(kind, ref), offset=blocks[1][1])
        print(f"{tag}: the middle clip of {n}, {plan.last_kernel}, worst frame at {worst:.3f} of its bound")
        # the neighbours: the bits of the equal-length launch (row padding included: the fill on both sides)
        got = [lc.download_block(zafx, d_out, *blocks[i]) for i in (0, 2)]
        for x, g, (shape, _) in zip(shorts, got, (blocks[0], blocks[2])):
            d_x = zafx.DeviceBuffer.from_host(x)
            d_one = lc.device_filled(zafx, (1,) + shape, plan.out_dtype)
            try:
                if pcm:
                    plan.execute_pcm(d_x, d_one, 1, len(x), 1)
                else:
                    plan.execute(d_x, d_one, 1, len(x))
                plan.sync()
                alone = d_one.download()[0]
            finally:
                d_x.free()
                d_one.free()
            assert np.array_equal(g.view(np.uint32), alone.view(np.uint32)), (tag, len(x), "a neighbour differs from its equal-length result")
            full = lc.plain_oracle(kind, x.astype(np.float64) * scale, **prm)   # (and those bits are the clip's own result, not the fill twice)
            val = g.reshape(-1) if stereo else g[:, :full.shape[1]]
            if stereo:
                full = full.T.reshape(-1)[:2 * len(x)]
            assert val.shape == full.shape and np.abs(val - full).max() <= lc.TOL[kind] * np.abs(full).max(), (tag, len(x))
    finally:
        d_in.free()
        if d_out is not None:
            d_out.free()


# The inverse entry points (zafx_capi.cpp: kIstftRagged, kImdctRagged): three blocks of spectra / coefficients, the middle one just below and just
# above the size a block may have in the one launch -- W pitch 8 < 2^31 bytes (ISTFT), W / 2 pitch 4 < 2^32 bytes (IMDCT) --; above it the call
# runs one execute per block and last_kernel is the last (short) block's kernel.  The blocks come from forward launches of the periodic clip
# (the middle one checked first); the neighbours must have the bits of their equal-length inverse.
RAGGED_INVERSE = [
    ("istft_ragged", "istft", 16, 131056, 131057, "k_istft_ragged", "k_istft_ft16"),
    ("imdct_ragged", "imdct", 32, (1 << 20) - 32, (1 << 20) - 31, "k_imdct_ragged", "k_imdct"),
]


# (the IMDCT case, 4 GiB in and 4 GiB out, is split by kind: "input" checks the middle block the forward launch wrote, "output" the inverse)
RAGGED_INVERSE_PARTS = [(RAGGED_INVERSE[0], "both"), (RAGGED_INVERSE[1], "input"), (RAGGED_INVERSE[1], "output")]


@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("case,part", RAGGED_INVERSE_PARTS, ids=[f"{r[0]}-{part}" for r, part in RAGGED_INVERSE_PARTS])
def test_ragged_inverse_middle_block(zafx, consts, timed, case, part, side):
    name, kind, align, t_below, t_above, kernel_below, above = case
    frames_mid = t_below if side == "below" else t_above
    want = kernel_below if side == "below" else above
    tag, hop, w = f"{name}.{side}", 1024, 2048
    if kind == "istft":
        prm, fkind = dict(w=consts["ham", w], hop=hop), "stft"
        fwd, inv = zafx.stft_plan(prm["w"], hop, row_align=align), zafx.istft_plan(prm["w"], hop, row_align=align)
        rows, limit = w, (w * 8, 1 << 31)
    else:
        prm, fkind = dict(w=consts["kbd", w]), "mdct"
        fwd, inv = zafx.mdct_plan(prm["w"], row_align=align), zafx.mdct_plan(prm["w"], inverse=True, row_align=align)
        rows, limit = w // 2, (w // 2 * 4, 1 << 32)
    p = lc.period_block(hop)
    lengths = [SHORT[0] // hop * hop, hop * (frames_mid - 1), SHORT[1] // hop * hop]   # (whole hops: T = n / hop + 1 for both transforms)
    clips = [lc.periodic_clip(lc.period_block(hop, seed=1), lengths[0]), None, lc.periodic_clip(lc.period_block(hop, seed=2), lengths[2])]
    frames = [fwd.out_dims(n)[1] for n in lengths]
    pitch = [fwd.row_pitch(n) for n in lengths]
    assert frames[1] == frames_mid and (limit[0] * pitch[1] < limit[1]) == (side == "below"), (frames, pitch)
    in_off = np.concatenate([[0], np.cumsum([rows * tp for tp in pitch])]).astype(np.int64)
    out_len = [inv.out_shape(1, t)[1] for t in frames]
    out_off = np.concatenate([[0], np.cumsum([-(-k // 32) * 32 for k in out_len])]).astype(np.int64)
    d_spec = lc.device_filled(zafx, (int(in_off[-1]),), fwd.out_dtype)
    d_out = None
    try:
        for i, n in enumerate(lengths):   # the blocks: a forward launch each, into its place
            d_x = lc.device_clip(zafx, p, n) if clips[i] is None else zafx.DeviceBuffer.from_host(clips[i])
            view = lc._view(zafx, d_spec, (1, rows, pitch[i]), int(in_off[i]))
            try:
                fwd.execute(d_x, view, 1, n)
                fwd.sync()
            finally:
                view.ptr = ctypes.c_void_p()
                d_x.free()
        spectrum = lc.periodic_reference(fkind, p, lengths[1], **prm)
        if part != "output":
            worst = lc.walk_frames(zafx, d_spec, rows, pitch[1], spectrum, lc.TOL[fkind], lc.floor_of(fkind, spectrum), offset=int(in_off[1]))
            print(f"{tag}: the middle block, {rows} x {frames[1]} (pitch {pitch[1]}), worst frame at {worst:.3f} of its bound")
        if part == "input":
            return
        d_out = lc.device_filled(zafx, (int(out_off[-1]),), np.float32)
        entry = inv.execute_istft_ragged if kind == "istft" else inv.execute_imdct_ragged
        entry(d_spec, in_off[:3], np.array(frames, np.int64), d_out, out_off[:3])
        inv.sync()
        assert inv.last_kernel == want, (tag, inv.last_kernel, want)
        ref = lc.inverse_reference(kind, spectrum, **prm)
        assert ref.n_out == out_len[1]
        worst = lc.walk_hops(zafx, d_out, out_len[1], ref, lc.TOL[kind], lc.floor_of(kind, ref), offset=int(out_off[1]))
        print(f"{tag}: the middle block's {out_len[1]} samples, {inv.last_kernel}, worst hop at {worst:.3f} of its bound")
        # nothing between the blocks' samples was written, and the neighbours have the bits of their equal-length inverse
        for i in (0, 2):
            got = lc.download_block(zafx, d_out, (int(out_off[i + 1] - out_off[i]),), int(out_off[i]))
            assert (got[out_len[i]:].view(np.uint32) == lc.arena.FILL32).all(), (tag, i, "written behind a block's samples")
            view = lc._view(zafx, d_spec, (1, rows, pitch[i]), int(in_off[i]))
            d_one = lc.device_filled(zafx, (1, out_len[i]), np.float32)
            try:
                inv.execute(view, d_one, 1, frames[i])
                inv.sync()
                alone = d_one.download()[0]
            finally:
                view.ptr = ctypes.c_void_p()
                d_one.free()
            assert np.array_equal(got[:out_len[i]].view(np.uint32), alone.view(np.uint32)), (tag, i, "a neighbour differs from its equal-length result")
            full = lc.plain_oracle(kind, clips[i].astype(np.float64), **prm).T.reshape(-1)[:out_len[i]]
            assert np.abs(alone - full).max() <= lc.TOL[kind] * np.abs(full).max(), (tag, i)
    finally:
        d_spec.free()
        if d_out is not None:
            d_out.free()


# ------------------------------------------------------------------------------------------------------------ outputs above 2^32 bytes inside one clip
# Kernels without a per-clip guard: they address the clip with pointers, and every index product has to be 64 bits wide.  One clip each whose
# output crosses 2^31 and 2^32 bytes: the float64 tiled STFT and, from its result, the float64 ISTFT (4.3 GB of complex128, 131088 frames); the
# float32 Bluestein STFT at a window that is no power of two (W = 1764, hop 441: 304497 frames of 1764 complex64 bins).
TOL_F64 = 1e-12   # the float64 kernels' bound (tests/test_gpu_signals.py: test_signal_in_float64)
EPS64 = float(np.finfo(np.float64).eps)


def test_float64_stft_and_istft_across_4_gib(zafx, consts, timed):
    w, hop, frames = consts["ham", 2048], 1024, 131088
    n = hop * (frames - 1)
    prm = dict(w=w, hop=hop)
    p = lc.period_block(hop).astype(np.float64)
    plan = zafx.stft_plan(w, hop, f64=True, row_align=8)
    inv = zafx.istft_plan(w, hop, f64=True, row_align=8)
    spectrum = lc.periodic_reference("stft", p, n, **prm)
    _, rows, pitch = plan.out_shape(1, n)
    assert (rows, pitch, spectrum.frames) == (2048, frames, frames) and rows * pitch * 16 > 1 << 32
    d_x = lc.device_clip(zafx, p, n)
    d_spec = d_y = None
    try:
        d_spec = lc.device_filled(zafx, (1, rows, pitch), np.complex128)
        plan.execute(d_x, d_spec, 1, n)
        plan.sync()
        d_x.free()
        assert plan.last_kernel == "k_stft_ft8_f64", plan.last_kernel
        worst = lc.walk_frames(zafx, d_spec, rows, pitch, spectrum, TOL_F64, lc.C_FLOOR * EPS64 * spectrum.peak)
        print(f"float64 stft: {rows} x {frames}, worst frame at {worst:.3f} of its bound")
        ref = lc.inverse_reference("istft", spectrum, **prm)
        assert inv.out_shape(1, frames) == (1, ref.n_out) and inv.row_pitch(frames) == pitch
        d_y = lc.device_filled(zafx, (1, ref.n_out), np.float64)
        inv.execute(d_spec, d_y, 1, frames)
        inv.sync()
        assert inv.last_kernel == "k_istft_ft8_f64", inv.last_kernel
        worst = lc.walk_hops(zafx, d_y, ref.n_out, ref, TOL_F64, lc.C_FLOOR * EPS64 * ref.peak)
        print(f"float64 istft: {ref.n_out} samples, worst hop at {worst:.3f} of its bound")
    finally:
        for buf in (d_x, d_spec, d_y):
            if buf is not None:
                buf.free()


def test_bluestein_stft_across_4_gib(zafx, timed):
    wl, hop = 1764, 441
    n = hop * 304496   # T = 304497 frames: 1764 x 304497 x 8 bytes = 1.0005 x 2^32
    w = zafx.hamming(wl)
    prm = dict(w=w, hop=hop)
    p = lc.period_block(hop)
    plan = zafx.stft_plan(w, hop)
    ref = lc.periodic_reference("stft", p, n, **prm)
    _, rows, pitch = plan.out_shape(1, n)
    assert (rows, plan.out_dims(n)[1]) == (ref.rows, ref.frames) == (wl, ref.frames) and rows * pitch * 8 > 1 << 32, (rows, pitch, ref.frames)
    d_x = lc.device_clip(zafx, p, n)
    d_out = None
    try:
        d_out = lc.device_filled(zafx, (1, rows, pitch), np.complex64)
        plan.execute(d_x, d_out, 1, n)
        plan.sync()
        assert plan.last_kernel == "k_stft_bs32", plan.last_kernel
        worst = lc.walk_frames(zafx, d_out, rows, pitch, ref, lc.TOL_FFT, lc.floor_of("stft", ref))
        print(f"bluestein stft: {rows} x {ref.frames}, worst frame at {worst:.3f} of its bound")
    finally:
        d_x.free()
        if d_out is not None:
            d_out.free()


# ------------------------------------------------------------------------------------------------------------ the drop-in functions
def test_drop_in_round_trip_of_51_minutes(zafx, consts, timed):
    """zafx.istft(zafx.stft(x, w, 1024), w, 1024) on a host array of 135 000 000 samples (51 minutes at 44.1 kHz): 131837 frames, rows padded to
    131840 -- past the ISTFT's 2^31-byte bound, so the inverse runs on k_istft.  The round trip returns x to 1e-5 absolute (the project's
    bound), and the spectrum passes the per-frame check.  The only case in which the host holds the clip."""
    w, hop, n = consts["ham", 2048], 1024, 135_000_000
    p = lc.period_block(hop)
    x = np.tile(p, -(-n // len(p)))[:n]
    ref = lc.periodic_reference("stft", p, n, w=w, hop=hop)
    spec = zafx.stft(x, w, hop)
    assert spec.shape == (2048, ref.frames) == (2048, 131837) and spec.dtype == np.complex128
    assert zafx.stft_plan(w, hop, row_align=16).last_kernel == "k_stft_ft16"
    ck = lc.FrameChecker(ref, lc.TOL_FFT, lc.floor_of("stft", ref))
    for r0 in range(0, 2048, 16):   # (no fill on this path: the drop-in owns its device arrays)
        ck.add(r0, spec[r0:r0 + 16])
    print(f"drop-in stft: worst frame at {ck.finish():.3f} of its bound")
    y = zafx.istft(spec, w, hop)
    assert zafx.istft_plan(w, hop, row_align=16).last_kernel == "k_istft"
    del spec
    assert y.shape[0] >= n
    worst = 0.0
    for i in range(0, n, 1 << 24):
        worst = max(worst, float(np.abs(y[i:i + (1 << 24)][:n - i] - x[i:i + (1 << 24)]).max()))
    print(f"drop-in round trip: max |istft(stft(x)) - x| = {worst:.3e}")
    assert worst <= 1e-5, worst


# ------------------------------------------------------------------------------------------------------------ float64 MDCT / IMDCT across 2^32 bytes
# 524304 frames of 1024 float64 coefficients: 4.3 GB in one clip, in and out.  Split by kind: the forward transform is checked in the first
# test, the second takes the same launch's result as its input.
F64_FRAMES = 524304


def _float64_mdct(zafx, consts):
    w, hop = consts["kbd", 2048], 1024
    n = hop * (F64_FRAMES - 1)
    p = lc.period_block(hop).astype(np.float64)
    plan = zafx.mdct_plan(w, f64=True, row_align=16)
    _, rows, pitch = plan.out_shape(1, n)
    assert (rows, pitch) == (1024, F64_FRAMES) and rows * pitch * 8 > 1 << 32
    d_x = lc.device_clip(zafx, p, n)
    try:
        d_coefs = lc.device_filled(zafx, (1, rows, pitch), np.float64)
        try:
            plan.execute(d_x, d_coefs, 1, n)
            plan.sync()
        except BaseException:
            d_coefs.free()
            raise
    finally:
        d_x.free()
    assert plan.last_kernel == "k_mdct_ft16_f64", plan.last_kernel
    return d_coefs, lc.periodic_reference("mdct", p, n, w=w), dict(w=w)


def test_float64_mdct_across_4_gib(zafx, consts, timed):
    d_coefs, spectrum, _ = _float64_mdct(zafx, consts)
    try:
        worst = lc.walk_frames(zafx, d_coefs, 1024, F64_FRAMES, spectrum, TOL_F64, lc.C_FLOOR * EPS64 * spectrum.peak)
        print(f"float64 mdct: 1024 x {F64_FRAMES}, worst frame at {worst:.3f} of its bound")
    finally:
        d_coefs.free()


def test_float64_imdct_across_4_gib(zafx, consts, timed):
    d_coefs, spectrum, prm = _float64_mdct(zafx, consts)   # (checked by test_float64_mdct_across_4_gib)
    d_y = None
    try:
        inv = zafx.mdct_plan(prm["w"], inverse=True, f64=True, row_align=16)
        ref = lc.inverse_reference("imdct", spectrum, **prm)
        assert inv.out_shape(1, F64_FRAMES) == (1, ref.n_out) and ref.n_out * 8 > 1 << 32
        d_y = lc.device_filled(zafx, (1, ref.n_out), np.float64)
        inv.execute(d_coefs, d_y, 1, F64_FRAMES)
        inv.sync()
        assert inv.last_kernel == "k_imdct_ft16_f64", inv.last_kernel
        worst = lc.walk_hops(zafx, d_y, ref.n_out, ref, TOL_F64, lc.C_FLOOR * EPS64 * ref.peak)
        print(f"float64 imdct: {ref.n_out} samples, worst hop at {worst:.3f} of its bound")
    finally:
        d_coefs.free()
        if d_y is not None:
            d_y.free()


# ------------------------------------------------------------------------------------------------------------ 2^32 bytes between clips
def test_mdct_and_imdct_batches_across_4_gib(zafx, consts, timed):
    """Two equal-length batches of 6720 clips of 160000 samples at KBD 2048: 4.35 GB of coefficients and 4.32 GB of samples, the first MDCT /
    IMDCT arrays above 2^32 bytes (clip offsets, not offsets inside a clip).  Eight distinct clips, replicated: every group of eight is
    bit-identical to the first, and the first against the oracle."""
    from oracle import zaf_oracle as orc
    w, n, clips, distinct = consts["kbd", 2048], 160000, 6720, 8
    base = np.stack([lc.periodic_clip(lc.period_block(1024, seed=10 + c), n) for c in range(distinct)])
    fwd, inv = zafx.mdct_plan(w), zafx.mdct_plan(w, inverse=True)
    shape = fwd.out_shape(clips, n)
    frames = shape[2]
    samples = inv.out_shape(clips, frames)[1]
    assert int(np.prod(shape, dtype=np.int64)) * 4 > 1 << 32 and clips * samples * 4 > 1 << 32, (shape, samples)
    d_x = lc._replicate(zafx.DeviceBuffer((clips, n), np.float32), base)
    d_coefs = d_y = None

    def groups_equal(buf, what):
        first = buf.download(0, distinct)
        assert np.isfinite(first).all(), what
        for g in range(1, clips // distinct):
            assert np.array_equal(buf.download(g * distinct, distinct).view(np.uint32), first.view(np.uint32)), (what, "group", g)
        return first

    try:
        d_coefs = lc.device_filled(zafx, shape, np.float32)
        fwd.execute(d_x, d_coefs, clips, n)
        fwd.sync()
        d_x.free()
        coefs = groups_equal(d_coefs, "mdct")
        refs = [orc.mdct(base[c].astype(np.float64), w) for c in range(distinct)]
        for c in range(distinct):
            assert np.abs(coefs[c] - refs[c]).max() <= lc.TOL_FFT * np.abs(refs[c]).max(), ("mdct", c)
        d_y = lc.device_filled(zafx, (clips, samples), np.float32)
        inv.execute(d_coefs, d_y, clips, frames)
        inv.sync()
        y = groups_equal(d_y, "imdct")
        for c in range(distinct):
            ref = orc.imdct(refs[c], w)
            assert ref.shape == y[c].shape and np.abs(y[c] - ref).max() <= lc.TOL_FFT * np.abs(ref).max(), ("imdct", c)
        print(f"between clips: {fwd.last_kernel} {shape}, {inv.last_kernel} ({clips}, {samples})")
    finally:
        for buf in (d_x, d_coefs, d_y):
            if buf is not None:
                buf.free()


# ------------------------------------------------------------------------------------------------------------ float64 mel / MFCC across 2^32 bytes
# k_mel_ft8_f64 takes any hop: at hop 128, 2^22 + 16 frames of 128 float64 mel bands are 4.3 GB in one clip, from a clip of 4.3 GB.  The MFCC
# form (20 rows) runs on the same clip: its samples cross 2^32 bytes, its output 2^29.  Bounds: those of tests/test_gpu_signals.py's float64
# mel / MFCC check (1e-12 and 1e-10), per frame.
MEL64_FRAMES, MEL64_HOP = (1 << 22) + 16, 128
TOL_F64_MFCC = 1e-10


@pytest.mark.parametrize("kind", ["mel", "mfcc"])
def test_float64_mel_across_4_gib(zafx, consts, timed, kind):
    w, fb, hop = consts["ham", 2048], consts["fb", 2048], MEL64_HOP
    n = hop * (MEL64_FRAMES - 1)
    prm = dict(w=w, hop=hop, fb=fb, ncoef=20)
    p = lc.period_block(hop).astype(np.float64)
    plan = zafx.mel_plan(w, hop, fb, None if kind == "mel" else 20, f64=True)
    ref = lc.periodic_reference(kind, p, n, **prm)
    _, rows, pitch = plan.out_shape(1, n)
    assert (rows, pitch, ref.frames) == (128 if kind == "mel" else 20, MEL64_FRAMES, MEL64_FRAMES) and n * 8 > 1 << 32
    assert kind != "mel" or rows * pitch * 8 > 1 << 32
    d_x = lc.device_clip(zafx, p, n)
    d_out = None
    try:
        d_out = lc.device_filled(zafx, (1, rows, pitch), np.float64)
        plan.execute(d_x, d_out, 1, n)
        plan.sync()
        d_x.free()
        assert plan.last_kernel == "k_mel_ft8_f64", plan.last_kernel
        worst = lc.walk_frames(zafx, d_out, rows, pitch, ref, TOL_F64 if kind == "mel" else TOL_F64_MFCC, lc.C_FLOOR * EPS64 * ref.peak)
        print(f"float64 {kind}: {rows} x {MEL64_FRAMES}, worst frame at {worst:.3f} of its bound")
    finally:
        d_x.free()
        if d_out is not None:
            d_out.free()
