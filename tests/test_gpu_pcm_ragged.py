"""Ragged batches of integer PCM on the GPU (-m gpu): int16 / int32 clips of different lengths in one call (zafx_execute_ragged_pcm).

Geometry: W = 2048, hop 1024, melfilterbank(44100, 2048, 128), 20 coefficients, KBD 2048 for the MDCT.  Tolerances: those of
tests/test_gpu_ragged.py (TOL_FFT, TOL_FB with conftest.relerr) against the float64 oracle on x64 = pcm / 32768 averaged over the channels.

A NATIVE case (int16 mono / stereo in the kernel's own loads) asserts three things: plan.last_kernel is the native name; the result is
bit-identical (np.array_equal) to the float twin, *_ragged, on the clips normalised on the host in float32; every clip is within the oracle
tolerance.  A CONVERT-FIRST case asserts equality with the float twin on the converted samples: array_equal where the float twin reports the
same kernel family, else relerr <= 1e-6 (the rule of tests/test_gpu_ragged.py assert_matches_padded)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import arena
from conftest import ROOT, relerr
from oracle import zaf_oracle as orc

pytestmark = pytest.mark.gpu

TOL_FFT = 1e-5
TOL_FB = 1e-4
W, HOP, NMEL, NCOEF = 2048, 1024, 128, 20
# an empty clip, clips shorter than a window, both sides of a 16-frame tile edge, odd lengths, clips of several tiles
L = [0, 1, 1023, 2048, 2049, 16 * 1024 + 3, 17 * 1024 + 2048, 44100, 50001, 33 * 1024 + 5]
# the MDCT's native route (multiples of 4): both sides of a 32-frame tile edge
L4 = [0, 4, 1020, 2048, 32 * 1024, 32 * 1024 + 4, 44100, 50000]


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    return z


# ------------------------------------------------------------------------------------------------------------------ inputs and references
def pcm_clips(lengths, channels, seed=91, dtype=np.int16):
    """Full-range random PCM from a fixed seed, (N_i,) for channels = None, else (N_i, channels).  Clip 0 starts with 7 sample frames of the
    most negative value and then 7 of the most positive one -- as far as it reaches (in L it is empty), and so does the first clip of 14
    sample frames or more."""
    info = np.iinfo(dtype)
    out = []
    for i, n in enumerate(lengths):
        shape = (n,) if channels is None else (n, channels)
        out.append(np.random.default_rng([seed, i, channels or 0]).integers(info.min, info.max, shape, dtype=dtype, endpoint=True))
    for c in (out[0], next((c for c in out if len(c) >= 14), out[0])):
        c[:7], c[7:14] = info.min, info.max
    return out


def host_f32(clips):
    """wavread's x / 2^15 and the channel mean in float32 on the host: exact for int16 of one or two channels."""
    out = []
    for c in clips:
        x = c.astype(np.float32) / np.float32(32768.0)
        out.append(x if x.ndim == 1 else x.mean(axis=1, dtype=np.float32))
    return out


def x64_of(clips):
    return [(c.astype(np.float64) / 32768.0) if c.ndim == 1 else (c.astype(np.float64) / 32768.0).mean(axis=1) for c in clips]


def device_mono(zafx, clips):
    """The clips as k_pcm_to_float normalises them (what the convert-first route feeds the float kernels)."""
    packed, offs, lens = zafx.pack_ragged_pcm(clips)
    mono = zafx.pcm_to_mono(packed[None])[0]
    return [mono[o:o + n] for o, n in zip(offs.tolist(), lens.tolist())]


def line(dtype):
    return 128 // np.dtype(dtype).itemsize


def grid_plan(zafx, kind):
    """The plan a *_pcm_ragged call of this kind runs on (rows of whole lines): its last_kernel names what ran.  Asked for AFTER the call: the
    plan cache is bounded and drops its oldest entry on a miss, so a plan looked up ahead of the call may no longer be the cached one."""
    w, kbd = zafx.hamming(W), zafx.kaiser_bessel_derived(W)
    fb = zafx.melfilterbank(44100, W, NMEL)
    if kind == "mel":
        return zafx.mel_plan(w, HOP, fb, row_align=32)
    if kind == "mfcc":
        return zafx.mel_plan(w, HOP, fb, NCOEF, row_align=32)
    if kind == "mel_mfcc":
        return zafx.mel_plan(w, HOP, fb, NCOEF, row_align=32, also_mel=True)
    if kind == "mdct":
        return zafx.mdct_plan(kbd, row_align=32)
    onesided = {"stft": False, "stft_one": True, "stft_mag": "magnitude", "stft_pow": "power"}[kind]
    p = zafx.stft_plan(w, HOP, onesided=onesided)
    return zafx.stft_plan(w, HOP, onesided=onesided, row_align=line(p.out_dtype))


NATIVE = {"mel": "k_mel2_ragged", "mfcc": "k_mel2_ragged", "mel_mfcc": "k_mel2_ragged", "stft": "k_stft_ft16_ragged", "stft_one": "k_stft_ft16_ragged",
          "stft_mag": "k_mel2_ragged", "stft_pow": "k_mel2_ragged", "mdct": "k_mdct_ft32_ragged"}
STFT_KIND = {"stft": False, "stft_one": True, "stft_mag": "magnitude", "stft_pow": "power"}


def call(zafx, kind, clips, pcm):
    """The public function of `kind`: the PCM one or its float twin.  mel_mfcc: the two lists concatenated per clip."""
    w, fb = zafx.hamming(W), zafx.melfilterbank(44100, W, NMEL)
    sfx = "_pcm_ragged" if pcm else "_ragged"
    if kind == "mel":
        return getattr(zafx, "melspectrogram" + sfx)(clips, w, HOP, fb)
    if kind == "mfcc":
        return getattr(zafx, "mfcc" + sfx)(clips, w, HOP, fb, NCOEF)
    if kind == "mel_mfcc":
        m, c = getattr(zafx, "mel_mfcc" + sfx)(clips, w, HOP, fb, NCOEF)
        return [np.concatenate([a, b]) for a, b in zip(m, c)]
    if kind == "mdct":
        return getattr(zafx, "mdct" + sfx)(clips, zafx.kaiser_bessel_derived(W))
    return getattr(zafx, "stft" + sfx)(clips, w, HOP, onesided=STFT_KIND[kind])


_ORACLE = {}


def oracle(zafx, kind, clips, key):
    """The float64 oracle's per-clip results, computed once per (kind, key) and shared."""
    if (kind, key) not in _ORACLE:
        w, fb = zafx.hamming(W), zafx.melfilterbank(44100, W, NMEL)
        out = []
        for x in x64_of(clips):
            if kind == "mel":
                r = orc.melspectrogram(x, w, HOP, fb)
            elif kind == "mfcc":
                r = orc.mfcc(x, w, HOP, fb, NCOEF)
            elif kind == "mel_mfcc":
                r = np.concatenate([orc.melspectrogram(x, w, HOP, fb), orc.mfcc(x, w, HOP, fb, NCOEF)])
            elif kind == "mdct":
                r = orc.mdct(x, zafx.kaiser_bessel_derived(W))
            else:
                s = orc.stft(x, w, HOP)
                one = s[: W // 2 + 1]
                r = {"stft": s, "stft_one": one, "stft_mag": np.abs(one), "stft_pow": np.abs(one) ** 2}[kind]
            r.setflags(write=False)
            out.append(r)
        _ORACLE[kind, key] = out
    return _ORACLE[kind, key]


def tol_of(kind):
    return TOL_FFT if kind.startswith("stft") or kind == "mdct" else TOL_FB


def family(name):
    return name[: -len("_ragged")] if name.endswith("_ragged") else name


def assert_native(zafx, kind, clips, key):
    """The three assertions of a native case; -> the results."""
    got = call(zafx, kind, clips, True)
    ran = grid_plan(zafx, kind).last_kernel
    twin = call(zafx, kind, host_f32(clips), False)
    refs = oracle(zafx, kind, clips, key)
    assert len(got) == len(clips) == len(twin)
    errs = [relerr(g, r) if g.shape == r.shape else np.inf for g, r in zip(got, refs)]
    print(kind, key, ran, "max relerr", max(errs))
    assert ran == NATIVE[kind], (kind, ran)
    for i, (g, t, r) in enumerate(zip(got, twin, refs)):
        assert g.shape == r.shape and g.dtype == t.dtype, (kind, i, g.shape, r.shape)
        assert np.array_equal(g, t), (kind, i, len(clips[i]))
        assert errs[i] <= tol_of(kind), (kind, i, len(clips[i]), errs[i])
    return got


def assert_equals_float_twin(got, k_pcm, twin, k_float, what):
    assert len(got) == len(twin), what
    same = family(k_pcm) == family(k_float)
    for i, (g, t) in enumerate(zip(got, twin)):
        assert g.shape == t.shape, (what, i, g.shape, t.shape)
        if same:
            assert np.array_equal(g, t), (what, i, k_pcm)
        else:
            assert relerr(g, t) <= 1e-6, (what, i, k_pcm, k_float, relerr(g, t))


# ------------------------------------------------------------------------------------------------------------------ G1: native, lengths L
@pytest.mark.parametrize("channels", [None, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("kind", ["mel", "mfcc", "stft", "stft_one", "stft_mag", "stft_pow"])
def test_native(zafx, kind, channels):
    assert_native(zafx, kind, pcm_clips(L, channels), ("L", channels))


@pytest.mark.parametrize("channels", [None, 2], ids=["mono", "stereo"])
def test_native_mel_mfcc_halves_equal_the_single_output_results(zafx, channels):
    clips = pcm_clips(L, channels)
    both = assert_native(zafx, "mel_mfcc", clips, ("L", channels))
    mel, cep = call(zafx, "mel", clips, True), call(zafx, "mfcc", clips, True)
    for i, b in enumerate(both):
        assert np.array_equal(b[:NMEL], mel[i]) and np.array_equal(b[NMEL:], cep[i]), i


# ------------------------------------------------------------------------------------------------------------------ G2: the MDCT
@pytest.mark.parametrize("channels", [None, 2], ids=["mono", "stereo"])
def test_mdct_native(zafx, channels):
    assert_native(zafx, "mdct", pcm_clips(L4, channels), ("L4", channels))


@pytest.mark.parametrize("channels", [None, 2], ids=["mono", "stereo"])
def test_mdct_any_lengths_convert_first(zafx, channels):
    clips = pcm_clips(L, channels)
    got = call(zafx, "mdct", clips, True)
    k_pcm = grid_plan(zafx, "mdct").last_kernel
    twin = call(zafx, "mdct", device_mono(zafx, clips), False)
    k_float = grid_plan(zafx, "mdct").last_kernel
    assert_equals_float_twin(got, k_pcm, twin, k_float, "mdct L")
    assert k_pcm == k_float == "k_mdct_ft32_ragged"   # (the float launch behind the conversion: the 4-byte-load form)


# ------------------------------------------------------------------------------------------------------------------ G3: convert first
def run_plan(zafx, plan, flat, in_offsets, lengths, channels=0, shift=0):
    """Plan.execute_ragged_pcm (channels >= 1) or Plan.execute_ragged (0) on a hand-made array; shift: the device array is a view that many
    bytes into an allocation.  -> (per-clip results, last_kernel)."""
    in_offsets, lengths = np.asarray(in_offsets, np.int64), np.asarray(lengths, np.int64)
    flat = np.ascontiguousarray(flat)
    offs, frames, pitch = plan.ragged_layout(lengths)
    rows = plan.out_dims(0)[0]
    host = np.concatenate([np.zeros(shift // flat.dtype.itemsize, flat.dtype), flat.reshape(-1)])
    alloc = zafx.DeviceBuffer.from_host(host if host.size else np.zeros(1, flat.dtype), plan.device)
    d_in = zafx.DeviceBuffer((max(flat.size, 1),), flat.dtype, _ptr_from_pool=ctypes.c_void_p(alloc.ptr.value + shift))
    d_out = zafx.DeviceBuffer((max(int(offs[-1]), 1),), plan.out_dtype, plan.device)
    try:
        if channels:
            plan.execute_ragged_pcm(d_in, in_offsets, lengths, d_out, channels)
        else:
            plan.execute_ragged(d_in, in_offsets, lengths, d_out)
        plan.sync()
        res = d_out.download()
    finally:
        d_in.ptr = ctypes.c_void_p()   # (a view: nothing to free)
        alloc.free()
        d_out.free()
    if plan.layout == zafx.LAYOUT_FT:
        out = [res[o:o + rows * p].reshape(rows, p)[:, :t] for o, t, p in zip(offs.tolist(), frames.tolist(), pitch.tolist())]
    else:
        out = [res[o:o + t * rows].reshape(t, rows) for o, t in zip(offs.tolist(), frames.tolist())]
    return out, plan.last_kernel


def laid_out(clips, starts):
    """The clips at sample frames `starts` of one zero-filled array."""
    ch = clips[0].shape[1:]
    total = max(s + len(c) for s, c in zip(starts, clips)) + 1
    flat = np.zeros((total,) + ch, clips[0].dtype)
    for s, c in zip(starts, clips):
        flat[s:s + len(c)] = c
    return flat


@pytest.mark.parametrize("case", ["int32_mono", "int16_5ch", "hop441", "w1024"])
def test_convert_first_through_the_functions(zafx, case):
    w, fb = zafx.hamming(W), zafx.melfilterbank(44100, W, NMEL)
    if case == "int32_mono":
        clips = pcm_clips(L, None, dtype=np.int32)
        plan = lambda: grid_plan(zafx, "mel")
        fn = lambda c, sfx: getattr(zafx, "melspectrogram" + sfx)(c, w, HOP, fb)
    elif case == "int16_5ch":
        clips = pcm_clips(L, 5)
        plan = lambda: grid_plan(zafx, "stft_one")
        fn = lambda c, sfx: getattr(zafx, "stft" + sfx)(c, w, HOP, onesided=True)
    elif case == "hop441":
        clips = pcm_clips(L, None)
        plan = lambda: zafx.mel_plan(w, 441, fb, row_align=32)
        fn = lambda c, sfx: getattr(zafx, "melspectrogram" + sfx)(c, w, 441, fb)
    else:
        clips = pcm_clips(L, 2)
        w1 = zafx.hamming(1024)
        plan = lambda: zafx.stft_plan(w1, 512, row_align=16)
        fn = lambda c, sfx: getattr(zafx, "stft" + sfx)(c, w1, 512)
    got = fn(clips, "_pcm_ragged")
    k_pcm = plan().last_kernel
    twin = fn(device_mono(zafx, clips), "_ragged")
    assert_equals_float_twin(got, k_pcm, twin, plan().last_kernel, case)


def test_convert_first_cqt_plan(zafx):
    ck = zafx.cqtkernel(44100, 24, 55, 3520)
    plan = zafx.cqt_plan(44100, 25, ck)
    clips = [c for c in pcm_clips(L, None) if len(c)]
    clips = sorted(clips, key=len)[:3]   # the three shortest non-empty clips
    packed, in_off, lens = zafx.pack_ragged_pcm(clips)
    got, k_pcm = run_plan(zafx, plan, packed, in_off, lens, channels=1)
    x, f_off, f_lens = zafx.pack_ragged(device_mono(zafx, clips))
    twin, k_float = run_plan(zafx, plan, x, f_off, f_lens)
    assert_equals_float_twin(got, k_pcm, twin, k_float, "cqt")


@pytest.mark.parametrize("case", ["odd_offsets", "two_bytes_off"])
def test_convert_first_through_the_plan(zafx, case):
    clips = pcm_clips(L, None)
    plan = grid_plan(zafx, "mel")
    if case == "odd_offsets":
        starts, at = [], 1
        for c in clips:
            starts.append(at)            # every clip on an odd sample frame
            at += len(c) + 2 + (len(c) % 2)
        assert all(s % 2 == 1 for s in starts)
        got, k_pcm = run_plan(zafx, plan, laid_out(clips, starts), starts, [len(c) for c in clips], channels=1)
    else:
        packed, in_off, lens = zafx.pack_ragged_pcm(clips)
        got, k_pcm = run_plan(zafx, plan, packed, in_off, lens, channels=1, shift=2)
    twin = call(zafx, "mel", device_mono(zafx, clips), False)
    assert_equals_float_twin(got, k_pcm, twin, grid_plan(zafx, "mel").last_kernel, case)
    # (what the route leaves out is the integers in the loads, not the launch: the float kernel's name)
    assert k_pcm == "k_mel2_ragged"


# ------------------------------------------------------------------------------------------------------------------ G4: the persistent loop
@pytest.mark.parametrize("kind", ["mel", "stft_one", "mdct"])
def test_every_workgroup_walks_several_tiles(zafx, kind):
    """80 clips of 8 x 16 x 1024 + 2 i sample frames: more than 2 x 256 tiles of either size, so every workgroup of the grid walks several."""
    lengths = [8 * 16 * 1024 + 2 * i for i in range(80)]
    if kind == "mdct":
        lengths = [n - n % 4 for n in lengths]
    clips = pcm_clips(lengths, None, seed=92)
    got = call(zafx, kind, clips, True)
    assert grid_plan(zafx, kind).last_kernel == NATIVE[kind]
    twin = call(zafx, kind, host_f32(clips), False)
    for i, (g, t) in enumerate(zip(got, twin)):
        assert np.array_equal(g, t), (kind, i)


# ------------------------------------------------------------------------------------------------------------------ G5: permutation
@pytest.mark.parametrize("channels", [None, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("kind", ["mel", "mfcc", "stft", "stft_pow", "mdct"])
def test_permutation_gives_identical_clips(zafx, kind, channels):
    clips = pcm_clips(L4 if kind == "mdct" else L, channels)
    perm = np.random.default_rng(93).permutation(len(clips)).tolist()
    a = call(zafx, kind, clips, True)
    assert grid_plan(zafx, kind).last_kernel == NATIVE[kind]
    b = call(zafx, kind, [clips[i] for i in perm], True)
    for j, i in enumerate(perm):
        assert np.array_equal(a[i], b[j]), (kind, i)


# ------------------------------------------------------------------------------------------------------------------ G6: the arena contract
ARENA_PAIRS = [(128, 128), (128, 8), (2, 128), (8, 128), (16, 128)]
INPUT_GAPS = (1, 3, 5)   # poisoned sample frames behind clips 0, 1 and 2


@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("route", ["mel", "stft", "mdct_edge", "mdct_aligned"])
def test_arena(zafx, route, channels):
    """Three clips in one call at row_align = one line, as tests/test_gpu_arena.py test_ragged and test_mdct_ragged: the array of integers
    starts 128, 2, 8 or 16 bytes into an arena of -32768, the output 128 or 8 bytes into one of marked NaNs.  mel / stft / mdct_edge: 1, 3 and 5
    poisoned sample frames behind the clips (the offsets stay even: lengths and gaps are odd); mdct_aligned: lengths that are multiples of 4,
    back to back.  The integers are read by the kernel itself where route A's conditions hold -- d_pcm on 8 bytes (the MDCT: 16, aligned
    lengths) and d_out on the line grid --; otherwise the conversion feeds the float launch (the same name) or, with d_out off the lines,
    one execute per clip.  (a), (b), (c) of the harness; with the middle clip -32768 throughout, the other clips are bit-identical."""
    from test_gpu_arena import Prep, run
    lengths = [37 * 1024 + 5, 3001, 33 * 1024]
    if route == "mdct_aligned":
        lengths = [n - n % 4 for n in lengths]
    gaps = (0, 0, 0) if route == "mdct_aligned" else INPUT_GAPS
    clips = [c.reshape(len(c), channels) for c in pcm_clips(lengths, channels, seed=94)]
    poison = np.iinfo(np.int16).min
    pieces, in_offsets, at = [], [], 0
    for c, g in zip(clips, gaps):
        in_offsets.append(at)
        pieces += [c, np.full((g, channels), poison, np.int16)]
        at += len(c) + g
    flat, in_offsets, lengths = np.concatenate(pieces), np.array(in_offsets, np.int64), np.array(lengths, np.int64)
    assert not (in_offsets % 2).any() and (route != "mdct_aligned" or not (in_offsets % 4).any())
    kind = "mdct" if route.startswith("mdct") else route
    plan = grid_plan(zafx, kind)
    ref = oracle(zafx, kind, [c[:, 0] if channels == 1 else c for c in clips], ("arena", route, channels))
    offs, frames, pitch = plan.ragged_layout(lengths)
    rows = ref[0].shape[0]
    blocks = [arena.Block(int(offs[i]), (rows, int(pitch[i])), int(frames[i]), ref[i]) for i in range(3)]
    assert int(offs[3]) == sum(rows * int(p) for p in pitch) and [r.shape[1] for r in ref] == frames.tolist()
    poisoned = flat.copy()
    poisoned[in_offsets[1]:in_offsets[1] + lengths[1]] = poison
    launch = lambda d_in, d_out: (plan.execute_ragged_pcm(d_in, in_offsets, lengths, d_out, channels), plan.sync())
    prep = Prep(plan, flat, None, blocks, tol_of(kind), lambda di, do: NATIVE[kind] if do % 128 == 0 else "per-clip*", launch=launch, poisoned=poisoned,
                n_clips=1)
    prep.guard = arena.guard_bytes(int(lengths.max()) * 2 * channels, max(rows * int(p) for p in pitch) * plan.out_dtype.itemsize)
    run(zafx, prep, ARENA_PAIRS)


# ------------------------------------------------------------------------------------------------------------------ G7: groups
def child_groups():
    """Body of test_groups_under_a_small_budget's child process (ZAFX_SCRATCH_BUDGET_MB=1: 262144 float32 samples of staging)."""
    import zafx
    for reps in (1, 3):   # the L clips: one group; three times over, 506586 sample frames: the budget cuts them
        clips = pcm_clips(L * reps, None, dtype=np.int32)
        twin = call(zafx, "mel", device_mono(zafx, clips), False)
        k_float = grid_plan(zafx, "mel").last_kernel
        got = call(zafx, "mel", clips, True)
        plan = grid_plan(zafx, "mel")
        assert_equals_float_twin(got, plan.last_kernel, twin, k_float, ("in order", reps))
        assert plan.last_kernel == k_float == "k_mel2_ragged"
        # shuffled offsets: the clips keep their order in the list and lie in another one in the array
        order = np.random.default_rng(95).permutation(len(clips)).tolist()
        starts, at = [0] * len(clips), 0
        for i in order:
            starts[i] = at
            at += (len(clips[i]) + 63) // 64 * 64
        assert starts != sorted(starts)
        got, k_pcm = run_plan(zafx, plan, laid_out(clips, starts), starts, [len(c) for c in clips], channels=1)
        assert_equals_float_twin(got, k_pcm, twin, k_float, ("shuffled", reps))
    print("groups ok")


def test_groups_under_a_small_budget():
    code = (f"import sys\nfor p in ({os.path.join(ROOT, 'tests')!r}, {ROOT!r}, {os.path.join(ROOT, 'zaf-python_amd')!r}):\n    sys.path.insert(0, p)\n"
            "import test_gpu_pcm_ragged as t\nt.child_groups()\n")
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, ZAFX_SCRATCH_BUDGET_MB="1"), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "groups ok" in res.stdout, (res.stdout + res.stderr)[-3000:]
