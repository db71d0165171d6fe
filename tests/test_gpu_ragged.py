"""Ragged batches on the GPU (-m gpu): clips of different lengths in one call (zafx_execute_ragged), against the CPU oracle, against the
padded equal-length batch, and on the paths that fall back to one execute per clip."""
import numpy as np
import pytest

from conftest import relerr
from oracle import zaf_oracle as orc

pytestmark = pytest.mark.gpu

TOL_FFT = 1e-5
TOL_FB = 1e-4
KINDS = [False, True, "magnitude", "power"]


@pytest.fixture(scope="module")
def zafx():
    import zafx as z
    assert z.device_count() >= 1
    return z


def lengths_for(w, hop, seed, n_random=4):
    rng = np.random.default_rng([seed, w, hop])
    return [0, 1, w // 2 - 1, w, w + 1, 16 * hop + 3, 44100, 123457] + rng.integers(0, 50000, n_random).tolist()


def noise_clips(lengths, seed):
    return [np.random.default_rng([seed, i]).standard_normal(n).astype(np.float32) for i, n in enumerate(lengths)]


def line(dtype):
    return 128 // np.dtype(dtype).itemsize


def stft_grid_plan(zafx, w, hop, kind):
    p = zafx.stft_plan(w, hop, onesided=kind)
    return zafx.stft_plan(w, hop, onesided=kind, row_align=line(p.out_dtype))


def of_kind(spec, kind, w):
    if kind is False:
        return spec
    one = spec[: w // 2 + 1]
    return one if kind is True else np.abs(one) if kind == "magnitude" else np.abs(one) ** 2


def family(name):
    return name[: -len("_ragged")] if name.endswith("_ragged") else name


def padded_reference(plan, clips):
    """The padded equal-length batch on the same plan: (B, F, pitch) results sliced to each clip's frames, and the kernel that ran."""
    nmax = max(len(c) for c in clips)
    x = np.zeros((len(clips), nmax), plan.in_dtype)
    for i, c in enumerate(clips):
        x[i, : len(c)] = c
    out = plan.run_host(x, nmax)
    return out, plan.last_kernel


def assert_matches_padded(got, pad, frames, same_family):
    for i, g in enumerate(got):
        ref = pad[i][..., : frames[i]]
        if same_family:
            assert np.array_equal(g, ref), i
        else:
            assert relerr(g, ref) <= 1e-6, i


# ------------------------------------------------------------------ 1 + 3: against the oracle, native path taken
@pytest.mark.parametrize("w", [256, 512, 1024, 2048])
@pytest.mark.parametrize("hop_of", ["half", "quarter", 100, 37])
def test_stft_ragged_against_oracle(zafx, w, hop_of):
    hop = {"half": w // 2, "quarter": w // 4}.get(hop_of, hop_of)
    lengths = lengths_for(w, hop, 1)
    clips = noise_clips(lengths, 2)
    window = zafx.hamming(w)
    refs = [orc.stft(c.astype(np.float64), window, hop) for c in clips]
    for kind in KINDS:
        got = zafx.stft_ragged(clips, window, hop, onesided=kind)
        plan = stft_grid_plan(zafx, window, hop, kind)
        want = "k_mel2_ragged" if w == 2048 and kind in ("magnitude", "power") else "k_stft_ft16_ragged"
        assert plan.last_kernel == want, (kind, plan.last_kernel)
        assert len(got) == len(clips)
        for i, (g, r) in enumerate(zip(got, refs)):
            ref = of_kind(r, kind, w)
            assert g.shape == ref.shape, (kind, i, g.shape, ref.shape)
            assert g.dtype == (np.complex64 if kind in (False, True) else np.float32)
            assert relerr(g, ref) <= TOL_FFT, (kind, i, lengths[i], relerr(g, ref))


@pytest.mark.parametrize("hop", [1024, 512, 100, 37])
def test_mel_mfcc_ragged_against_oracle(zafx, hop):
    w = 2048
    lengths = lengths_for(w, hop, 3)
    clips = noise_clips(lengths, 4)
    window = zafx.hamming(w)
    fb = zafx.melfilterbank(44100, w, 128)
    mel = zafx.melspectrogram_ragged(clips, window, hop, fb)
    assert zafx.mel_plan(window, hop, fb, row_align=32).last_kernel == "k_mel2_ragged"
    cep = zafx.mfcc_ragged(clips, window, hop, fb, 20)
    assert zafx.mel_plan(window, hop, fb, 20, row_align=32).last_kernel == "k_mel2_ragged"
    both_mel, both_cep = zafx.mel_mfcc_ragged(clips, window, hop, fb, 20)
    assert zafx.mel_plan(window, hop, fb, 20, row_align=32, also_mel=True).last_kernel == "k_mel2_ragged"
    for i, c in enumerate(clips):
        x = c.astype(np.float64)
        rm, rc = orc.melspectrogram(x, window, hop, fb), orc.mfcc(x, window, hop, fb, 20)
        assert mel[i].shape == rm.shape and cep[i].shape == rc.shape
        assert relerr(mel[i], rm) <= TOL_FB, (i, lengths[i])
        assert relerr(cep[i], rc) <= TOL_FB, (i, lengths[i])
        assert np.array_equal(both_mel[i], mel[i]) and np.array_equal(both_cep[i], cep[i]), i


# ------------------------------------------------------------------ 2: against the padded batch
@pytest.mark.parametrize("w", [256, 512, 1024, 2048])
@pytest.mark.parametrize("parity", ["even", "any"])
def test_stft_ragged_equals_padded_batch(zafx, w, parity):
    rng = np.random.default_rng([5, w])
    lengths = rng.integers(0, 40000, 64)
    if parity == "even":
        lengths -= lengths % 2   # (with an even hop: the aligned loads)
    clips = noise_clips(lengths.tolist(), 6)
    window = zafx.hamming(w)
    for kind in KINDS:
        got = zafx.stft_ragged(clips, window, w // 2, onesided=kind)
        plan = stft_grid_plan(zafx, window, w // 2, kind)
        ragged_kernel = plan.last_kernel
        pad, pad_kernel = padded_reference(plan, clips)
        frames = [g.shape[-1] for g in got]
        assert_matches_padded(got, pad, frames, family(ragged_kernel) == family(pad_kernel))


@pytest.mark.parametrize("parity", ["even", "any"])
def test_mel_ragged_equals_padded_batch(zafx, parity):
    rng = np.random.default_rng(7)
    lengths = rng.integers(0, 60000, 64)
    if parity == "even":
        lengths -= lengths % 2
    clips = noise_clips(lengths.tolist(), 8)
    window = zafx.hamming(2048)
    fb = zafx.melfilterbank(44100, 2048, 128)
    for ncoef, also in ((None, False), (20, False), (20, True)):
        plan = zafx.mel_plan(window, 1024, fb, ncoef, row_align=32, also_mel=also)
        if also:
            m, c = zafx.mel_mfcc_ragged(clips, window, 1024, fb, 20)
            got = [np.concatenate([a, b]) for a, b in zip(m, c)]
        elif ncoef is None:
            got = zafx.melspectrogram_ragged(clips, window, 1024, fb)
        else:
            got = zafx.mfcc_ragged(clips, window, 1024, fb, ncoef)
        ragged_kernel = plan.last_kernel
        assert ragged_kernel == "k_mel2_ragged"
        pad, pad_kernel = padded_reference(plan, clips)
        assert_matches_padded(got, pad, [g.shape[-1] for g in got], family(ragged_kernel) == family(pad_kernel))


# ------------------------------------------------------------------ 4: gaps untouched
@pytest.mark.parametrize("w,kind", [(256, False), (1024, True), (2048, True), (2048, "power"), (512, "magnitude")])
def test_ragged_writes_nothing_but_the_clips(zafx, w, kind):
    lengths = [0, 1, 3 * w + 7, 5000, 77, 20000]
    clips = noise_clips(lengths, 9)
    plan = stft_grid_plan(zafx, zafx.hamming(w), w // 4, kind)
    x, in_off, lens = zafx.pack_ragged(clips)
    offs, frames, pitch = plan.ragged_layout(lens)
    rows = plan.out_dims(0)[0]
    total = int(offs[-1]) + 64
    sentinel = np.full(total, np.nan, plan.out_dtype)
    d_in = zafx.DeviceBuffer.from_host(x, plan.device)
    d_out = zafx.DeviceBuffer.from_host(sentinel, plan.device)
    plan.execute_ragged(d_in, in_off, lens, d_out)
    plan.sync()
    assert plan.last_kernel in ("k_stft_ft16_ragged", "k_mel2_ragged")
    res = d_out.download()
    real = np.zeros(total, bool)
    for o, t, p in zip(offs.tolist(), frames.tolist(), pitch.tolist()):
        block = real[o: o + rows * p].reshape(rows, p)
        block[:, :t] = True
    assert np.all(np.isfinite(res[real]))
    assert np.all(np.isnan(res[~real]))


# ------------------------------------------------------------------ 5: order does not matter
def test_ragged_permutation_gives_identical_clips(zafx):
    lengths = np.random.default_rng(10).integers(0, 30000, 48).tolist()
    clips = noise_clips(lengths, 11)
    perm = np.random.default_rng(12).permutation(len(clips))
    window = zafx.hamming(2048)
    fb = zafx.melfilterbank(44100, 2048, 128)
    for fn in (lambda c: zafx.stft_ragged(c, window, 1024), lambda c: zafx.stft_ragged(c, window, 512, onesided="power"),
               lambda c: zafx.mfcc_ragged(c, window, 1024, fb, 20), lambda c: zafx.stft_ragged(c, zafx.hamming(512), 100, onesided=True)):
        a = fn(clips)
        b = fn([clips[i] for i in perm])
        for j, i in enumerate(perm.tolist()):
            assert np.array_equal(a[i], b[j]), i


# ------------------------------------------------------------------ 6: the kinds that run one execute per clip
def _fallback_cases(zafx):
    kbd = zafx.kaiser_bessel_derived(2048)
    ck = zafx.cqtkernel(44100, 24, 55, 3520)
    return [
        ("mdct", zafx.mdct_plan(kbd), lambda c: zafx.mdct_batch(c[None], kbd, row_align=0)[0], np.float32),
        ("cqt", zafx.cqt_plan(44100, 25, ck), lambda c: zafx.cqtspectrogram_batch(c[None], 44100, 25, ck)[0], np.float32),
        ("chroma", zafx.cqt_plan(44100, 25, ck, 24), lambda c: zafx.cqtchromagram_batch(c[None], 44100, 25, 24, ck)[0], np.float32),
        ("stft TF", zafx.stft_plan(zafx.hamming(1024), 256, layout="TF"),
         lambda c: zafx.stft_batch(c[None], zafx.hamming(1024), 256, layout="TF")[0], np.float32),
        ("stft f64", zafx.stft_plan(zafx.hamming(1024), 256, f64=True),
         lambda c: zafx.stft_batch(c[None], zafx.hamming(1024), 256, f64=True, row_align=0)[0], np.float64),
    ]


@pytest.mark.parametrize("case", range(5))
def test_fallback_kinds_equal_per_clip_batches(zafx, case):
    name, plan, per_clip, dtype = _fallback_cases(zafx)[case]
    lengths = [0, 1, 3000, 44100, 100003, 25000]
    if name == "mdct":
        lengths = lengths[1:]
    if name in ("cqt", "chroma"):
        lengths = [n for n in lengths if n >= 1764] + [1764, 50000]   # (CQT: whole steps of 1764 samples give frames)
    clips = [c.astype(dtype) for c in noise_clips(lengths, 13)]
    x, in_off, lens = zafx.pack_ragged(clips, dtype)
    offs, frames, pitch = plan.ragged_layout(lens)
    rows = plan.out_dims(0)[0]
    d_in = zafx.DeviceBuffer.from_host(x, plan.device)
    d_out = zafx.DeviceBuffer((max(int(offs[-1]), 1),), plan.out_dtype, plan.device)
    plan.execute_ragged(d_in, in_off, lens, d_out)
    plan.sync()
    assert plan.last_kernel.startswith("per-clip "), plan.last_kernel
    res = d_out.download()
    for i, c in enumerate(clips):
        o, t, p = int(offs[i]), int(frames[i]), int(pitch[i])
        got = res[o: o + rows * p].reshape(rows, p)[:, :t] if plan.layout == zafx.LAYOUT_FT else res[o: o + t * rows].reshape(t, rows)
        assert np.array_equal(got, per_clip(c)), (name, i)


# ------------------------------------------------------------------ 7: the staging copy of the table
def test_back_to_back_calls_each_see_their_own_table(zafx):
    window = zafx.hamming(2048)
    plan = stft_grid_plan(zafx, window, 1024, True)
    rng = np.random.default_rng(14)
    batches = []
    for b in range(2):
        lengths = rng.integers(0, 20000, 1024).tolist()
        clips = noise_clips(lengths, 15 + b)
        x, in_off, lens = zafx.pack_ragged(clips)
        offs, frames, pitch = plan.ragged_layout(lens)
        batches.append((zafx.DeviceBuffer.from_host(x), in_off, lens, int(offs[-1])))
    outs = [zafx.DeviceBuffer((n,), plan.out_dtype) for *_, n in batches]
    expect = []
    for (d_in, in_off, lens, _), d_out in zip(batches, outs):   # one call at a time
        plan.execute_ragged(d_in, in_off, lens, d_out)
        plan.sync()
        expect.append(d_out.download())
        d_out.upload(np.zeros(d_out.shape, plan.out_dtype))
    for (d_in, in_off, lens, _), d_out in zip(batches, outs):   # both enqueued, no sync between them
        plan.execute_ragged(d_in, in_off, lens, d_out)
    plan.sync()
    for e, d_out in zip(expect, outs):
        assert np.array_equal(d_out.download(), e)


# ------------------------------------------------------------------ 8: full size
def test_full_size_batch(zafx):
    rng = np.random.default_rng(16)
    lengths = rng.integers(5 * 44100, 15 * 44100 + 1, 1024).tolist()
    clips = noise_clips(lengths, 17)
    window = zafx.hamming(2048)
    got = zafx.stft_ragged(clips, window, 1024, onesided=True)
    plan = stft_grid_plan(zafx, window, 1024, True)
    assert plan.last_kernel == "k_stft_ft16_ragged"
    for i in (0, 511, 1023):
        ref = orc.stft(clips[i].astype(np.float64), window, 1024)[:1025]
        assert got[i].shape == ref.shape and relerr(got[i], ref) <= TOL_FFT, i
    nmax = max(lengths)
    for c0 in range(0, 1024, 128):   # the padded batch in chunks (its result is 1.5 x the ragged one)
        chunk = clips[c0: c0 + 128]
        x = np.zeros((len(chunk), nmax), np.float32)
        for j, c in enumerate(chunk):
            x[j, : len(c)] = c
        pad = plan.run_host(x, nmax)
        same = family(plan.last_kernel) == "k_stft_ft16"
        for j in range(len(chunk)):
            ref = pad[j][:, : got[c0 + j].shape[1]]
            assert np.array_equal(got[c0 + j], ref) if same else relerr(got[c0 + j], ref) <= 1e-6, c0 + j
