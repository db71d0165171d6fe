"""Deterministic test signals that are NOT white noise (verdict r4 item 2), shared by
tests/golden/make_golden.py (which feeds them to the real reference) and the parity tests.

The reference's own examples run on music (zaf.py:62-66); where a float32 pipeline can part from the
float64 reference is on near-silent bands under a loud one, exact zeros, and full-scale / clipped
input (zaf.py:443-446 takes the log of whatever the filterbank leaves).  Every recipe returns float32
(what both sides are fed); `clipped_pcm` also has an int16 form for the PCM entry points
(zaf.py:1202 scales by 2**15).
"""
import numpy as np

FS = 44100
W = 2048
HOP = 1024
N_FRAMES = 3072        # stft / mdct family: 4 STFT frames (two whole, two over the zero padding)
N_CQT = 17640          # cqt family: 10 frames of 32768 samples

NAMES = ("silence", "dc", "sine_bin", "sine_half", "two_tones", "impulse", "chirp", "noise_m90", "clipped_pcm")


def clipped_pcm16(n):
    """A sine 3.5 dB over full scale, rounded and clipped the way a 16-bit recorder does."""
    t = np.arange(n, dtype=np.float64)
    v = np.rint(1.5 * 32767.0 * np.sin(2 * np.pi * 97.3 * t / W))
    return np.clip(v, -32768, 32767).astype(np.int16)


def signal(name, n):
    t = np.arange(n, dtype=np.float64)
    if name == "silence":
        x = np.zeros(n)
    elif name == "dc":
        x = np.full(n, 0.5)
    elif name == "sine_bin":          # full scale, exactly on bin 100 of a 2048-point frame
        x = np.sin(2 * np.pi * 100.0 * t / W)
    elif name == "sine_half":         # halfway between bins 100 and 101
        x = np.sin(2 * np.pi * 100.5 * t / W)
    elif name == "two_tones":         # 100 dB apart
        x = np.sin(2 * np.pi * 100.25 * t / W) + 1e-5 * np.sin(2 * np.pi * 700.5 * t / W + 0.3)
    elif name == "impulse":           # unit impulses on, and one sample before, hop boundaries
        x = np.zeros(n)
        for p in (HOP, 2 * HOP, 3 * HOP - 1, n - 1):
            if 0 <= p < n:
                x[p] = 1.0
    elif name == "chirp":             # linear sweep 0 .. fs/2 over the clip
        x = 0.8 * np.sin(np.pi * (t * t) / (2.0 * n))
    elif name == "noise_m90":         # white noise at -90 dBFS
        x = np.random.default_rng([90, n]).standard_normal(n) * 10.0 ** (-90.0 / 20.0)
    elif name == "clipped_pcm":
        x = clipped_pcm16(n).astype(np.float64) / 32768.0
    else:
        raise KeyError(name)
    return x.astype(np.float32)


# Stereo clips for the center / sides extraction (zaf.py:155-198), built from the mono recipes above -- which stay as they are: signals.npz
# pins their sums.  Each name is a case of the mask arithmetic (zafx_center.hpp): 0 / 0 in every bin, one channel's peak over the other's
# leakage, a mask of exactly 0.5, a == b in every bin, a loud passage in front of a quiet one, a reference that is identically zero.
STEREO_NAMES = ("silence", "dc", "pan_tones", "gain", "anti", "tones_chirp", "impulse", "noise_m90", "clipped", "loud_quiet", "left_only")


def stereo_signal(name, n):
    """(n, 2) float32: left, right."""
    if name == "silence":
        l, r = signal("silence", n), signal("silence", n)
    elif name == "dc":
        l, r = signal("dc", n), np.full(n, 0.25, np.float32)
    elif name == "pan_tones":         # hard-panned tones: each channel's peak sits over the other's leakage
        l, r = signal("sine_bin", n), signal("sine_half", n)
    elif name == "gain":              # m0 = 0.5 exactly, m1 = 1: the center is 0.5 s in both channels
        l = signal("sine_half", n)
        r = np.float32(0.5) * l
    elif name == "anti":              # a == b in every bin: both masks 1
        l = signal("chirp", n)
        r = -l
    elif name == "tones_chirp":
        l, r = signal("two_tones", n), signal("chirp", n)
    elif name == "impulse":
        l = signal("impulse", n)
        r = np.roll(l, 3)
    elif name == "noise_m90":         # two independent noises at -90 dBFS
        l = signal("noise_m90", n)
        r = (np.random.default_rng([91, n]).standard_normal(n) * 10.0 ** (-90.0 / 20.0)).astype(np.float32)
    elif name == "clipped":
        l = signal("clipped_pcm", n)
        r = (np.rint(0.7 * l.astype(np.float64) * 32768.0) / 32768.0).astype(np.float32)
    elif name == "loud_quiet":        # unit noise, then noise at -90 dB / the same reversed in time
        g = np.random.default_rng([92, n]).standard_normal(n)
        g[n // 2:] *= 10.0 ** (-90.0 / 20.0)
        l = g.astype(np.float32)
        r = l[::-1]
    elif name == "left_only":         # the center is exactly 0 in the reference arithmetic
        l, r = signal("chirp", n), signal("silence", n)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(np.stack([l, r], axis=1), dtype=np.float32)
