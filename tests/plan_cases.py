"""The plans of tests/test_gpu_plan_lifecycle.py and tests/golden/make_plan_golden.py: one per family of tables zafx_plan_create and
zafx_plan_set_constant build, each at the smallest shape that has them, with one execute of two short clips.

A case is a function -> (plan, run): `plan` comes from the package's own factory (constants set), `run(plan)` executes once and returns the
output as a host array.  Inputs are seeded; nothing here reads the oracle."""
import os

import numpy as np
import scipy.sparse

import zafx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FS = 44100


def noise(tag, shape, dtype=np.float32):
    r = np.random.default_rng([41, tag])
    if np.dtype(dtype).kind == "c":
        return (r.standard_normal(shape) + 1j * r.standard_normal(shape)).astype(dtype)
    return r.standard_normal(shape).astype(dtype)


def execute(plan, x, n_in):
    """One zafx_execute of the clips x (clips first) -> the whole output array."""
    d_in = zafx.DeviceBuffer.from_host(np.ascontiguousarray(x, dtype=plan.in_dtype))
    d_out = zafx.DeviceBuffer(plan.out_shape(len(x), n_in), plan.out_dtype).fill_zero()
    try:
        plan.execute(d_in, d_out, len(x), n_in)
        plan.sync()
        return d_out.download()
    finally:
        d_in.free()
        d_out.free()


def forward(make, tag, n):
    """Two clips of n samples through a plan that takes samples."""
    def case():
        plan = make()
        return plan, lambda p: execute(p, noise(tag, (2, n), p.in_dtype), n)
    return case


def inverse(make, tag, rows, frames):
    """Two (rows, frames) arrays through an ISTFT / IMDCT plan."""
    def case():
        plan = make()
        return plan, lambda p: execute(p, noise(tag, (2, rows, frames), p.in_dtype), frames)
    return case


def fb(w, n):
    return zafx.melfilterbank(FS, w, n)


def tiny_cqt():
    ck = scipy.sparse.csr_matrix(np.load(os.path.join(GOLDEN, "tiny.npz"))["ck_dense"])
    return zafx.cqt_plan(4000, 50, ck)


def linear_case():
    plan = zafx.linear_plan(noise(90, (4, 4), np.float64))
    return plan, lambda p: execute(p, noise(91, (2, 4)), 4)


def dct_case(n, kind):
    def case():
        plan = zafx.dct_plan(n, kind)
        return plan, lambda p: execute(p, noise(100 + n, (2, n)), n)
    return case


def center_case():
    plan = zafx.center_plan(zafx.hamming(256))
    return plan, lambda p: execute(p, noise(80, (2, 1000, 2)), 1000)


def ragged_case():
    plan = zafx.stft_plan(zafx.hamming(2048), 512, row_align=16)

    def run(p):
        lengths = np.array([3000, 5000], np.int64)
        offs = np.array([0, 3008], np.int64)
        out_offs, _, _ = p.ragged_layout(lengths)
        d_in = zafx.DeviceBuffer.from_host(noise(70, (8192,)))
        d_out = zafx.DeviceBuffer((int(out_offs[-1]),), p.out_dtype).fill_zero()
        try:
            p.execute_ragged(d_in, offs, lengths, d_out)
            p.sync()
            return d_out.download()
        finally:
            d_in.free()
            d_out.free()
    return plan, run


def run_host_case():
    plan = zafx.stft_plan(zafx.hamming(1024), 256)
    return plan, lambda p: p.run_host(noise(71, (2, 4000)), 4000)


def ham(w):
    return zafx.hamming(w)


def sin(w):
    return zafx.sine(w)


CASES = {
    "stft_64": forward(lambda: zafx.stft_plan(ham(64), 32), 1, 500),
    "stft_2048": forward(lambda: zafx.stft_plan(ham(2048), 1024), 2, 9000),          # claim counters, d_tw_r32
    "stft_4096": forward(lambda: zafx.stft_plan(ham(4096), 2048), 3, 17000),         # d_tw_sub
    "stft_8192": forward(lambda: zafx.stft_plan(ham(8192), 4096), 4, 33000),         # d_tw_sub, d_tw_quad
    "istft_64": inverse(lambda: zafx.istft_plan(ham(64), 32), 5, 64, 9),
    "mdct_64": forward(lambda: zafx.mdct_plan(sin(64)), 6, 500),
    "mdct_2048": forward(lambda: zafx.mdct_plan(sin(2048)), 7, 9000),
    "mdct_4096": forward(lambda: zafx.mdct_plan(sin(4096)), 8, 17000),               # d_tw_sub, d_tw_band
    "mdct_8192": forward(lambda: zafx.mdct_plan(sin(8192)), 9, 33000),               # d_tw_sub, d_tw_quad
    "imdct_4096": inverse(lambda: zafx.mdct_plan(sin(4096), inverse=True), 10, 2048, 9),
    "imdct_8192": inverse(lambda: zafx.mdct_plan(sin(8192), inverse=True), 11, 4096, 9),   # d_tw_sub, d_tw_quad
    "mel_2048": forward(lambda: zafx.mel_plan(ham(2048), 1024, fb(2048, 40)), 12, 9000),   # the fused kernel: PackedBand
    "mel_4096": forward(lambda: zafx.mel_plan(ham(4096), 2048, fb(4096, 40)), 13, 17000),  # the wide route: d_fbw
    "mfcc_4096": forward(lambda: zafx.mel_plan(ham(4096), 2048, fb(4096, 40), 13), 14, 17000),   # d_dctw
    "mfcc_2048": forward(lambda: zafx.mel_plan(ham(2048), 1024, fb(2048, 40), 13), 15, 9000),    # both bands, d_direct
    "mfcc_also_mel": forward(lambda: zafx.mel_plan(ham(2048), 1024, fb(2048, 40), 13, also_mel=True), 16, 9000),   # d_whole, d_dct2
    "center": center_case,
    "cqt_tiny": forward(tiny_cqt, 17, 4000),
    "linear_4x4": linear_case,
    "dct_64": dct_case(64, 2),       # N / 2 a power of two >= 32: k_dct
    "dct_16": dct_case(16, 2),       # N = 4 j: k_dct_bsh
    "dct_12": dct_case(12, 2),
    "dct_15": dct_case(15, 2),       # every other length: k_dct_bs32
    # rows as whole 128-byte lines: what the four-class kernels of W = 8192 take (d_tw_quad in use)
    "stft_8192_lines": forward(lambda: zafx.stft_plan(ham(8192), 4096, row_align=16), 26, 70000),
    "istft_8192_lines": inverse(lambda: zafx.istft_plan(ham(8192), 4096, row_align=16), 27, 8192, 32),
    "imdct_8192_lines": inverse(lambda: zafx.mdct_plan(sin(8192), inverse=True, row_align=32), 28, 4096, 32),
    "stft_bs32_100": forward(lambda: zafx.stft_plan(ham(100), 50), 18, 700),
    "mdct_bs32_100": forward(lambda: zafx.mdct_plan(sin(100)), 19, 700),             # the Bluestein plan's second d_tw_aux
    "stft_2048_f64": forward(lambda: zafx.stft_plan(ham(2048), 1024, f64=True), 20, 9000),
    "mdct_2048_f64": forward(lambda: zafx.mdct_plan(sin(2048), f64=True), 21, 9000),
    "mel_2048_f64": forward(lambda: zafx.mel_plan(ham(2048), 1024, fb(2048, 40), f64=True), 22, 9000),
    "mfcc_2048_f64": forward(lambda: zafx.mel_plan(ham(2048), 1024, fb(2048, 40), 13, f64=True), 23, 9000),
    "istft_2048_f64": inverse(lambda: zafx.istft_plan(ham(2048), 1024, f64=True), 24, 2048, 5),   # the plan's scratch
    "stft_bs_100_f64": forward(lambda: zafx.stft_plan(ham(100), 50, f64=True), 25, 700),
    "execute_ragged": ragged_case,
    "run_host": run_host_case,
}


def record(name):
    """Build the case's plan, execute once, destroy the plan -> (kernel_name, last_kernel, sha256 of the output's bytes)."""
    import hashlib
    zafx.clear_plan_cache()
    plan, run = CASES[name]()
    try:
        out = np.ascontiguousarray(run(plan))
        return plan.kernel_name, plan.last_kernel, hashlib.sha256(out.tobytes()).hexdigest()
    finally:
        zafx.clear_plan_cache()
