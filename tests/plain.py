"""Every operation of the oracle (oracle/zaf_oracle.py) once more, at a chosen precision.  TEST INFRASTRUCTURE ONLY.

Each function takes the input, the constants AS DATA (window, dense filterbank, DCT rows, CSR kernel, matrix) and a `dtype` out of
np.float32, np.float64, np.longdouble; every array and every arithmetic step -- framing, window product, FFT, modulus, products, log,
overlap-add, the division by the COLA gain -- is in that precision.  Three uses (tests/accuracy.py):

  float32     the yardstick of the float32 kernels: what a plain, correct single-precision implementation achieves on this very input;
  float64     the yardstick of the float64 kernels (and, held to the pinned oracle at 1e-12, the proof that this file restates it);
  longdouble  the reference of the float64 kernels: the float64 oracle is itself at 2e-16 ... 3e-16 and cannot judge them below 1e-12.

Three traps:

  * np.fft.fft on complex64 is NOT a single-precision computation (NumPy 2.2.6: its rms error is 2.5e-8 at every length, one final
    rounding).  scipy.fft computes in the input's precision -- complex64 9.9e-8 / 1.20e-7 / 1.38e-7 at N = 256 / 2048 / 16384, float64
    2.0e-16 ... 3.0e-16 against its own complex256 result -- and is the only transform used here
    (tests/test_accuracy_host.py::test_the_yardstick_is_single_precision);
  * the roots of unity of the MDCT / IMDCT twiddles: the angle is reduced in integers and evaluated with a long-double pi (np.pi is a
    double), then rounded once to float64 and from there to float32 -- as the kernels' host-built tables round roots computed in double;
  * long double must be the x87 format (64-bit mantissa): asserted at import, on purpose not a skip.

Batches: clips are the leading axis; a forward transform gives (B, rows, frames), an inverse one (B, samples)."""
import numpy as np
import scipy.fft

assert np.finfo(np.longdouble).nmant >= 63, "plain.py needs an 80-bit long double (x86-64): np.longdouble is no wider than a double here"

DTYPES = (np.float32, np.float64, np.longdouble)
PI_LONG = 4 * np.arctan(np.longdouble(1))


def real_of(dtype):
    dtype = np.dtype(dtype)
    assert dtype in [np.dtype(d) for d in DTYPES], dtype
    return dtype


def complex_of(dtype):
    return np.result_type(real_of(dtype), np.complex64)


def roots(num, den, dtype):
    """exp(-2 pi i num / den) for integer arrays num and an integer den, in `dtype`."""
    dtype = real_of(dtype)
    k = np.asarray(num, dtype=np.int64) % int(den)
    angle = -2 * PI_LONG * k.astype(np.longdouble) / np.longdouble(den)
    z = np.cos(angle) + 1j * np.sin(angle)
    if dtype != np.dtype(np.longdouble):
        z = z.astype(np.complex128)   # a table built in double ...
    return z.astype(complex_of(dtype))   # ... and rounded to the kernel's type


def fft(a, axis=-1, n=None):
    out = scipy.fft.fft(a, n=n, axis=axis)
    assert out.dtype == np.result_type(a.dtype, np.complex64), (a.dtype, out.dtype)
    return out


def ifft(a, axis=-1):
    out = scipy.fft.ifft(a, axis=axis)
    assert out.dtype == a.dtype, (a.dtype, out.dtype)
    return out


def _clips(x, dtype):
    x = np.asarray(x)
    assert x.ndim == 2, x.shape
    return x.astype(dtype)


def _frames(xp, count, hop, length):
    idx = (np.arange(count) * hop)[:, None] + np.arange(length)[None, :]
    return xp[:, idx]   # (B, T, W)


def _overlap_add(frames, hop, total):
    """frames (B, W, T) -> (B, total): frame after frame, as the reference's loop adds them."""
    b, wl, nt = frames.shape
    y = np.zeros((b, total), frames.dtype)
    for j in range(nt):
        y[:, j * hop:j * hop + wl] = y[:, j * hop:j * hop + wl] + frames[:, :, j]
    return y


# ------------------------------------------------------------------------------------------------ stft / istft  (zaf.py:45-243)
def stft_num_frames(n, wl, hop):
    return -(-(n + 2 * (wl // 2) - wl) // hop) + 1


def stft(x, window, hop, dtype, spectrum=False):
    """(B, N) -> (B, W, T) complex; spectrum True: rows 0 .. W/2; "magnitude" / "power": their modulus / its square, real."""
    dtype = real_of(dtype)
    x, w = _clips(x, dtype), np.asarray(window).astype(dtype)
    b, n = x.shape
    wl = len(w)
    nt = stft_num_frames(n, wl, hop)
    xp = np.zeros((b, nt * hop + (wl - hop)), dtype)
    xp[:, wl // 2:wl // 2 + n] = x
    spec = fft(_frames(xp, nt, hop, wl) * w, axis=-1).transpose(0, 2, 1)
    assert spec.dtype == complex_of(dtype)
    if spectrum is False:
        return spec
    half = spec[:, :wl // 2 + 1]
    return half if spectrum is True else np.abs(half) if spectrum == "magnitude" else np.abs(half) ** 2


def istft(spec, window, hop, dtype, onesided=False):
    """(B, W, T) complex (onesided: (B, W/2 + 1, T)) -> (B, T H - (W - H))."""
    dtype = real_of(dtype)
    s, w = np.asarray(spec).astype(complex_of(dtype)), np.asarray(window).astype(dtype)
    if onesided:
        s = np.concatenate([s, np.conj(s[:, -2:0:-1])], axis=1)
    b, wl, nt = s.shape
    assert wl == len(w)
    total = nt * hop + (wl - hop)
    y = _overlap_add(np.real(ifft(s, axis=1)), hop, total)[:, wl - hop:total - (wl - hop)]
    gain = dtype.type(0)
    for v in w[0:wl:hop]:
        gain = gain + v
    out = y / gain
    assert out.dtype == dtype
    return out


# ------------------------------------------------------------------------------------------------ mask filter  (zaf.py:185-195)
def _maskfilter(x, window, mirrored, dtype):
    """x (N,), mirrored (W, T): the two-sided mask -> (N,): istft(mirrored * stft(x)) at hop W / 2, unpacked, one frame per transform."""
    dtype = real_of(dtype)
    x = np.asarray(x)
    assert x.ndim == 1 and mirrored.shape[0] == len(window), (x.shape, mirrored.shape)
    hop = len(window) // 2
    spec = stft(x[None], window, hop, dtype)
    assert spec.shape[1:] == mirrored.shape, (spec.shape, mirrored.shape)
    prod = spec * mirrored[None]   # (mirrored: already `dtype` or its complex type)
    assert prod.dtype == complex_of(dtype)
    out = istft(prod, window, hop, dtype)[0, :len(x)]
    assert out.dtype == dtype
    return out


def maskfilter(x, window, mask, dtype):
    """x (N,), mask (W/2 + 1, T) real -> (N,): y = istft(concat(m, m[-2:0:-1]) * stft(x, w, W/2), w, W/2)[0:N]."""
    m = np.asarray(mask).astype(real_of(dtype))
    return _maskfilter(x, window, np.concatenate((m, m[-2:0:-1])), dtype)


def maskfilter_complex(x, window, mask, dtype):
    """The same under a complex mask (W/2 + 1, T) and its Hermitian mirror, concat(M, conj(M[-2:0:-1])); istft keeps the real part."""
    m = np.asarray(mask).astype(complex_of(dtype))
    return _maskfilter(x, window, np.concatenate((m, np.conj(m[-2:0:-1]))), dtype)


def maskfilter_stems(x, window, masks, dtype, rest=False):
    """x (N,), masks (S, W/2 + 1, T) real -> (S, N), with rest (S + 1, N): the last row is ((x - y_0) - y_1) - ... in `dtype`, left to right."""
    dtype = real_of(dtype)
    rows = [maskfilter(x, window, m, dtype) for m in masks]
    if rest:
        r = np.asarray(x).astype(dtype)
        for y in rows:
            r = r - y
        rows.append(r)
    out = np.stack(rows)
    assert out.dtype == dtype
    return out


def maskfilter_stereo(x, window, masks, dtype, rest=False):
    """x (N, 2), masks (W/2 + 1, T) for both channels or (2, W/2 + 1, T) -> (2, N): y_L, y_R, each channel alone through maskfilter -- no
    packing of the two into one transform; with rest (4, N): rest_L, rest_R = x - y in `dtype` behind them."""
    x, masks = np.asarray(x), np.asarray(masks)
    assert x.ndim == 2 and x.shape[1] == 2 and masks.ndim in (2, 3), (x.shape, masks.shape)
    per = [maskfilter_stems(np.ascontiguousarray(x[:, c]), window, (masks if masks.ndim == 2 else masks[c])[None], dtype, rest=rest) for c in (0, 1)]
    return np.stack([per[c][j] for j in range(1 + int(rest)) for c in (0, 1)])


# ------------------------------------------------------------------------------------------------ mdct / imdct  (zaf.py:984-1184)
def mdct_num_frames(n, wl):
    return -(-n // (wl // 2)) + 1


def mdct(x, window, dtype):
    """(B, N) -> (B, W/2, T)."""
    dtype = real_of(dtype)
    x, w = _clips(x, dtype), np.asarray(window).astype(dtype)
    b, n = x.shape
    wl = len(w)
    hop = wl // 2
    nt = mdct_num_frames(n, wl)
    xp = np.zeros((b, (nt + 2) * hop), dtype)
    xp[:, hop:hop + n] = x
    pre = roots(np.arange(wl), 2 * wl, dtype)                                   # exp(-i pi k / W)
    post = roots((hop + 1) * (2 * np.arange(hop) + 1), 4 * wl, dtype)           # exp(-i pi (W/2 + 1)(j + 1/2) / W)
    seg = fft(_frames(xp, nt, hop, wl) * w * pre, axis=-1)
    out = np.real(seg[..., :hop] * post).transpose(0, 2, 1)
    assert out.dtype == dtype
    return out


def imdct(coefs, window, dtype):
    """(B, W/2, T) -> (B, (W/2)(T - 1) - 1)."""
    dtype = real_of(dtype)
    c, w = np.asarray(coefs).astype(dtype), np.asarray(window).astype(dtype)
    b, nf, nt = c.shape
    assert 2 * nf == len(w)
    pre = roots((nf + 1) * np.arange(nf), 4 * nf, dtype)                        # exp(-i pi (nf + 1) k / (2 nf))
    post = roots(4 * np.arange(2 * nf) + 2 + 2 * nf, 16 * nf, dtype) / dtype.type(nf)   # exp(-i pi (j + 1/2 + nf/2) / (2 nf)) / nf
    spec = fft(c * pre[None, :, None], n=2 * nf, axis=1)
    frames = 2 * (np.real(spec * post[None, :, None]) * w[None, :, None])
    out = _overlap_add(frames, nf, nf * (nt + 1))[:, nf:-nf - 1]
    assert out.dtype == dtype
    return out


# ------------------------------------------------------------------------------------------------ mel / mfcc  (zaf.py:324-454)
def melspectrogram(x, window, hop, fb, dtype):
    """fb: the dense (n_mel, W/2) filterbank.  (B, N) -> (B, n_mel, T)."""
    dtype = real_of(dtype)
    wl = len(window)
    mag = np.abs(stft(x, window, hop, dtype)[:, 1:wl // 2 + 1])
    out = np.matmul(np.asarray(fb).astype(dtype), mag)
    assert out.dtype == dtype
    return out


def logmel(x, window, hop, fb, dtype):
    """The values the MFCC's DCT rows are applied to: log(fb |X|^2 + eps), eps the double's (zaf.py:444-446).  (B, n_mel, T)."""
    dtype = real_of(dtype)
    wl = len(window)
    mag = np.abs(stft(x, window, hop, dtype)[:, 1:wl // 2 + 1])
    return np.log(np.matmul(np.asarray(fb).astype(dtype), mag ** 2) + dtype.type(np.finfo(float).eps))


def mfcc(x, window, hop, fb, dct_rows, dtype, also_mel=False):
    """dct_rows: the (n_coef, n_mel) rows applied to the log-mel values (the reference fixes them to DCT-II rows 1 .. n_coef).
    (B, N) -> (B, n_coef, T); also_mel: the melspectrogram's rows in front of them."""
    dtype = real_of(dtype)
    cep = np.matmul(np.asarray(dct_rows).astype(dtype), logmel(x, window, hop, fb, dtype))
    assert cep.dtype == dtype
    return np.concatenate([melspectrogram(x, window, hop, fb, dtype), cep], axis=1) if also_mel else cep


# ------------------------------------------------------------------------------------------------ cqt  (zaf.py:562-700)
def cqtspectrogram(x, step, cqt_kernel, dtype):
    """cqt_kernel: scipy.sparse CSR (n_bins, fft_length), complex.  (B, N) -> (B, n_bins, floor(N / step))."""
    dtype = real_of(dtype)
    x = _clips(x, dtype)
    b, n = x.shape
    ck = cqt_kernel.tocsr()
    ck.sort_indices()
    nbins, fft_len = ck.shape
    data = ck.data.astype(complex_of(dtype))
    nt = n // step
    left = -(-(fft_len - step) // 2)
    xp = np.zeros((b, left + n + (fft_len - step) // 2), dtype)
    xp[:, left:left + n] = x
    spec = fft(_frames(xp, nt, step, fft_len), axis=-1)                          # (B, T, fft_len)
    out = np.zeros((b, nbins, nt), dtype)
    for r in range(nbins):
        lo, hi = ck.indptr[r], ck.indptr[r + 1]
        if hi > lo:
            out[:, r] = np.abs((spec[:, :, ck.indices[lo:hi]] * data[lo:hi]).sum(axis=-1))
    return out


def cqtchromagram(x, step, octave_resolution, cqt_kernel, dtype):
    spec = cqtspectrogram(x, step, cqt_kernel, dtype)
    out = np.stack([spec[:, i::octave_resolution].sum(axis=1) for i in range(octave_resolution)], axis=1)
    assert out.dtype == real_of(dtype)
    return out


# ------------------------------------------------------------------------------------------------ dct / dst  (zaf.py:703-981)
def _ext_fft(parts, length, dtype):
    """Pieces (start, stop, step, values (B, n)) scattered into zero rows of `length`, and their FFT."""
    b = parts[0][3].shape[0]
    ext = np.zeros((b, length), dtype)
    for start, stop, step, values in parts:
        ext[:, start:stop:step] = values
    return fft(ext, axis=-1)


def dct(x, dct_type, dtype):
    """(B, N) -> (B, N): the orthonormal DCT-I .. IV of every row by the FFT of a symmetric extension."""
    dtype = real_of(dtype)
    x = _clips(x, dtype).copy()
    n = x.shape[1]
    two = dtype.type(2)
    r2 = np.sqrt(two)
    rev = x[:, ::-1]
    if dct_type == 1:
        x[:, [0, -1]] = x[:, [0, -1]] * r2
        out = np.real(fft(np.concatenate((x, x[:, -2:0:-1]), axis=1), axis=-1)[:, :n]) / 2
        out[:, [0, -1]] = out[:, [0, -1]] / r2
        return out * np.sqrt(two / dtype.type(n - 1))
    if dct_type == 2:
        out = np.real(_ext_fft([(1, 2 * n, 2, x), (2 * n + 1, 4 * n, 2, rev)], 4 * n, dtype)[:, :n]) / 2
        out[:, 0] = out[:, 0] / r2
        return out * np.sqrt(two / dtype.type(n))
    if dct_type == 3:
        x[:, 0] = x[:, 0] * r2
        rev = x[:, ::-1]
        spec = _ext_fft([(0, n, 1, x), (n + 1, 2 * n + 1, 1, -rev), (2 * n + 1, 3 * n, 1, -x[:, 1:]), (3 * n + 1, 4 * n, 1, x[:, :0:-1])], 4 * n, dtype)
        return np.real(spec[:, 1:2 * n:2]) / 4 * np.sqrt(two / dtype.type(n))
    if dct_type == 4:
        spec = _ext_fft([(1, 2 * n, 2, x), (2 * n + 1, 4 * n, 2, -rev), (4 * n + 1, 6 * n, 2, -x), (6 * n + 1, 8 * n, 2, rev)], 8 * n, dtype)
        return np.real(spec[:, 1:2 * n:2]) / 4 * np.sqrt(two / dtype.type(n))
    raise ValueError("dct_type must be 1, 2, 3 or 4")


def dst(x, dst_type, dtype):
    """(B, N) -> (B, N): the orthonormal DST-I .. IV of every row by the FFT of an antisymmetric extension."""
    dtype = real_of(dtype)
    x = _clips(x, dtype).copy()
    n = x.shape[1]
    two = dtype.type(2)
    r2 = np.sqrt(two)
    rev = x[:, ::-1]
    if dst_type == 1:
        spec = _ext_fft([(1, n + 1, 1, x), (n + 2, 2 * n + 2, 1, -rev)], 2 * n + 2, dtype)
        return -np.imag(spec[:, 1:n + 1]) / 2 * np.sqrt(two / dtype.type(n + 1))
    if dst_type == 2:
        out = -np.imag(_ext_fft([(1, 2 * n, 2, x), (2 * n + 1, 4 * n, 2, -rev)], 4 * n, dtype)[:, 1:n + 1]) / 2
        out[:, -1] = out[:, -1] / r2
        return out * np.sqrt(two / dtype.type(n))
    if dst_type == 3:
        x[:, -1] = x[:, -1] * r2
        spec = _ext_fft([(1, n + 1, 1, x), (n + 1, 2 * n, 1, x[:, -2::-1]), (2 * n + 1, 3 * n + 1, 1, -x), (3 * n + 1, 4 * n, 1, -x[:, -2::-1])], 4 * n, dtype)
        return -np.imag(spec[:, 1:2 * n:2]) / 4 * np.sqrt(two / dtype.type(n))
    if dst_type == 4:
        spec = _ext_fft([(1, 2 * n, 2, x), (2 * n + 1, 4 * n, 2, rev), (4 * n + 1, 6 * n, 2, -x), (6 * n + 1, 8 * n, 2, -rev)], 8 * n, dtype)
        return -np.imag(spec[:, 1:2 * n:2]) / 4 * np.sqrt(two / dtype.type(n))
    raise ValueError("dst_type must be 1, 2, 3 or 4")


# ------------------------------------------------------------------------------------------------ the dense linear map
def linear(x, matrix, dtype):
    """(B, cols) -> (B, rows): matrix @ x for every row of x."""
    dtype = real_of(dtype)
    out = np.matmul(_clips(x, dtype), np.asarray(matrix).astype(dtype).T)
    assert out.dtype == dtype
    return out


def linear_chain(x, matrix, dtype):
    """(B, cols) -> (B, rows) as ONE accumulator per output, k ascending: acc = dtype(acc + dtype(a_k * b_k)).

    What np.matmul computes depends on the shape (BLAS's vector form runs 8 interleaved partial sums, blocked forms more), and at rows of
    thousands of columns its error is several times below any single chain's: no yardstick for kernels that ARE a single chain
    (tests/accuracy_cases.py, OWN_FACTORS).  This one is: vectorised over clips and rows, a Python loop over k, the matrix transposed once
    so that every step reads one contiguous row.  Unfused -- product and sum are rounded separately --, so slightly above a fused chain."""
    dtype = real_of(dtype)
    x = _clips(x, dtype)
    mt = np.ascontiguousarray(np.asarray(matrix).astype(dtype).T)   # (cols, rows)
    assert mt.shape[0] == x.shape[1], (mt.shape, x.shape)
    acc = np.zeros((x.shape[0], mt.shape[1]), dtype)
    term = np.empty_like(acc)
    for k in range(mt.shape[0]):
        np.multiply(x[:, k:k + 1], mt[k][None, :], out=term)
        np.add(acc, term, out=acc)
    return acc
