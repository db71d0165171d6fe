"""bench.py --dump-outputs: what the last timed step left in the output buffer, as float32 / float64 .npy files of at most
60 MB (a fixed, seeded sample of whole clips beyond that), with device row padding cut off.  The helper on stand-in buffers
(no GPU); the real run is tests/test_gpu_bench_plain.py."""
import numpy as np

import bench


class _Buf:
    def __init__(self, arr):
        self.arr, self.shape, self.dtype, self.nbytes = arr, arr.shape, arr.dtype, arr.nbytes

    def download(self, first=0, count=None):
        count = self.shape[0] - first if count is None else count
        return self.arr[first:first + count].copy()


class _Plan:
    def __init__(self, rows, frames, layout):
        self.rows, self.frames, self.layout = rows, frames, layout

    def out_dims(self, n_in):
        return self.rows, self.frames


def _wl(arr, rows, frames, kind="stft"):
    import zafx
    return {"kind": kind, "d_out": _Buf(arr), "n_clips": arr.shape[0], "n_in": 0, "plan": _Plan(rows, frames, zafx.LAYOUT_FT)}


def test_complex_output_becomes_float_pairs(tmp_path):
    rng = np.random.default_rng(3)
    out = (rng.standard_normal((4, 6, 5)) + 1j * rng.standard_normal((4, 6, 5))).astype(np.complex64)
    path, clips = bench.dump_outputs(_wl(out, 6, 5), str(tmp_path))
    got = np.load(path)
    assert path.endswith("stft.npy") and got.dtype == np.float32 and got.shape == (4, 6, 5, 2)
    assert np.array_equal(got[..., 0], out.real) and np.array_equal(got[..., 1], out.imag) and list(clips) == [0, 1, 2, 3]


def test_float64_stays_float64_and_padding_is_cut(tmp_path):
    out = np.arange(3 * 4 * 8, dtype=np.float64).reshape(3, 4, 8)   # pitch 8, 5 frames
    path, _ = bench.dump_outputs(_wl(out, 4, 5, kind="mdct64"), str(tmp_path))
    got = np.load(path)
    assert got.dtype == np.float64 and np.array_equal(got, out[:, :, :5])


def test_large_output_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 64 * 4)
    out = np.arange(100 * 64, dtype=np.float32).reshape(100, 64)   # (clips, samples): an inverse kind's output
    path, clips = bench.dump_outputs(_wl(out, 64, 1, kind="istft"), str(tmp_path / "a"))
    again, clips2 = bench.dump_outputs(_wl(out, 64, 1, kind="istft"), str(tmp_path / "b"))
    got = np.load(path)
    assert len(clips) == 10 and list(clips) == sorted(set(clips)) and list(clips) == list(clips2)
    assert got.nbytes <= bench.DUMP_LIMIT_BYTES and np.array_equal(got, out[clips]) and np.array_equal(got, np.load(again))


def test_headline_sample_fits_64_mb():
    per_clip = 2048 * 432 * 8   # one clip of the headline's (1024, 2048, 432) complex64 output
    assert 8 * per_clip <= bench.DUMP_LIMIT_BYTES <= 64_000_000
