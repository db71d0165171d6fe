"""The cases of tests/test_gpu_linear.py, tests/test_linear_host.py and the linear/ lines of tests/test_gpu_accuracy.py.  Host only.

zafx_linear.hip holds two matrix-core kernels behind one launcher.  Its rule, written out once (`kernel`): k_linear128 when the column count
is a multiple of its K tile (32), the clips and the plan's matrix start on 16-byte boundaries and rows x clips >= 128 x 128 x 64; k_linear
otherwise.  The matrix is the plan's own allocation, always on that grid, so of the two addresses only the clips' can vary.

A case is (rows, cols, clips) and is there for the branches `geometry` names:

  k_linear     64 x 64 output tile, K tile 32 staged in 4-float pieces with a bounds test per element
    (1, 1, 1)          every side 1
    (65, 33, 65)       every side one past a tile: two row tiles, two K tiles (the second holds one column), two clip tiles
    (63, 31, 130)      every side one short of a tile; three clip tiles, the last with 2 clips
    (129, 64, 70)      three row tiles, a whole number of K tiles
  k_linear128  128 x 128 output tile, K tile 32 double-buffered from registers to LDS, float4 stores where rows % 4 == 0 and y is aligned
    (8191, 96, 129)    three K tiles (both buffers, buffer 0 used again), rows % 4 != 0: scalar stores; a last row tile of 127 rows; a second
                       clip tile with ONE clip, behind which the staging reads are clamped to it
    (4100, 64, 256)    two K tiles, float4 stores, a last row tile of exactly one float4 group (4 rows), two whole clip tiles
    (1024, 4096, 1024) 128 K tiles: the accuracy case (tests/test_gpu_accuracy.py), not an arena case

Inputs: the matrix is default_rng([rows, cols]).standard_normal rounded to float32, the clips conftest.synth_clip plus a little further noise
-- white, so no output row has a vanishing reference.  Reference: x @ m.T in float64 on those float32 values."""
import numpy as np

from conftest import synth_clip

SMALL_TILE, BIG_TILE, K_TILE = 64, 128, 32     # kLinTile, kBigTile, kLinK == kBigK
BIG_WORK = 128 * 128 * 64                      # rows x clips from which the launcher takes the 128-tile kernel

ARENA_CASES = [(1, 1, 1), (65, 33, 65), (63, 31, 130), (129, 64, 70), (8191, 96, 129), (4100, 64, 256)]
LONG_ROWS = (1024, 4096, 1024)
CASES = ARENA_CASES + [LONG_ROWS]
BIG_ARENA_CASES = [(8191, 96, 129), (4100, 64, 256)]

DCT_N, DCT_CLIPS, DCT_DISTINCT = 8224, 130, 16   # dct-II by the dense matrix: 32 * 257 columns, N / 2 no power of two
N_JUDGED = 16


def kernel(rows, cols, clips, x_offset=0):
    """launch_linear's choice for clips that start `x_offset` bytes off the 16-byte grid."""
    return "k_linear128" if cols % K_TILE == 0 and x_offset % 16 == 0 and rows * clips >= BIG_WORK else "k_linear"


def geometry(rows, cols, clips, x_offset=0, y_offset=0):
    """The launch as the chosen kernel sees it: tile counts, the last tiles' extents, the store form."""
    name = kernel(rows, cols, clips, x_offset)
    tile = BIG_TILE if name == "k_linear128" else SMALL_TILE
    return {"kernel": name, "tile": tile,
            "k_tiles": -(-cols // K_TILE), "last_k_tile": cols - (-(-cols // K_TILE) - 1) * K_TILE,
            "row_tiles": -(-rows // tile), "last_row_tile": rows - (-(-rows // tile) - 1) * tile,
            "clip_tiles": -(-clips // tile), "last_clip_tile": clips - (-(-clips // tile) - 1) * tile,
            "float4_stores": name == "k_linear128" and rows % 4 == 0 and y_offset % 16 == 0}


def name_of(case):
    return "%dx%dx%d" % tuple(case)


def matrix(rows, cols):
    return np.random.default_rng([rows, cols]).standard_normal((rows, cols)).astype(np.float32)


def clips(rows, cols, count):
    x = np.stack([synth_clip(rows, c, cols) for c in range(count)])
    return x + np.float32(2.0 ** -6) * np.random.default_rng([rows, cols, count]).standard_normal(x.shape).astype(np.float32)


def reference(x, m):
    return x.astype(np.float64) @ m.astype(np.float64).T


def judged(count):
    """The clips the accuracy lines measure: the first 8 and the last 8 (every clip where there are no more than 16).  Fewer than 16 would
    make e_row a maximum over rms estimates of a handful of samples."""
    return np.arange(count) if count <= N_JUDGED else np.r_[0:N_JUDGED // 2, count - N_JUDGED // 2:count]


def dct_clips(n=DCT_N, count=DCT_CLIPS, distinct=DCT_DISTINCT):
    """`distinct` vectors, replicated to `count` clips: the replicas land in other tiles and must come back as the same bits."""
    return np.stack([synth_clip(n, c % distinct, n) for c in range(count)])


def fused_chain(x, m):
    """What v_mfma_f32_16x16x4_f32 computes per output (tests/accuracy_cases.py, OWN_FACTORS): acc = float32(fma(a_k, b_k, acc)), k ascending.
    A product of two float32 values is exact in float64; the float64 sum is rounded once more to float32 -- off a true fma only where the
    float64 sum itself lands within 2^-29 of a float32 tie."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    mt = np.ascontiguousarray(np.asarray(m, np.float32).astype(np.float64).T)
    acc = np.zeros((x64.shape[0], mt.shape[1]), np.float32)
    for k in range(mt.shape[0]):
        acc = (acc.astype(np.float64) + x64[:, k:k + 1] * mt[k][None, :]).astype(np.float32)
    return acc
