"""A plain `bench.py --gpus 1 --steps K --warmup W` times the headline and nothing else, and --dump-outputs writes what its last
timed step computed: the sampled clips of the STFT output, each within tolerance of the NumPy oracle on its input clip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr, synth_clip

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(600)
def test_plain_run_with_dump_outputs(tmp_path):
    from oracle import zaf_oracle as orc
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "ZAFX_RDZV_DIR", "ZAFX_RDZV_NS")}
    env["ZAFX_BENCH_PREWARM_S"] = "0.1"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=500)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-1000:]
    line = json.loads(lines[0])
    assert line["metric"] == "audio Msamples/sec (STFT win=2048 hop=1024)" and line["unit"] == "Msamples/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["value"] - 1024 * 441000 / (line["ms_per_step"] * 1e-3) / 1e6) < 1e-3 * line["value"]
    for key in ("configs", "extras", "cpu_baseline", "parity", "end_to_end_pcie"):   # (--full only)
        assert key not in line, key
    assert sorted(os.listdir(tmp_path)) == ["stft.npy"]
    out = np.load(tmp_path / "stft.npy")
    assert out.dtype == np.float32 and out.shape == (8, 2048, 432, 2) and out.nbytes <= 64_000_000
    clips = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(1024, 8, replace=False))
    ham = orc.hamming_periodic(2048)
    for i in (0, 7):   # bench.py replicates 8 distinct clips: clip b holds synth(0, b % 8)
        ref = orc.stft(synth_clip(0, int(clips[i]) % 8, 441000).astype(np.float64), ham, 1024)
        assert relerr(out[i, ..., 0] + 1j * out[i, ..., 1].astype(np.float64), ref) <= 1e-5
