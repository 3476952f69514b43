"""A plain bench run (no --full) in a fresh child process, on a tiny frame: it runs exactly --steps timed
steps, its line carries the headline fields and none of the --full blocks, and --dump-outputs writes the
last timed step's frame, which equals a direct render of the same arguments through the C ABI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

W, H, SPP, SEED = 64, 48, 8, 0x5EED


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_frame(rt, gpu_scenes, tmp_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_"))}
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--width", str(W), "--height",
           str(H), "--spp", str(SPP), "--seed", hex(SEED), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    # value and ms_per_step are two views of the same timed region (both rounded to 3 decimals)
    samples = W * H * 4 * (SPP // 4)
    assert line["value"] == pytest.approx(samples / (line["ms_per_step"] / 1e3) / 1e6, rel=0.01, abs=2e-3)
    assert "roofline" not in line and "cpu_baseline" not in line
    assert "frame_sha1" not in line["config"] and "vertices" not in line["config"]
    assert os.listdir(out_dir) == ["frame_rgb.npy"]
    frame = np.load(out_dir / "frame_rgb.npy")
    assert frame.dtype == np.float32 and frame.shape == (H, W, 3)
    rgb, _, _ = rt.render(gpu_scenes["cornell_box"], W, H, SPP, SEED, megakernel=True)
    assert np.array_equal(frame, rgb.astype(np.float32))
