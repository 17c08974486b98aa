"""bench.py on the GPU at a small size: a plain run prints the metric line without the
`--full` legs, and `--dump-outputs` writes the frame its timed path computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import gpu_pipeline

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, H = 32, 200, 130


@pytest.mark.gpu
def test_plain_run_and_dump(gpu_ready, tmp_path):
    """One plain run (3 timed steps): the line holds the metric fields and none of the
    `--full` ones; the dumped frame equals, bit for bit, a single trace of the same
    procedural scene, light, camera and rastered G-buffer made here."""
    import torch
    from vct import scenes
    from vct.camera import Camera
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "frame"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--n", str(N), "--width", str(W), "--height", str(H), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=240, env=env, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "Mcone-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and d["frame_cone_steps"] > 0
    assert d["value"] == pytest.approx(d["frame_cone_steps"] / d["ms_per_step"] / 1e3, rel=1e-3)
    for k in ("roofline", "cpu_baseline", "frame_loop", "stress", "secondary", "multi_config", "latency",
              "k4_kernel_ms_avg", "k1_voxelize_ms", "timed_equals_counting"):
        assert k not in d, k
    assert sorted(os.listdir(out)) == ["diffuse.npy", "spec.npy"]
    got_d, got_s = np.load(out / "diffuse.npy"), np.load(out / "spec.npy")
    assert got_d.dtype == got_s.dtype == np.float32 and got_d.shape == got_s.shape == (H, W, 4)

    ctx, _, _, _ = gpu_pipeline(N, "atrium")
    cam = Camera()
    dev = torch.device("cuda")
    gb = tuple(torch.empty((H, W, 4), device=dev) for _ in range(3))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.gbuffer_raster_device(cam, W, H, scenes.ROUGHNESS, *gb)
    ref_d, ref_s = torch.empty((H, W, 4), device=dev), torch.empty((H, W, 4), device=dev)
    ctx.trace_device(*gb, W, H, [float(x) for x in cam.position], ref_d, ref_s)
    torch.cuda.synchronize()
    assert np.array_equal(got_d, ref_d.cpu().numpy()) and np.array_equal(got_s, ref_s.cpu().numpy())
    assert np.isfinite(got_d).all() and got_d.any()
    ctx.close()
