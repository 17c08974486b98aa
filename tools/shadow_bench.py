"""vct_shadow_cones_device on one GPU: the atrium at 256^3 (or --scene / --n), the bench's
1080p G_scene frame, the directional light plus the 8 gallery lamps of tools/lights_bench.py.
One JSON line, also written to profiles/shadow_bench.json.  Device events on the context's
stream, warmed; every figure is the median of `--blocks` blocks of back-to-back calls, each
block grown until its calls fill `--window` seconds (at least 0.5; `window_s` is the shortest
block kept), with the fastest and slowest block beside it.

  per tan_half in 0.02, 0.1, 0.3 (every light of the frame):
      ms per shadow call, cone steps, G cone-steps/s, ms of the shadowed composite
  hard:  the same call with tan_half 0 (the voxel walk into the vis planes), and
         vct_composite_lights_device on the same frame: what the hard shadows cost
  k4:    the plain `bench.py` line of the same session (its Mcone-steps/s), unless --no-k4
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--scene", default="atrium")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--no-k4", action="store_true", help="do not run the plain bench.py line")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shadow_bench.json"))
    a = ap.parse_args()
    import torch
    import vct
    from vct import Context, scenes
    from vct.camera import Camera
    n, w, h = a.n, a.width, a.height
    g0, E = scenes.grid_for_unit_box(n)
    ctx = Context(n, g0, E)
    st = torch.cuda.current_stream()
    ctx.set_stream(st.cuda_stream)
    ctx.voxelize(*scenes.SCENES[a.scene]().arrays())
    sun = vct.directional_light(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    lamps = [vct.point_light((x, -0.1, z), (1.0, 0.8, 0.5), 0.6) for x in (-0.78, 0.78) for z in (-0.7, -0.25, 0.2, 0.65)]
    lights = [sun] + lamps
    ctx.inject_lights(lights)
    ctx.build_mips()
    dev = torch.device("cuda")
    cam = Camera()
    gb = tuple(torch.empty((h, w, 4), device=dev) for _ in range(3))
    ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
    diff, spec, lin = (torch.empty((h, w, 4), device=dev) for _ in range(3))
    ctx.trace_device(*gb, w, h, [float(x) for x in cam.position], diff, spec)
    vis = torch.zeros((len(lights), h, w), device=dev)
    steps = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def block(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps, ms = 3, []
        while len(ms) < a.blocks:           # a block counts once its calls filled the window
            t = block(fn, reps)
            if t * reps * 1e-3 >= a.window:
                ms.append(t)
            else:
                reps = int(reps * max(1.1 * a.window / max(t * reps * 1e-3, 1e-6), 1.25)) + 1
        return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                "calls": reps * a.blocks, "window_s": round(reps * min(ms) * 1e-3, 3)}

    def cones(tan):
        th = [tan] * len(lights)
        return lambda: ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, th, vis)

    def counted(tan):
        steps.zero_()
        ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, [tan] * len(lights), vis, steps)
        torch.cuda.synchronize()
        return int(steps.item())

    shadowed = lambda: ctx.composite_shadowed_device(*gb, diff, spec, w, h, lights, vis, out_linear4=lin)
    valid = int((gb[0][..., 3] != 0).sum().item())
    out = {"scene": a.scene, "n": n, "width": w, "height": h, "device": torch.cuda.get_device_name(0),
           "lights": len(lights), "valid_pixels": valid, "blocks": a.blocks, "sweep": []}
    for tan in (0.02, 0.1, 0.3):
        row = {"tan_half": tan, "cone_steps": counted(tan), "shadow": timed(cones(tan))}
        row["G_cone_steps_per_s"] = round(row["cone_steps"] / (row["shadow"]["ms"] * 1e-3) / 1e9, 3)
        lit = vis[:, gb[0][..., 3] != 0]
        row["mean_V"] = round(float(lit.mean().item()), 4)
        row["penumbra_share"] = round(float(((lit > 0.05) & (lit < 0.95)).float().mean().item()), 4)
        row["composite_shadowed"] = timed(shadowed)
        out["sweep"].append(row)
    out["hard"] = {
        "shadow_tan_0": timed(cones(0.0)),
        "composite_shadowed": timed(shadowed),
        "composite_lights": timed(lambda: ctx.composite_lights_device(*gb, diff, spec, w, h, lights, out_linear4=lin)),
    }
    ctx.close()
    del ctx
    if not a.no_k4:
        # the plain bench.py line in a process of its own, while this one holds no context
        p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")], capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("{")]
        k4 = json.loads(line[-1]) if p.returncode == 0 and line else None
        out["k4_bench_line"] = None if k4 is None else {key: k4.get(key) for key in ("value", "unit", "ms_per_step")}
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
