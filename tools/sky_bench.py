"""Sky light (include/vct_sky.h) on one GPU: the atrium at 256^3 (or --scene / --n), the bench's
1080p G_scene frame, 9 diffuse cones (workload C3).  One JSON line, also written to
profiles/sky_bench.json.  Device events on the context's stream, warmed; every figure is the
median of `--blocks` blocks of back-to-back calls, each block grown until its calls fill
`--window` seconds (at least 0.5; `window_s` is the shortest block kept), with the fastest and
slowest block beside it.

  sky_cones:   ms per vct_sky_cones_device call, its cone steps and G cone-steps/s (also with
               the add into the diffuse plane)
  inject_sky:  ms of vct_inject_lights + vct_build_mips + vct_inject_sky minus the pair alone,
               the stages of one call from events (march, add, K3; vct_debug_sky), the sources
  frame:       a relit frame (inject_lights + build_mips [+ inject_sky] + K4 [+ sky_cones]),
               queued back to back, with and without the sky
  comparison points of the same session:
    shadow:    vct_shadow_cones_device at tan_half 0.3, the sun plus the 8 gallery lamps of
               tools/shadow_bench.py (the same alpha loads, per-lane directions)
    k4:        vct_trace_device on the frame without the specular cone (the diffuse cones the
               sky call repeats) and with it, counted; and the plain `bench.py` line unless --no-k4
  `stage_check`: level 0 after inject_sky differs from level 0 before in rgb at sources only.
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sky_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import vct
    from vct import Context, _lib, scenes
    from vct.camera import Camera
    n, w, h = a.n, a.width, a.height
    g0, E = scenes.grid_for_unit_box(n)
    arrays = scenes.SCENES[a.scene]().arrays()
    st = torch.cuda.current_stream()
    dev = torch.device("cuda")
    sun = vct.directional_light(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    lamps = [vct.point_light((x, -0.1, z), (1.0, 0.8, 0.5), 0.6) for x in (-0.78, 0.78) for z in (-0.7, -0.25, 0.2, 0.65)]
    sky = vct.sky_light((0.25, 0.45, 0.9), (0.7, 0.7, 0.65), (0.08, 0.07, 0.05))
    cam = Camera()
    eye = [float(x) for x in cam.position]

    def context(specular=True):
        c = Context(n, g0, E, aniso=True, n_diffuse=9, specular=specular)
        c.set_stream(st.cuda_stream)
        c.voxelize(*arrays)
        c.inject_lights([sun])
        c.build_mips()
        return c

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

    ctx = context()
    gb = tuple(torch.empty((h, w, 4), device=dev) for _ in range(3))
    ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
    diff, spec, sk = (torch.empty((h, w, 4), device=dev) for _ in range(3))
    steps = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    valid = int((gb[0][..., 3] != 0).sum().item())
    out = {"tool": "sky_bench", "scene": a.scene, "n": n, "cones": 9, "width": w, "height": h,
           "device": torch.cuda.get_device_name(0), "valid_pixels": valid, "blocks": a.blocks}

    def counted(fn):
        steps.zero_()
        fn(steps)
        torch.cuda.synchronize()
        return int(steps.item())

    def rate(row, key):
        row["G_cone_steps_per_s"] = round(row["cone_steps"] / (row[key]["ms"] * 1e-3) / 1e9, 3)
        return row

    # ---- the per-pixel call ----------------------------------------------------------------
    row = {"cone_steps": counted(lambda s: ctx.sky_cones_device(gb[0], gb[1], w, h, sky, sk, None, s)),
           "call": timed(lambda: ctx.sky_cones_device(gb[0], gb[1], w, h, sky, sk))}
    rate(row, "call")
    lit = sk[gb[0][..., 3] != 0]
    row["mean_vis"] = round(float(lit[:, 3].mean().item()), 4)
    row["address_path"] = _lib.debug_sky_path(ctx.lib, ctx.h)
    ctx.trace_device(*gb, w, h, eye, diff, spec)
    row["call_adding_to_diffuse"] = timed(lambda: ctx.sky_cones_device(gb[0], gb[1], w, h, sky, sk, diff))
    out["sky_cones"] = row

    # ---- comparison points of the same session ---------------------------------------------
    lights = [sun] + lamps
    vis = torch.zeros((len(lights), h, w), device=dev)
    th = [0.3] * len(lights)
    out["shadow_tan_0.3"] = rate({
        "lights": len(lights),
        "cone_steps": counted(lambda s: ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, th, vis, s)),
        "call": timed(lambda: ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, th, vis))}, "call")
    del vis

    def settle(c):           # K4 settled on the frame first (its timed choice of form)
        last, run = None, 0
        for _ in range(256):
            c.trace_device(*gb, w, h, eye, diff, spec)
            torch.cuda.synchronize()
            f = c.trace_form
            run = run + 1 if (f >= 0 and f == last) else 0
            last = f
            if run >= 24:
                break

    settle(ctx)
    out["k4_frame"] = rate({
        "cone_steps": counted(lambda s: ctx.trace_device(*gb, w, h, eye, diff, spec, cone_steps=s)),
        "call": timed(lambda: ctx.trace_device(*gb, w, h, eye, diff, spec))}, "call")
    dctx = context(specular=False)
    settle(dctx)
    out["k4_diffuse_only"] = rate({
        "cone_steps": counted(lambda s: dctx.trace_device(*gb, w, h, eye, diff, spec, cone_steps=s)),
        "call": timed(lambda: dctx.trace_device(*gb, w, h, eye, diff, spec))}, "call")
    dctx.close()
    out["sky_steps_equal_k4_diffuse_steps"] = out["sky_cones"]["cone_steps"] == out["k4_diffuse_only"]["cone_steps"]

    # ---- the per-voxel call ------------------------------------------------------------------
    def relight():
        ctx.inject_lights([sun])
        ctx.build_mips()

    def relight_sky():
        relight()
        ctx.inject_sky(sky)

    relight()
    L0 = ctx.download_level(0)
    ao, nm = ctx.download_voxels()
    _lib.debug_sky(ctx.lib, ctx.h, profile=1)
    ctx.inject_sky(sky)                                       # the first call also builds the source list
    relight_sky()
    stages = _lib.debug_sky(ctx.lib, ctx.h, profile=0)
    L1 = ctx.download_level(0)
    src = (ao[..., 3] != 0) & np.any(nm[..., :3] != 0, axis=-1)
    changed = np.any(L0.view(np.uint32) != L1.view(np.uint32), axis=-1)
    stage_ok = bool(not (changed & ~src).any() and changed.any() and
                    np.array_equal(L0[..., 3].view(np.uint32), L1[..., 3].view(np.uint32)))
    alone, pair = timed(relight), timed(relight_sky)
    out["inject_sky"] = {"sources": int(src.sum()), "sources_changed": int(changed.sum()),
                         "relight": alone, "relight_then_inject_sky": pair,
                         "inject_sky_ms": round(pair["ms"] - alone["ms"], 4),
                         "stages_ms": {"march": round(stages[0], 4), "add": round(stages[1], 4), "k3": round(stages[2], 4)}}
    out["stage_check"] = stage_ok
    del L0, L1, ao, nm

    # ---- the relit frame ----------------------------------------------------------------------
    def frame(with_sky):
        def fn():
            relight()
            if with_sky:
                ctx.inject_sky(sky)
            ctx.trace_device(*gb, w, h, eye, diff, spec)
            if with_sky:
                ctx.sky_cones_device(gb[0], gb[1], w, h, sky, sk, diff)
        return fn
    out["frame_relight"] = timed(frame(False))
    out["frame_relight_with_sky"] = timed(frame(True))
    out["trace_form"] = ctx.trace_form
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
    if not stage_ok:
        raise SystemExit("inject_sky changed something other than the rgb of the sources")


if __name__ == "__main__":
    main()
