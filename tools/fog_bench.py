"""Volumetric fog (include/vct_fog.h) on one GPU: the atrium with the sun and the 8 gallery lamps
of tools/lights_bench.py at `level` 2 and 3 and `step` 1 and 0.5, and the courtyard with the
sun, at 256^3 (or --n), the bench's 1080p G_scene frame.  One JSON line, also written to
profiles/fog_bench.json.  tools/mixed_bench.py's method: device events on the context's stream,
warmed; every figure is the median of `--blocks` blocks of back-to-back calls, each block grown
until its calls fill `--window` seconds, with the fastest and slowest block beside it.

Per scene and level:
  build:     vct_build_fog with the lights alone (ambient 0: the light cones and the combine, one
             kernel), with the ambient term alone (no light: the records, the two-sided K4 gather
             and the combine) and with both; the light cones' and the gather's cone steps
  per step:  rays, march (its sample count and samples/s, and the bytes its loads ask of the
             cache: 8 corners x 16 bytes per sample) and apply
  frame:     a relit frame (inject_lights + build_mips + K4 + composite) without fog, and with
             it (+ build_fog + rays + march + apply)
Yardsticks of the same session, on the same frame: vct_sky_cones_device and the shadow march at
the fog's aperture over the same lights.  (The bounce gather's rate, the yardstick of the
ambient launch, is tools/bounce_bench.py's: run it in the same session.)
--march-only SCENE,LEVEL,STEP runs the march alone a few times (for a counter pass of its own).
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd")]

TAN = 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--scenes", default="atrium,courtyard")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--density", type=float, default=1.0)
    ap.add_argument("--march-only", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "fog_bench.json"))
    a = ap.parse_args()
    import torch
    import vct
    from vct import Context, _lib, scenes
    from vct.camera import Camera
    n, w, h = a.n, a.width, a.height
    g0, E = scenes.grid_for_unit_box(n)
    st = torch.cuda.current_stream()
    dev = torch.device("cuda")
    sun = vct.directional_light(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    lamps = [vct.point_light((x, -0.1, z), (1.0, 0.8, 0.5), 0.6) for x in (-0.78, 0.78) for z in (-0.7, -0.25, 0.2, 0.65)]
    sky = vct.sky_light((0.25, 0.45, 0.9), (0.7, 0.7, 0.65), (0.08, 0.07, 0.05))
    cam = Camera()
    eye = [float(x) for x in cam.position]

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
                "calls": reps * a.blocks}

    def scene_ctx(scene, lights):
        ctx = Context(n, g0, E, aniso=True, n_diffuse=9, specular=True)
        ctx.set_stream(st.cuda_stream)
        ctx.voxelize(*scenes.SCENES[scene]().arrays())
        ctx.inject_lights(lights)
        ctx.build_mips()
        gb = tuple(torch.empty((h, w, 4), device=dev) for _ in range(3))
        ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
        torch.cuda.synchronize()
        return ctx, gb

    if a.march_only:
        scene, level, step = a.march_only.split(",")
        lights = [sun] + lamps if scene == "atrium" else [sun]
        ctx, gb = scene_ctx(scene, lights)
        f = vct.fog(a.density, level=int(level), step=float(step))
        ctx.build_fog(f, lights, [TAN] * len(lights))
        ray, fog4 = (torch.empty((h, w, 4), device=dev) for _ in range(2))
        ctx.fog_rays_device(cam, eye, gb[0], w, h, ray)
        for _ in range(5):
            ctx.fog_march_device(f, eye, ray, w, h, fog4)
        torch.cuda.synchronize()
        ctx.close()
        print(json.dumps({"tool": "fog_bench", "march_only": a.march_only, "launches": 5}))
        return

    out = {"tool": "fog_bench", "n": n, "width": w, "height": h, "device": torch.cuda.get_device_name(0),
           "blocks": a.blocks, "density": a.density, "tan_half": TAN, "scenes": {}}
    for scene in a.scenes.split(","):
        lights = [sun] + lamps if scene == "atrium" else [sun]
        ctx, gb = scene_ctx(scene, lights)
        th = [TAN] * len(lights)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        ray, fog4, d, s, lin, sk = (torch.empty((h, w, 4), device=dev) for _ in range(6))
        for _ in range(96):                 # the tuner's timed choice of the frame's K4 workload
            ctx.trace_device(*gb, w, h, eye, d, s)
            torch.cuda.synchronize()
        row = {"lights": len(lights), "valid_pixels": int((gb[0][..., 3] != 0).sum().item()), "levels": {}}
        for level in ((2, 3) if scene == "atrium" else (2,)):
            m = n >> level
            lr = {"cells": m ** 3, "volume_bytes": 16 * m ** 3, "build": {}, "steps": {}}
            for name, f, ll in (("lights_only", vct.fog(a.density, ambient=0.0, level=level), lights),
                                ("ambient_only", vct.fog(a.density, ambient=1.0, level=level), []),
                                ("both", vct.fog(a.density, ambient=1.0, level=level), lights)):
                _lib.debug_fog(ctx.lib, ctx.h, counters=(0, 0))
                call = timed(lambda: ctx.build_fog(f, ll, [TAN] * len(ll)))
                cnt.zero_()
                _lib.debug_fog(ctx.lib, ctx.h, counters=(cnt.data_ptr(), cnt.data_ptr() + 8))
                ctx.build_fog(f, ll, [TAN] * len(ll))
                torch.cuda.synchronize()
                _lib.debug_fog(ctx.lib, ctx.h, counters=(0, 0))
                light_steps, amb_steps = int(cnt[0].item()), int(cnt[1].item())
                call.update(light_cone_steps=light_steps, ambient_cone_steps=amb_steps,
                            G_cone_steps_per_s=round((light_steps + amb_steps) / (call["ms"] * 1e-3) / 1e9, 2))
                lr["build"][name] = call
            for step in ((1.0, 0.5) if scene == "atrium" else (1.0,)):
                f = vct.fog(a.density, ambient=1.0, level=level, step=step)
                ctx.build_fog(f, lights, th)
                steps = torch.zeros(1, dtype=torch.int64, device=dev)
                ctx.fog_rays_device(cam, eye, gb[0], w, h, ray)
                ctx.fog_march_device(f, eye, ray, w, h, fog4, steps)
                torch.cuda.synchronize()
                samples = int(steps.item())
                sr = {"rays": timed(lambda: ctx.fog_rays_device(cam, eye, gb[0], w, h, ray)),
                      "march": timed(lambda: ctx.fog_march_device(f, eye, ray, w, h, fog4)),
                      "apply": timed(lambda: ctx.fog_apply_device(fog4, w, h, lin)),
                      "samples": samples, "mean_T": float(fog4[..., 3].mean().item())}
                ms = sr["march"]["ms"] * 1e-3
                sr["G_samples_per_s"] = round(samples / ms / 1e9, 2)
                sr["requested_bytes_per_sample"] = 128
                sr["requested_TB_per_s"] = round(samples * 128 / ms / 1e12, 2)

                def relit(fog_on):
                    ctx.inject_lights(lights)
                    ctx.build_mips()
                    if fog_on:
                        ctx.build_fog(f, lights, th)
                    ctx.trace_device(*gb, w, h, eye, d, s)
                    ctx.composite_lights_device(*gb, d, s, w, h, lights, out_linear4=lin)
                    if fog_on:
                        ctx.fog_rays_device(cam, eye, gb[0], w, h, ray)
                        ctx.fog_march_device(f, eye, ray, w, h, fog4)
                        ctx.fog_apply_device(fog4, w, h, lin)
                sr["relit_frame"] = timed(lambda: relit(False))
                sr["relit_frame_with_fog"] = timed(lambda: relit(True))
                lr["steps"][str(step)] = sr
            row["levels"][str(level)] = lr
        # ---- yardsticks of the same session, on the same frame ------------------------------
        ctx.inject_lights(lights)
        ctx.build_mips()
        c1 = torch.zeros(1, dtype=torch.int64, device=dev)
        ctx.sky_cones_device(gb[0], gb[1], w, h, sky, sk, None, c1)
        torch.cuda.synchronize()
        y = {"sky_cones": timed(lambda: ctx.sky_cones_device(gb[0], gb[1], w, h, sky, sk))}
        y["sky_cones"].update(cone_steps=int(c1.item()),
                              G_cone_steps_per_s=round(int(c1.item()) / (y["sky_cones"]["ms"] * 1e-3) / 1e9, 2))
        vis = torch.zeros((len(lights), h, w), device=dev)
        c1.zero_()
        ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, th, vis, c1)
        torch.cuda.synchronize()
        y["shadow_march"] = timed(lambda: ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, th, vis))
        y["shadow_march"].update(cone_steps=int(c1.item()),
                                 G_cone_steps_per_s=round(int(c1.item()) / (y["shadow_march"]["ms"] * 1e-3) / 1e9, 2))
        row["yardsticks"] = y
        out["scenes"][scene] = row
        ctx.close()
        del ctx, gb
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
