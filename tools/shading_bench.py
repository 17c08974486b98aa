"""The shading G-buffer (include/vct_shading.h) on one GPU: the atrium and the courtyard with
smooth normals (vct.shading.smooth; planar TexCoords so that the maps are sampled) at 256^3, the
bench's 1080p frame.  One JSON line, also written to profiles/shading_bench.json.  Device events
on the context's stream, warmed; every figure is the median of `--blocks` blocks of back-to-back
calls, each block grown until its calls fill `--window` seconds (`window_s` is the shortest block
kept), with the fastest and slowest block beside it.  No counters are collected here.

  per scene:
    raster:        vct_gbuffer_raster_device on the same frame in the same session: the yardstick
    shaded_*:      vct_gbuffer_shaded_device with no maps; with normal maps; with normal and
                   specular maps and all optional outputs (geo4, tri_id, bary2); `ratio` to raster
    floor:         the compulsory traffic of the extra planes: written bytes / the float4 copy rate
                   of the session (a device-to-device copy of one plane: bytes written per second),
                   and how far above raster + floor each form runs (`over_floor`)
    set_shading:   vct_set_shading wall time, host clock around the synchronous call, 5 calls
    tint:          vct_specular_tint_device, in place
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--scenes", default="atrium,courtyard")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--tex", type=int, default=512, help="edge of the two maps")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "shading_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from vct import Context, scenes
    from vct.camera import Camera
    from vct.shading import ShadingMaterial, smooth
    n, w, h = a.n, a.width, a.height
    g0, E = scenes.grid_for_unit_box(n)
    st = torch.cuda.current_stream()
    dev = torch.device("cuda")
    cam = Camera()

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

    rng = np.random.default_rng(9)
    nmap = rng.integers(96, 160, (a.tex, a.tex, 4), dtype=np.uint8)
    nmap[..., 2] = 255
    smap = rng.integers(0, 256, (a.tex, a.tex, 4), dtype=np.uint8)
    planes = {k: torch.zeros((h, w, 4), device=dev) for k in ("pos", "nrm", "alb", "ks", "geo", "src")}
    tri_id = torch.empty((h, w), dtype=torch.int32, device=dev)
    bary = torch.empty((h, w, 2), device=dev)
    out = {"tool": "shading_bench", "n": n, "width": w, "height": h, "maps": f"{a.tex} x {a.tex} RGBA8, bilinear",
           "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "counters": "none: device-event times only"}
    copy = timed(lambda: planes["geo"].copy_(planes["src"]))
    plane_bytes = w * h * 16
    rate = plane_bytes / (copy["ms"] * 1e-3)
    out["float4_copy"] = dict(copy, plane_bytes=plane_bytes, written_GBps=round(rate / 1e9, 1))
    out["scenes"] = {}
    for name in a.scenes.split(","):
        verts, idx, mat, kd = scenes.SCENES[name]().arrays()
        verts = verts.copy()
        verts[:, 6] = (verts[:, 0] + verts[:, 2]) * 2.0          # planar TexCoords: the maps are sampled
        verts[:, 7] = verts[:, 1] * 2.0
        t0 = time.perf_counter()
        verts, idx, mat, kd = smooth((verts, idx, mat, kd))
        smooth_s = time.perf_counter() - t0
        ctx = Context(n, g0, E)
        ctx.set_stream(st.cuda_stream)
        ctx.set_textures([nmap, smap])
        ctx.voxelize(verts, idx, mat, kd)
        nm = kd.shape[0]
        forms = {
            "no_maps": [ShadingMaterial((0.8, 0.8, 0.8), 0.1 + 0.05 * (j % 8)) for j in range(nm)],
            "normal_maps": [ShadingMaterial((0.8, 0.8, 0.8), 0.1 + 0.05 * (j % 8), normal_map=0) for j in range(nm)],
            "normal_specular_all_outputs": [ShadingMaterial((0.8, 0.8, 0.8), 0.1 + 0.05 * (j % 8), normal_map=0, specular_map=1)
                                            for j in range(nm)],
        }
        row = {"triangles": int(idx.size // 3), "materials": int(nm), "smooth_host_s": round(smooth_s, 2)}
        row["raster"] = timed(lambda: ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, planes["pos"], planes["nrm"],
                                                                planes["alb"]))
        torch.cuda.synchronize()
        row["valid_pixels"] = int((planes["pos"][..., 3] != 0).sum().item())
        wall = []
        for k, mats in forms.items():
            for _ in range(5 if k == "no_maps" else 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.set_shading(verts, idx, mat, mats)
                wall.append((time.perf_counter() - t0) * 1e3)
            extra = (planes["geo"], tri_id, bary) if k.endswith("all_outputs") else ()
            r = timed(lambda: ctx.gbuffer_shaded_device(cam, w, h, scenes.ROUGHNESS, planes["pos"], planes["nrm"], planes["alb"],
                                                        planes["ks"], *extra))
            written = w * h * (16 + (28 if extra else 0))
            floor = written / rate * 1e3
            r.update(ratio=round(r["ms"] / row["raster"]["ms"], 3), extra_written_bytes=written, floor_ms=round(floor, 4),
                     over_floor=round(r["ms"] / (row["raster"]["ms"] + floor), 3))
            row["shaded_" + k] = r
        row["set_shading_wall_ms"] = {"ms": round(statistics.median(wall[1:5]), 3), "min": round(min(wall[1:]), 3),
                                      "max": round(max(wall[1:]), 3), "first_call": round(wall[0], 3)}
        out["scenes"][name] = row
        out["tint"] = timed(lambda: ctx.specular_tint_device(planes["src"], planes["ks"], w, h))
        ctx.close()
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
