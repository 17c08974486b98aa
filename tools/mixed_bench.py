"""The mixed-resolution trace (include/vct_mixed.h) on one GPU: the atrium and the courtyard at
256^3 (or --scenes / --n), the bench's 1080p G_scene frame, 9 diffuse cones + specular (workload
C3).  One JSON line, also written to profiles/mixed_bench.json.  tools/sky_bench.py's method:
device events on the context's stream, warmed; every figure is the median of `--blocks` blocks
of back-to-back calls, each block grown until its calls fill `--window` seconds (at least 0.5),
with the fastest and slowest block beside it.  Every K4 workload is settled (the tuner's choice
made) before it is timed.

Per scene:
  full:        vct_trace_device at full resolution (the yardstick, measured in the same session),
               its cone steps
  mixed_f2/4:  vct_trace_mixed_device at the header defaults: total ms, cone steps, and each
               stage on its own buffers (pick, K4 low, upsample with listing, K4 holes, scatter,
               K4 specular); the upsample's bytes and rate against the 6.29 TB/s float4 copy
               rate; kernel launches per frame; hole share, overflow count; max and mean
               |delta| of the diffuse plane's rgb and AO against the full trace over valid pixels
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd")]

COPY_RATE_TBS = 6.29      # measured float4 copy rate of the device (bytes read + written per second)
DIFF, SPEC = 1, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--scenes", default="atrium,courtyard")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mixed_bench.json"))
    a = ap.parse_args()
    import torch
    import vct
    from vct import Context, scenes
    from vct.camera import Camera
    n, w, h = a.n, a.width, a.height
    g0, E = scenes.grid_for_unit_box(n)
    st = torch.cuda.current_stream()
    dev = torch.device("cuda")
    sun = vct.directional_light(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
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
                "calls": reps * a.blocks, "window_s": round(reps * min(ms) * 1e-3, 3)}

    def settle(ctx, fn, frames=96):         # the tuner's timed choice of every K4 workload fn launches
        for _ in range(frames):
            fn()
            torch.cuda.synchronize()
        return ctx.trace_form

    out = {"tool": "mixed_bench", "n": n, "cones": "9 + specular", "width": w, "height": h,
           "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "copy_rate_TBs": COPY_RATE_TBS,
           "scenes": {}}
    for scene in a.scenes.split(","):
        ctx = Context(n, g0, E, aniso=True, n_diffuse=9, specular=True)
        ctx.set_stream(st.cuda_stream)
        ctx.voxelize(*scenes.SCENES[scene]().arrays())
        ctx.inject_lights([sun])
        ctx.build_mips()
        gb = tuple(torch.empty((h, w, 4), device=dev) for _ in range(3))
        ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
        full_d, full_s, d, s = (torch.empty((h, w, 4), device=dev) for _ in range(4))
        steps = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        valid = gb[0][..., 3] != 0
        nvalid = int(valid.sum().item())

        def counted(fn):
            steps.zero_()
            fn(steps)
            torch.cuda.synchronize()
            return int(steps.item())

        form = settle(ctx, lambda: ctx.trace_device(*gb, w, h, eye, full_d, full_s))
        row = {"valid_pixels": nvalid,
               "full": {"call": timed(lambda: ctx.trace_device(*gb, w, h, eye, full_d, full_s)), "trace_form": form,
                        "cone_steps": counted(lambda c: ctx.trace_device(*gb, w, h, eye, full_d, full_s, cone_steps=c))}}
        for f in (2, 4):
            p = ctx.mixed_params(f)
            wl, hl = (w + f - 1) // f, (h + f - 1) // f
            m = ctx.mixed_max_holes(w, h)
            rows = (m + 63) // 64
            frame = lambda: ctx.trace_mixed_device(p, *gb, w, h, eye, d, s)
            settle(ctx, frame)
            r = {"params": {"normal_cos": p.normal_cos, "plane_eps": p.plane_eps, "max_holes": m},
                 "low_frame": [wl, hl], "hole_frame": [64, rows], "total": timed(frame),
                 "cone_steps": counted(lambda c: ctx.trace_mixed_device(p, *gb, w, h, eye, d, s, cone_steps=c))}
            frame()
            torch.cuda.synchronize()
            err = (d - full_d).abs()[valid]
            r["quality"] = {"rgb_max": float(err[:, :3].max().item()), "rgb_mean": float(err[:, :3].mean().item()),
                            "ao_max": float(err[:, 3].max().item()), "ao_mean": float(err[:, 3].mean().item()),
                            "full_rgb_mean": float(full_d[valid][:, :3].mean().item()),
                            "spec_bit_equal": bool(torch.equal(s.view(torch.int32), full_s.view(torch.int32)))}
            # the stages, each on buffers of its own
            lo = [torch.empty((hl, wl, 4), device=dev) for _ in range(4)]          # pos, nrm, alb, diffuse
            src = torch.empty((hl, wl), dtype=torch.int32, device=dev)
            hg = [torch.empty((rows, 64, 4), device=dev) for _ in range(4)]        # pos, nrm, alb, diffuse
            px = torch.empty((m,), dtype=torch.int32, device=dev)
            cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            stats = torch.zeros(4, dtype=torch.int32, device=dev)
            ho = ctx.mixed_holes(m, hg[0], hg[1], hg[2], px, cnt, stats)
            stage = {
                "pick": lambda: ctx.mixed_pick_device(*gb, w, h, eye, f, lo[0], lo[1], lo[2], src),
                "k4_low": lambda: ctx.trace_cones_device(DIFF, lo[0], lo[1], lo[2], wl, hl, eye, lo[3]),
                "upsample": lambda: ctx.mixed_upsample_device(*gb, w, h, f, lo[0], lo[1], src, lo[3], p, d, ho),
                "k4_holes": lambda: ctx.trace_cones_device(DIFF, hg[0], hg[1], hg[2], 64, rows, eye, hg[3]),
                "scatter": lambda: ctx.mixed_scatter_device(hg[3], ho, d),
                "k4_specular": lambda: ctx.trace_cones_device(SPEC, *gb, w, h, eye, None, s),
            }
            for fn in stage.values():       # in frame order: every stage reads what the one before wrote
                fn()
            torch.cuda.synchronize()
            st4 = [int(v) for v in stats.tolist()]
            r["stats"] = {"representatives": st4[0], "interpolated": st4[1], "holes": st4[2], "overflowed": st4[3],
                          "hole_share": round(st4[2] / max(nvalid, 1), 5)}
            r["stages"] = {k: timed(fn) for k, fn in stage.items()}
            r["stages_sum_ms"] = round(sum(v["ms"] for v in r["stages"].values()), 4)
            r["hole_steps"] = counted(lambda c: ctx.trace_cones_device(DIFF, hg[0], hg[1], hg[2], 64, rows, eye, hg[3],
                                                                      cone_steps=c))
            r["low_steps"] = counted(lambda c: ctx.trace_cones_device(DIFF, lo[0], lo[1], lo[2], wl, hl, eye, lo[3],
                                                                     cone_steps=c))
            # what the upsample stage has to move: pos read and plane written per pixel, the normal
            # of every valid pixel that is no representative, the hole records read and written,
            # the rest of the hole frame cleared, and the low frame once (pos, nrm, src, plane)
            listed = min(st4[2], m)
            by = w * h * 32 + (nvalid - st4[0]) * 16 + listed * (2 * 48 + 4) + (rows * 64 - listed) * 48 + wl * hl * 52
            ms = r["stages"]["upsample"]["ms"]
            r["upsample_bytes"] = by
            r["upsample_TBs"] = round(by / (ms * 1e-3) / 1e12, 3)
            r["upsample_fraction_of_copy_rate"] = round(by / (ms * 1e-3) / 1e12 / COPY_RATE_TBS, 3)
            # pick, K4 low, upsample + scan + list, K4 holes, scatter, K4 specular; the two small K4
            # launches of a settled frame each add the order kernel of their longest-first
            # dispatch (a kernel trace of the atrium frame shows these ten), and a K4 launch
            # whose workload settled on ray reordering adds its sort kernels
            r["kernel_launches"] = 8
            r["kernel_launches_with_dispatch_order"] = 10
            r["speedup_vs_full"] = round(row["full"]["call"]["ms"] / r["total"]["ms"], 3)
            row[f"mixed_f{f}"] = r
            del lo, src, hg, px
        out["scenes"][scene] = row
        ctx.close()
        del ctx, gb, full_d, full_s, d, s
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
