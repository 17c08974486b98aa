"""Temporal accumulation (include/vct_temporal.h) on one GPU: the atrium at 256^3 (or --scene /
--n), the bench's 1080p G_scene frame, 9 diffuse cones + specular.  One JSON line, also written
to profiles/temporal_bench.json.  tools/mixed_bench.py's protocol: device events on the
context's stream, warmed; every figure is the median of `--blocks` blocks of back-to-back calls,
each block grown until its calls fill `--window` seconds, with the fastest and slowest block
beside it; every K4 workload is settled (the tuner's choice made) before it is timed.

  call:      vct_temporal_accumulate_device for n_planes 1, 2 and 4 on a same-camera and a
             moved-camera frame (stats off; n_planes 1 with stats too), the bytes it has to move
             and its rate against the 6.29 TB/s float4 copy rate, and the mixed trace's upsample
             stage (kmix_up + scan + list, f = 2) timed in the same session
  frame:     vct_trace_device alone (the yardstick) and followed by the call
  sequence:  --frames frames with tools/dynamic_bench.py's box moving a third of a voxel per
             frame under a fixed camera.  Stability: the mean |delta| between consecutive
             frames' diffuse rgb over the pixels whose G-buffer record did not change, for the
             full trace and the mixed trace at f = 2, each raw and accumulated at the default
             max_len (no motion vectors)
  response:  frames the accumulated plane needs after a light change (static scene, fixed
             camera) until its mean |acc - new| falls to 10 % of mean |old - new|
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd"), os.path.join(REPO, "tools")]

COPY_RATE_TBS = 6.29      # measured float4 copy rate of the device (bytes read + written per second)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--scene", default="atrium")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "temporal_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import vct
    from dynamic_bench import tessellated_box
    from vct import Context, scenes
    from vct.camera import Camera
    from vct.temporal import History
    n, w, h = a.n, a.width, a.height
    g0, E = scenes.grid_for_unit_box(n)
    st = torch.cuda.current_stream()
    dev = torch.device("cuda")
    sun = vct.directional_light(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    cam = Camera()
    moved = Camera(position=(0.05, 0.02, 2.95), yaw=-91.0, pitch=0.5)     # a frame's worth of walking and turning
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

    def settle(fn, frames=96):              # the tuner's timed choice of every K4 workload fn launches
        for _ in range(frames):
            fn()
            torch.cuda.synchronize()

    plane = lambda: torch.empty((h, w, 4), device=dev)
    ctx = Context(n, g0, E, aniso=True, n_diffuse=9, specular=True)
    ctx.set_stream(st.cuda_stream)
    static = scenes.SCENES[a.scene]().arrays()
    ctx.voxelize(*static)
    ctx.inject_lights([sun])
    ctx.build_mips()
    p = ctx.temporal_params()
    out = {"tool": "temporal_bench", "n": n, "scene": a.scene, "cones": "9 + specular", "width": w, "height": h,
           "device": torch.cuda.get_device_name(0), "blocks": a.blocks, "copy_rate_TBs": COPY_RATE_TBS,
           "params": {"normal_cos": p.normal_cos, "plane_eps": p.plane_eps, "max_len": p.max_len}}

    # ---- the call ------------------------------------------------------------------------------
    gb_a, gb_b = tuple(plane() for _ in range(3)), tuple(plane() for _ in range(3))
    ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb_a)
    ctx.gbuffer_raster_device(moved, w, h, scenes.ROUGHNESS, *gb_b)
    d_a, s_a, d_b, s_b = (plane() for _ in range(4))
    settle(lambda: ctx.trace_device(*gb_a, w, h, eye, d_a, s_a))
    ctx.trace_device(*gb_b, w, h, [float(x) for x in moved.position], d_b, s_b)
    torch.cuda.synchronize()
    nvalid = {"same": int((gb_a[0][..., 3] != 0).sum().item()), "moved": int((gb_b[0][..., 3] != 0).sum().item())}
    out["valid_pixels"] = nvalid
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    calls = {}
    for npl in (1, 2, 4):
        cur_a, cur_b = [d_a, s_a, d_a, s_a][:npl], [d_b, s_b, d_b, s_b][:npl]
        hist, outp = [plane() for _ in range(npl)], [plane() for _ in range(npl)]
        hlen, olen = (torch.empty((h, w), dtype=torch.int32, device=dev) for _ in range(2))
        ctx.temporal_accumulate_device(p, gb_a[0], gb_a[1], w, h, cur_a, hist, hlen)                # the history: a reset frame
        for tag, gb, cur in (("same", gb_a, cur_a), ("moved", gb_b, cur_b)):
            kw = dict(prev_cam=cam, prev_pos4=gb_a[0], prev_nrm4=gb_a[1], hist=hist, hist_len=hlen)
            call = lambda s=None: ctx.temporal_accumulate_device(p, gb[0], gb[1], w, h, cur, outp, olen, stats=s, **kw)
            call(stats)
            torch.cuda.synchronize()
            st4 = [int(v) for v in stats.tolist()]
            # pos, nrm, cur read and out, out_len written per valid pixel; a coherent frame reads
            # each previous pixel's pos, nrm, hist and length once; background: pos read, +0 written
            nv, nb = nvalid[tag], w * h - nvalid[tag]
            by = nv * (32 + 32 * npl + 4) + (st4[0] - st4[2]) * (36 + 16 * npl) + nb * (16 + 16 * npl + 4)
            r = {"call": timed(call), "stats": dict(zip(("valid", "reused", "reset_offscreen", "reset_rejected"), st4)),
                 "bytes": by}
            r["TBs"] = round(by / (r["call"]["ms"] * 1e-3) / 1e12, 3)
            r["fraction_of_copy_rate"] = round(r["TBs"] / COPY_RATE_TBS, 3)
            if npl == 1:
                r["call_with_stats"] = timed(lambda: call(stats))
            calls[f"{tag}_{npl}"] = r
        del hist, outp, hlen, olen
    out["call"] = calls

    # kmix_up's stage (upsample + scan + list at f = 2), as tools/mixed_bench.py times it
    f = 2
    mp = ctx.mixed_params(f)
    wl, hl = (w + f - 1) // f, (h + f - 1) // f
    m = ctx.mixed_max_holes(w, h)
    rows = (m + 63) // 64
    lo = [torch.empty((hl, wl, 4), device=dev) for _ in range(4)]
    src = torch.empty((hl, wl), dtype=torch.int32, device=dev)
    hg = [torch.empty((rows, 64, 4), device=dev) for _ in range(3)]
    px, cnt, mst = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (m, 1, 4))
    ho = ctx.mixed_holes(m, hg[0], hg[1], hg[2], px, cnt, mst)
    d_m, s_m = plane(), plane()
    ctx.mixed_pick_device(*gb_a, w, h, eye, f, lo[0], lo[1], lo[2], src)
    ctx.trace_cones_device(1, lo[0], lo[1], lo[2], wl, hl, eye, lo[3])
    up = lambda: ctx.mixed_upsample_device(*gb_a, w, h, f, lo[0], lo[1], src, lo[3], mp, d_m, ho)
    up()
    torch.cuda.synchronize()
    ms4 = [int(v) for v in mst.tolist()]
    listed = min(ms4[2], m)
    up_bytes = w * h * 32 + (nvalid["same"] - ms4[0]) * 16 + listed * (2 * 48 + 4) + (rows * 64 - listed) * 48 + wl * hl * 52
    up_t = timed(up)
    out["mixed_upsample_stage"] = {"call": up_t, "bytes": up_bytes, "TBs": round(up_bytes / (up_t["ms"] * 1e-3) / 1e12, 3),
                                   "fraction_of_copy_rate": round(up_bytes / (up_t["ms"] * 1e-3) / 1e12 / COPY_RATE_TBS, 3)}
    del lo, src, hg, px

    # ---- the frame -----------------------------------------------------------------------------
    hist1 = History(ctx, w, h, 1, p)

    def frame_acc():
        ctx.trace_device(*gb_a, w, h, eye, d_a, s_a)
        hist1.accumulate(gb_a, cam, [d_a])

    trace = lambda: ctx.trace_device(*gb_a, w, h, eye, d_a, s_a)
    settle(trace, 16)
    out["frame"] = {"trace": timed(trace), "trace_form": ctx.trace_form}
    out["frame"]["trace_and_accumulate"] = timed(frame_acc)       # History: the call and two plane copies
    out["frame"]["trace_again"] = timed(trace)
    out["frame"]["accumulate_over_trace"] = round(out["frame"]["trace_and_accumulate"]["ms"] / out["frame"]["trace"]["ms"], 4)

    # ---- the sequence --------------------------------------------------------------------------
    vox = float(E) / n
    to_dev = lambda mesh: (torch.from_numpy(np.ascontiguousarray(mesh[0])).to(dev), torch.from_numpy(mesh[1].view(np.int32)).to(dev),
                           torch.from_numpy(mesh[2].view(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(mesh[3])).to(dev))
    path = [to_dev(tessellated_box((0.25 + k * vox / 3.0, -0.55, 0.0), 0.12, 13)) for k in range(a.frames)]
    kinds = ("full", "mixed")
    hists = {k: History(ctx, w, h, 1, p, stats=True) for k in kinds}
    gb, prev_gb = tuple(plane() for _ in range(3)), tuple(plane() for _ in range(3))
    raw = {k: plane() for k in kinds}
    spec = plane()
    last = {}
    series = {f"{k}_{v}": [] for k in kinds for v in ("raw", "accumulated")}
    unchanged, reuse = [], []
    for k_frame, layer in enumerate(path):
        ctx.voxelize_dynamic_device(*layer)
        ctx.inject_lights([sun])
        ctx.build_mips()
        ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
        ctx.trace_device(*gb, w, h, eye, raw["full"], spec)
        ctx.trace_mixed_device(mp, *gb, w, h, eye, raw["mixed"], spec)
        acc = {k: hists[k].accumulate(gb, cam, [raw[k]])[0] for k in kinds}
        torch.cuda.synchronize()
        if k_frame:
            same = (gb[0][..., 3] != 0)
            for x, y in zip(gb, prev_gb):
                same &= (x.view(torch.int32) == y.view(torch.int32)).all(dim=-1)
            unchanged.append(int(same.sum().item()))
            st4 = [int(v) for v in hists["full"].stats.tolist()]
            reuse.append(round(st4[1] / max(st4[0], 1), 5))
            for k in kinds:
                for v, t in (("raw", raw[k]), ("accumulated", acc[k])):
                    series[f"{k}_{v}"].append(float((t[..., :3] - last[f"{k}_{v}"][..., :3]).abs()[same].mean().item()))
        for k in kinds:
            last[f"{k}_raw"], last[f"{k}_accumulated"] = raw[k].clone(), acc[k].clone()
        for x, y in zip(prev_gb, gb):
            x.copy_(y)
    mean_rgb = float(raw["full"][..., :3][gb[0][..., 3] != 0].mean().item())
    half = len(series["full_raw"]) // 2
    out["sequence"] = {"frames": a.frames, "step_voxels": 1.0 / 3.0, "unchanged_pixels": [min(unchanged), max(unchanged)],
                       "reused_share": [min(reuse), max(reuse)], "full_rgb_mean": mean_rgb,
                       "mean_abs_delta": {k: float(np.mean(v)) for k, v in series.items()},
                       "mean_abs_delta_second_half": {k: float(np.mean(v[half:])) for k, v in series.items()},
                       "per_frame": {k: [round(x, 8) for x in v] for k, v in series.items()}}
    for k in kinds:
        out["sequence"][f"{k}_accumulated_over_raw"] = round(out["sequence"]["mean_abs_delta"][f"{k}_accumulated"] /
                                                             max(out["sequence"]["mean_abs_delta"][f"{k}_raw"], 1e-30), 4)

    # ---- the response to a light change ------------------------------------------------------------
    ctx.voxelize_dynamic_device(*to_dev(tessellated_box((0.25, -0.55, 0.0), 0.12, 13)))
    other = vct.directional_light((-0.4, 0.8, 0.45), (1.0, 0.85, 0.6))
    ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
    valid = gb[0][..., 3] != 0
    hr = History(ctx, w, h, 1, p)

    def lit_frame(light):
        ctx.inject_lights([light])
        ctx.build_mips()
        ctx.trace_device(*gb, w, h, eye, raw["full"], spec)
        return hr.accumulate(gb, cam, [raw["full"]])[0]

    for _ in range(2 * p.max_len):
        old = lit_frame(sun).clone()
    gap = None
    resp = []
    for k_frame in range(1, 8 * p.max_len + 1):
        acc = lit_frame(other)
        torch.cuda.synchronize()
        if gap is None:
            gap = float((raw["full"][..., :3] - old[..., :3]).abs()[valid].mean().item())
        resp.append(float((acc[..., :3] - raw["full"][..., :3]).abs()[valid].mean().item()) / max(gap, 1e-30))
        if resp[-1] <= 0.1:
            break
    out["response"] = {"max_len": p.max_len, "frames_to_10_percent": k_frame if resp[-1] <= 0.1 else None,
                       "old_to_new_mean_abs_rgb": gap, "remaining_share_per_frame": [round(x, 5) for x in resp],
                       "expected": "the smallest j with (1 - 1 / max_len)^j <= 0.1 once the length has saturated"}
    ctx.close()
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
