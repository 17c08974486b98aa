"""Object motion (include/vct_motion.h) on one GPU: the courtyard and the atrium at 256^3 (or
--scenes / --n) with tools/objects_bench.py's 32 boxes, the bench's 1080p frame from the shaded
G-buffer pass.  One JSON line, also written to profiles/motion_bench.json.  tools/temporal_bench.py's
protocol: device events on the context's stream, warmed; every figure is the median of `--blocks`
blocks of back-to-back calls, each block grown until its calls fill `--window` seconds, with the
fastest and slowest block beside it.

  copy:      a float4 plane copied to another (bytes read + written per second), in this session:
             the rate every other figure is a fraction of (temporal_bench's constant is 6.29 TB/s)
  call:      vct_objects_motion_device with nothing moved since the snapshot, 4 of 32 objects
             moved and all 32 moved, with and without prev_nrm4 (stats off), against its
             compulsory traffic: pos4, tri_id and bary2 read and motion4 written, 44 bytes a
             pixel; nrm4 read and prev_nrm4 written on top, 76
  sequence:  temporal_bench's moving box (a third of a voxel per frame under a fixed camera) as
             one object of a set: the share of the box's pixels that keep their history, with
             and without the motion planes.  The share depends on the G-buffers, the planes and
             the history lengths only, so the frames are not traced.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd"), os.path.join(REPO, "tools")]

COPY_RATE_TBS = 6.29      # tools/temporal_bench.py's constant, for comparison with its fractions


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--scenes", default="courtyard,atrium")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--k", type=int, default=13, help="quads per box edge (12 k^2 triangles)")
    ap.add_argument("--objects", type=int, default=32)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "motion_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from dynamic_bench import tessellated_box
    from vct import Context, objects, scenes, shading
    from vct.camera import Camera
    from vct.motion import MotionTracker
    from vct.temporal import History
    n, w, h, count = a.n, a.width, a.height, a.objects
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

    plane = lambda: torch.empty((h, w, 4), device=dev)
    px = w * h
    out = {"tool": "motion_bench", "n": n, "width": w, "height": h, "objects": count, "device": torch.cuda.get_device_name(0),
           "blocks": a.blocks, "temporal_bench_copy_rate_TBs": COPY_RATE_TBS, "bytes_per_pixel": {"motion": 44, "with_normals": 76}}

    # ---- the copy rate, in this session -------------------------------------------------------------
    src, dst = plane().fill_(1.0), plane()
    cp = timed(lambda: dst.copy_(src))
    rate = 2 * px * 16 / (cp["ms"] * 1e-3) / 1e12
    out["copy"] = {"call": cp, "bytes": 2 * px * 16, "TBs": round(rate, 3)}
    del src, dst

    def planes_of(ctx):
        gb = {k: plane() for k in ("pos", "nrm", "alb", "ks")}
        gb["tri_id"] = torch.empty((h, w), dtype=torch.int32, device=dev)
        gb["bary"] = torch.empty((h, w, 2), device=dev)
        return gb

    def shaded(ctx, gb):
        ctx.gbuffer_shaded_device(cam, w, h, scenes.ROUGHNESS, gb["pos"], gb["nrm"], gb["alb"], gb["ks"], tri_id=gb["tri_id"],
                                  bary2=gb["bary"])

    # ---- the call -----------------------------------------------------------------------------------
    bv, bi, bm, bk = tessellated_box((0.0, 0.0, 0.0), 0.08, a.k)
    homes = [(-0.6 + 0.4 * (k % 4), -0.55 + 0.4 * ((k // 4) % 2), -0.6 + 0.4 * (k // 8)) for k in range(count)]

    def pose_of(k, step):                   # tools/objects_bench.py's loop around each home
        ang = 2.0 * np.pi * (step % 8) / 8.0
        hm = homes[k]
        return objects.pose((hm[0] + 0.05 * np.cos(ang), hm[1] + 0.05 * np.sin(ang), hm[2] + 0.05 * np.sin(2 * ang)))

    def dev_poses(moved):                   # every object at step 0, the `moved` ones a step earlier
        rec = objects.poses([pose_of(k, 7 if k in moved else 0) for k in range(count)])
        return torch.from_numpy(rec.view(np.uint8).reshape(count, 80).copy()).to(dev)

    every = list(range(count))
    subsets = {"moved_0": [], "moved_4": [1, count // 4, count // 2, count - 2], f"moved_{count}": every}
    out["scenes"] = {}
    for name in a.scenes.split(","):
        sv, si, sm, sk = scenes.SCENES[name]().arrays()
        ctx = Context(n, g0, E)
        ctx.set_stream(st.cuda_stream)
        ctx.voxelize(sv, si, sm, sk)
        shading.set_flat(ctx, sv, si, scenes.ROUGHNESS)
        ctx.objects_define([(bv, bi, bm)] * count, bk)
        ctx.objects_update_device(every, dev_poses([]))
        gb = planes_of(ctx)
        shaded(ctx, gb)
        motion4, pnrm4 = plane(), plane()
        stats = torch.zeros(4, dtype=torch.int32, device=dev)
        row = {"static_triangles": int(si.size // 3), "set_triangles": int(count * bi.size // 3)}
        for tag, moved in subsets.items():
            snap = dev_poses(moved)
            call = lambda nrm, s=None: ctx.objects_motion_device(w, h, gb["pos"], gb["tri_id"], gb["bary"], snap, motion4,
                                                                 nrm4=gb["nrm"] if nrm else None,
                                                                 prev_nrm4=pnrm4 if nrm else None, stats=s)
            call(True, stats)
            torch.cuda.synchronize()
            r = {"stats": dict(zip(("valid", "static_or_unmoved", "moved", "appeared"), (int(v) for v in stats.tolist())))}
            for key, nrm, per in (("motion", False, 44), ("with_normals", True, 76)):
                t = timed(lambda: call(nrm))
                tbs = px * per / (t["ms"] * 1e-3) / 1e12
                r[key] = {"call": t, "bytes": px * per, "TBs": round(tbs, 3), "fraction_of_copy_rate": round(tbs / rate, 3),
                          "fraction_of_temporal_bench_rate": round(tbs / COPY_RATE_TBS, 3),
                          "multiple_of_compulsory_time": round(rate / tbs, 3)}
            r["with_normals_and_stats"] = timed(lambda: call(True, stats))
            row[tag] = r
        out["scenes"][name] = row
        ctx.close()
        del gb, motion4, pnrm4

    # ---- the sequence ---------------------------------------------------------------------------------
    name = a.scenes.split(",")[-1]
    sv, si, sm, sk = scenes.SCENES[name]().arrays()
    n_static = int(si.size // 3)
    ctx = Context(n, g0, E)
    ctx.set_stream(st.cuda_stream)
    ctx.voxelize(sv, si, sm, sk)
    shading.set_flat(ctx, sv, si, scenes.ROUGHNESS)
    v0, i0, m0, k0 = tessellated_box((0.0, 0.0, 0.0), 0.12, a.k)
    ctx.objects_define([(v0, i0, m0)], k0)
    vox = float(E) / n
    hists = {k: History(ctx, w, h, 1, stats=True) for k in ("plain", "tracked")}
    tracker = MotionTracker(ctx, 1, w, h, stats=True)
    gb = planes_of(ctx)
    cur = plane().fill_(0.5)
    share = {"plain": [], "tracked": []}
    moved_px = []
    for f in range(a.frames):
        ctx.objects_update([0], objects.poses([objects.pose((0.25 + f * vox / 3.0, -0.55, 0.0))]))
        shaded(ctx, gb)
        motion4, pnrm4 = tracker.planes(gb["pos"], gb["nrm"], gb["tri_id"], gb["bary"])
        hists["plain"].accumulate((gb["pos"], gb["nrm"]), cam, [cur])
        hists["tracked"].accumulate((gb["pos"], gb["nrm"]), cam, [cur], motion=motion4, test_normals=pnrm4)
        tracker.end_frame()
        torch.cuda.synchronize()
        on = (gb["pos"][..., 3] != 0) & (gb["tri_id"] >= n_static)
        if f:
            for k in share:
                share[k].append(round(float((hists[k].lengths[on] >= 2).sum().item()) / max(int(on.sum().item()), 1), 5))
            moved_px.append(int(tracker.stats[2].item()))
    out["sequence"] = {"scene": name, "frames": a.frames, "step_voxels": 1.0 / 3.0, "object_pixels_moved": [min(moved_px), max(moved_px)],
                       "reused_share_of_object_pixels": {k: {"min": min(v), "max": max(v), "mean": round(float(np.mean(v)), 5)}
                                                         for k, v in share.items()}}
    ctx.close()
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
