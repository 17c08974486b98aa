"""Light bounces (vct_inject_bounces) on one GPU, C3: the atrium at 256^3, 9 diffuse cones,
1920x1080 G_scene frame.  One JSON line, also written to profiles/bounce_bench.json:

  sources, cone steps per bounce, bytes of the source list;
  ms of the list build (once per voxelization) and of one bounce's gather / accumulate / K3
  (HIP events inside the library, vct_debug_bounce), per compiled K4 form and source order
  (region runs against occ_list order);
  the gather's cone-steps/s beside the same run's G_scene K4 rate;
  a relit frame (K2 + K3 + bounces + K4, queued back to back) with 0, 1 and 2 bounces;
  `stage_check`: level 0 after one bounce equals L0 + A * diffuse of the source G-buffer
  traced by a specular=False context (the GPU tests' stage check, at full scale).
"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd")]


def source_gbuffer(n, g0, E, ao, nm, width=1024):
    """The sources as a [rows][width] G-buffer (vct_spec.h "light bounces"), padded with
    background pixels; -> (pos4, nrm4, alb4), (z, y, x)"""
    import numpy as np
    z, y, x = np.nonzero((ao[..., 3] != 0) & np.any(nm[..., :3] != 0, axis=-1))
    S = x.size
    rows = max(1, -(-S // width))
    pos = np.zeros((rows * width, 4), np.float32)
    nrm = np.zeros_like(pos)
    alb = np.zeros_like(pos)
    hh = np.float32(E) / np.float32(n)
    g0 = np.asarray(g0, np.float32)
    for c, idx in enumerate((x, y, z)):
        pos[:S, c] = g0[c] + (idx.astype(np.float32) + np.float32(0.5)) * hh
    pos[:S, 3] = 1.0
    nrm[:S, :3] = nm[z, y, x, :3]
    alb[:S, :3] = ao[z, y, x, :3]
    shape = (rows, width, 4)
    return (pos.reshape(shape), nrm.reshape(shape), alb.reshape(shape)), (z, y, x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--scene", default="atrium")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bounce_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from vct import Context, scenes
    from vct.camera import Camera
    n, w, h = a.n, a.width, a.height
    g0, E = scenes.grid_for_unit_box(n)
    arrays = scenes.SCENES[a.scene]().arrays()
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    ctx = Context(n, g0, E, aniso=True, n_diffuse=9, specular=True)
    ctx.set_stream(st.cuda_stream)
    dbg = ctx.lib.vct_debug_bounce
    dbg.restype = C.c_int
    dbg.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]

    def relight():
        ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
        ctx.build_mips()

    def times():
        ms = (C.c_float * 4)()
        dbg(ctx.h, -1, -1, 1, ms)
        return [float(x) for x in ms]

    ctx.voxelize(*arrays)
    relight()
    relight()                                           # the next builds are relight builds
    ao, nm = ctx.download_voxels()
    L0 = ctx.download_level(0)
    gbuf, (z, y, x) = source_gbuffer(n, g0, E, ao, nm)
    sources = ctx.bounce_sources()
    assert sources == x.size, (sources, x.size)

    # the gather as a plain trace of the source G-buffer: cone steps per bounce, stage check
    plain = Context(n, g0, E, aniso=True, n_diffuse=9, specular=False)
    plain.voxelize(*arrays)
    plain.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    plain.build_mips()
    out = plain.trace(*gbuf, (0.0, 0.0, 0.0), want_steps=False)
    steps_per_bounce = out["cone_steps"]
    want = L0.copy()
    want[z, y, x, :3] = L0[z, y, x, :3] + ao[z, y, x, :3] * out["diffuse"].reshape(-1, 4)[:x.size, :3]
    ctx.inject_bounces(1)
    L1 = ctx.download_level(0)
    stage_ok = bool(np.array_equal(L1.view(np.uint32), want.view(np.uint32)))
    lit = int((np.any(L1[z, y, x, :3] != 0, axis=-1) & ~np.any(L0[z, y, x, :3] != 0, axis=-1)).sum())
    plain.close()
    del out, want, gbuf

    # stage times per (source order, K4 form); every combination must give the same level 0
    stages = {}
    for order in (0, 1):                                # the library's defaults (regions, union) last
        for form in (1, 0):
            dbg(ctx.h, form, order, 1, None)
            if ctx.bounce_sources() != sources:         # rebuilt when the order changed
                raise SystemExit("source count changed with the order")
            best = None
            for _ in range(a.reps):
                relight()
                ctx.inject_bounces(1)
                t = times()
                best = t if best is None else [min(p, q) for p, q in zip(best, t)]
            same = bool(np.array_equal(ctx.download_level(0).view(np.uint32), L1.view(np.uint32)))
            stages[f"{'regions' if order else 'occ_list'}/{'occupancy' if form else 'union'}"] = {
                "list_build_ms": round(best[0], 4), "gather_ms": round(best[1], 4), "accumulate_ms": round(best[2], 4),
                "k3_ms": round(best[3], 4), "gather_gcone_steps_s": round(steps_per_bounce / best[1] / 1e6, 3),
                "equals_first": same}
    dbg(ctx.h, -1, -1, 0, None)                         # untimed from here on

    # the frame: G_scene at w x h, K4 settled on it
    cam = Camera()
    eye = [float(v) for v in cam.position]
    gb = tuple(torch.empty((h, w, 4), dtype=torch.float32, device=dev) for _ in range(3))
    relight()
    ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
    d, sp = torch.empty((h, w, 4), device=dev), torch.empty((h, w, 4), device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.trace_device(*gb, w, h, eye, d, sp, cone_steps=cnt)
    torch.cuda.synchronize()
    frame_steps = int(cnt.item())
    last, run = None, 0
    for _ in range(256):
        ctx.trace_device(*gb, w, h, eye, d, sp)
        torch.cuda.synchronize()
        f = ctx.trace_form
        run = run + 1 if (f >= 0 and f == last) else 0
        last = f
        if run >= 24:
            break

    def queued(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    k4_ms = min(queued(lambda: ctx.trace_device(*gb, w, h, eye, d, sp)) for _ in range(3))
    form_before = ctx.trace_form
    frames = {}
    for nb in (0, 1, 2):
        def frame():
            relight()
            if nb:
                ctx.inject_bounces(nb)
            ctx.trace_device(*gb, w, h, eye, d, sp)
        frame()
        frames[str(nb)] = round(min(queued(frame) for _ in range(3)), 4)
    res = {
        "tool": "bounce_bench", "scene": a.scene, "n": n, "cones": 9, "frame": [w, h], "reps": a.reps,
        "sources": sources, "cone_steps_per_bounce": steps_per_bounce,
        "source_list_bytes": sources * 20 + int(-(-sources // 4096)) * 4096 * 64,
        "newly_lit_voxels": lit, "stage_check": stage_ok, "stages": stages,
        "k4_scene_ms": round(k4_ms, 4), "k4_scene_cone_steps": frame_steps,
        "k4_scene_gcone_steps_s": round(frame_steps / k4_ms / 1e6, 3),
        "trace_form_before_after": [form_before, ctx.trace_form],
        "frame_relight_ms": frames,
    }
    line = json.dumps(res)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    ctx.close()
    if not stage_ok or not all(s["equals_first"] for s in stages.values()):
        raise SystemExit("bounce result differs from the stage composition")


if __name__ == "__main__":
    main()
