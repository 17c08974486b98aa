"""Emissive surfaces (include/vct_emission.h) on one GPU: the atrium at 256^3 with the eight
gallery lamps of tools/lights_bench.py turned into small emissive quads on the underside of
the gallery slabs, 9 diffuse cones, a 1920x1080 G_scene frame.  One JSON line, also written to
profiles/emission_bench.json.  Device events on the context's stream, warmed; a queued line is
`--blocks` blocks of `--reps` back-to-back calls, reported as the median block's ms per call
with the fastest and slowest block beside it.

  vct_voxelize_emission_device over the whole mesh (Ke per material: only the lamp material
    emits, so only its 16 triangles have candidates) and over the 16 lamp triangles alone;
    the call waits for the stream once, so it is timed on the host clock around a
    synchronised call (median of --blocks calls);
  vct_inject_emission, queued after a vct_inject_lights (the pair minus the inject alone);
  vct_composite_emissive_device beside vct_composite_shadowed_device on the same frame and
    vis planes, and with vis = NULL beside vct_composite_lights_device;
  a relit frame (inject_lights + build_mips + K4, queued back to back) with and without
    vct_inject_emission;
  `stage_check`: level 0 with emission == level 0 without + 1.0 * E, bit for bit.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd")]

LAMP_KD = (0.78, 0.78, 0.78)
LAMP_KE = (10.0, 8.0, 5.0)
LAMP_XZ = [(x, z) for x in (-0.78, 0.78) for z in (-0.7, -0.25, 0.2, 0.65)]   # lights_bench.py's gallery lamps
LAMP_HALF = 0.06                                                              # 12 cm panels


def lamp_atrium():
    """scenes.atrium() plus one emissive panel per gallery lamp, on the slabs' underside (y = 0.05).
    -> (scene, ke4, the lamp material)"""
    import numpy as np
    from vct import scenes
    s = scenes.atrium()
    lamp = s.material(LAMP_KD)
    for x, z in LAMP_XZ:
        s.rect_y(0.05, x - LAMP_HALF, x + LAMP_HALF, z - LAMP_HALF, z + LAMP_HALF, -1, lamp)
    ke = np.zeros((len(s.kd), 4), np.float32)
    ke[lamp, :3] = LAMP_KE
    return s, ke, lamp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "emission_bench.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import vct
    from vct import Context, scenes
    from vct.camera import Camera
    n, w, h = a.n, a.width, a.height
    g0, E = scenes.grid_for_unit_box(n)
    s, ke, lamp = lamp_atrium()
    v, i, m, k = s.arrays()
    dev = torch.device("cuda")
    st = torch.cuda.current_stream()
    ctx = Context(n, g0, E, aniso=True, n_diffuse=9, specular=True)
    ctx.set_stream(st.cuda_stream)
    ctx.voxelize(v, i, m, k)
    sun = vct.directional_light(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    court = vct.point_light((0.0, -0.3, 0.0), (6.0, 6.0, 5.0), 4.0)
    lights = [sun, court]

    def summary(ms, launches):
        return {"ms": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5),
                "launches": launches}

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def timed(fns):
        """Alternate the callables block by block; -> one summary per callable."""
        for fn in fns:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(a.blocks):
            for j, fn in enumerate(fns):
                ms[j].append(block(fn))
        return [summary(x, a.blocks * a.reps) for x in ms]

    def host_timed(fn):
        """A call that waits for the stream itself: host clock around a synchronised call."""
        fn()
        ms = []
        for _ in range(a.blocks):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return summary(ms, a.blocks)

    out = {"tool": "emission_bench", "scene": "atrium + 8 lamp panels", "n": n, "cones": 9, "frame": [w, h],
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "blocks": a.blocks,
           "triangles": int(m.size), "lamp_triangles": int((m == lamp).sum())}

    # ---- the build -------------------------------------------------------------------------
    t = lambda arr, dt: torch.from_numpy(np.ascontiguousarray(arr).view(dt)).to(dev)
    dv, di, dm, dke = t(v, np.float32), t(i, np.int32), t(m, np.int32), t(ke, np.float32)
    sel = np.flatnonzero(m == lamp)
    di_l, dm_l = t(i.reshape(-1, 3)[sel].reshape(-1), np.int32), t(m[sel], np.int32)
    out["voxelize_emission_device_whole_mesh"] = host_timed(lambda: ctx.voxelize_emission_device(dv, di, dm, dke))
    whole = ctx.download_emission()
    out["voxelize_emission_device_lamp_triangles"] = host_timed(lambda: ctx.voxelize_emission_device(dv, di_l, dm_l, dke))
    same_grid = bool(np.array_equal(ctx.download_emission().view(np.uint32), whole.view(np.uint32)))
    dkd = t(k, np.float32)
    out["voxelize_device_for_scale"] = host_timed(lambda: ctx.voxelize_device(dv, di, dm, dkd))
    ctx.voxelize_emission_device(dv, di, dm, dke)          # (the voxelization emptied the grid)
    n_em = ctx.emission_voxels()
    occupied = int((ctx.download_voxels()[0][..., 3] != 0).sum())
    out.update(occupied_voxels=occupied, emissive_voxels=n_em,
               emission_bytes=int(occupied * 44 + (n ** 3 // 64) * 12), lamp_subset_gives_the_same_grid=same_grid)

    # ---- level 0 -----------------------------------------------------------------------------
    inject = lambda: ctx.inject_lights(lights)

    def inject_emit():
        ctx.inject_lights(lights)
        ctx.inject_emission(1.0)
    alone, pair = timed([inject, inject_emit])
    out["inject_lights"] = alone
    out["inject_lights_then_inject_emission"] = pair
    out["inject_emission_ms"] = round(pair["ms"] - alone["ms"], 5)
    inject()
    L0 = ctx.download_level(0)
    inject_emit()
    L1 = ctx.download_level(0)
    em = whole[..., 3] != 0
    want = L0.copy()
    want[em, :3] = L0[em, :3] + np.float32(1.0) * whole[em, :3]
    stage_ok = bool(np.array_equal(L1.view(np.uint32), want.view(np.uint32))) and int(em.sum()) == n_em
    out["stage_check"] = stage_ok
    del L0, L1, want

    # ---- the frame ---------------------------------------------------------------------------
    cam = Camera()
    eye = [float(x) for x in cam.position]
    gb = tuple(torch.empty((h, w, 4), dtype=torch.float32, device=dev) for _ in range(3))
    ctx.build_mips()
    ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
    d, sp, lin = (torch.empty((h, w, 4), device=dev) for _ in range(3))
    px = torch.zeros((h, w), dtype=torch.int32, device=dev)
    vis = torch.empty((len(lights), h, w), device=dev)
    ctx.trace_device(*gb, w, h, eye, d, sp)
    ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, [0.05, 0.1], vis)
    torch.cuda.synchronize()
    pos = gb[0].cpu().numpy()
    q = (pos[..., :3] - np.asarray(g0, np.float32)) * (np.float32(n) / np.float32(E))
    inside = np.all((q >= 0) & (q < n), axis=-1) & (pos[..., 3] != 0)
    c = np.where(inside[..., None], np.floor(q), 0).astype(np.int64)
    out["pixels_on_emissive_voxels"] = int((inside & em[c[..., 2], c[..., 1], c[..., 0]]).sum())
    del pos, q, c
    shadowed, emissive, walked, emissive_walked = timed([
        lambda: ctx.composite_shadowed_device(*gb, d, sp, w, h, lights, vis, out_linear4=lin, out_rgba8=px),
        lambda: ctx.composite_emissive_device(*gb, d, sp, w, h, lights, vis, 1.0, out_linear4=lin, out_rgba8=px),
        lambda: ctx.composite_lights_device(*gb, d, sp, w, h, lights, out_linear4=lin, out_rgba8=px),
        lambda: ctx.composite_emissive_device(*gb, d, sp, w, h, lights, None, 1.0, out_linear4=lin, out_rgba8=px)])
    out["composite_shadowed_device"] = shadowed
    out["composite_emissive_device"] = emissive
    out["composite_lights_device"] = walked
    out["composite_emissive_device_vis_null"] = emissive_walked

    # a relit frame, K4 settled on the frame first
    last, run = None, 0
    for _ in range(256):
        ctx.trace_device(*gb, w, h, eye, d, sp)
        torch.cuda.synchronize()
        f = ctx.trace_form
        run = run + 1 if (f >= 0 and f == last) else 0
        last = f
        if run >= 24:
            break

    def frame(emit):
        def fn():
            ctx.inject_lights(lights)
            if emit:
                ctx.inject_emission(1.0)
            ctx.build_mips()
            ctx.trace_device(*gb, w, h, eye, d, sp)
        return fn
    dark, lit = timed([frame(False), frame(True)])
    out["frame_relight"] = dark
    out["frame_relight_with_emission"] = lit
    out["trace_form"] = ctx.trace_form

    line = json.dumps(out)
    print(line, flush=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    ctx.close()
    if not stage_ok or not same_grid or n_em == 0:
        raise SystemExit("emission result differs from the stage composition")


if __name__ == "__main__":
    main()
