"""The dynamic layer (include/vct_dynamic.h) on one GPU: the courtyard and the atrium at 256^3
(or --scenes / --n) with a moving object of about 2 K triangles, a tessellated box that steps
round a loop of 8 positions.  One JSON line, also written to profiles/dynamic_bench.json.
Device events on the context's stream, warmed; every figure is the median of `--blocks` blocks
of back-to-back calls, each block grown until its calls fill `--window` seconds (`window_s` is
the shortest block kept), with the fastest and slowest block beside it.  The calls wait for
the stream themselves (the error word), so a block's time is what the host sees per call.

Per scene:
  layer_device / layer_host:  ms per vct_voxelize_dynamic_device / vct_voxelize_dynamic as the
                              object steps along the path
  full_device / full_host:    ms per vct_voxelize_device / vct_voxelize of the concatenated mesh
                              at the same positions: the only way to move the object without
                              the layer
  static_device:              ms per vct_voxelize_device of the static scene alone
  frame_layer:                a frame with motion: layer + inject + full K3 + K4
  frame_full:                 the same frame with the concatenated mesh voxelized instead
  frame_relight:              the relit frame (inject + K3's relight build + K4), nothing moves
  layer_voxels:               voxels the layer hits at each position (vct_dynamic_voxels)
  check:                      after all of it, K1's sums and counts equal a fresh context's
                              vct_voxelize of the concatenated mesh at the last position
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd")]


def tessellated_box(centre, half, k, kd=(0.8, 0.3, 0.2)):
    """An axis-aligned box whose faces are k x k quads: 12 k^2 triangles (k = 13: 2028)."""
    import numpy as np
    from vct import scenes
    s = scenes.Scene("box")
    m = s.material(kd)
    c = np.asarray(centre, np.float64)
    t = np.linspace(-half, half, k + 1)
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for sign in (-1.0, 1.0):
            nrm = np.zeros(3)
            nrm[axis] = sign
            for i in range(k):
                for j in range(k):
                    p = []
                    for a, b in ((t[i], t[j]), (t[i + 1], t[j]), (t[i + 1], t[j + 1]), (t[i], t[j + 1])):
                        q = c.copy()
                        q[axis] += sign * half
                        q[u] += a
                        q[v] += b
                        p.append(q)
                    s.quad(*p, nrm, m)
    return s.arrays()


def union(static, layer):
    import numpy as np
    sv, si, sm, sk = static
    lv, li, lm, lk = layer
    return (np.concatenate([sv, lv]), np.concatenate([si, li + np.uint32(sv.shape[0])]),
            np.concatenate([sm, lm + np.uint32(sk.shape[0])]), np.concatenate([sk, lk]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--scenes", default="courtyard,atrium")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--k", type=int, default=13, help="quads per box edge (12 k^2 triangles)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dynamic_bench.json"))
    a = ap.parse_args()
    import numpy as np
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
        for _ in range(16):                 # warm: every position of the path twice
            fn()
        torch.cuda.synchronize()
        reps, ms = 8, []
        while len(ms) < a.blocks:           # a block counts once its calls filled the window
            t = block(fn, reps)
            if t * reps * 1e-3 >= a.window:
                ms.append(t)
            else:
                reps = int(reps * max(1.1 * a.window / max(t * reps * 1e-3, 1e-6), 1.25)) + 1
        return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                "calls": reps * a.blocks, "window_s": round(reps * min(ms) * 1e-3, 3)}

    def to_dev(mesh):
        v, i, m, k = mesh
        return (torch.from_numpy(np.ascontiguousarray(v)).to(dev), torch.from_numpy(i.view(np.int32)).to(dev),
                torch.from_numpy(m.view(np.int32)).to(dev), torch.from_numpy(np.ascontiguousarray(k)).to(dev))

    out = {"tool": "dynamic_bench", "n": n, "width": w, "height": h, "device": torch.cuda.get_device_name(0),
           "blocks": a.blocks, "scenes": {}}
    ok = True
    for name in a.scenes.split(","):
        static = scenes.SCENES[name]().arrays()
        # a loop in the open middle of both scenes, a little above the floor
        path = []
        for p in range(8):
            ang = 2.0 * np.pi * p / 8.0
            path.append(tessellated_box((0.25 * np.cos(ang), -0.55 + 0.15 * np.sin(ang), 0.25 * np.sin(ang)), 0.12, a.k))
        unions = [union(static, layer) for layer in path]
        d_static = to_dev(static)
        d_path = [to_dev(layer) for layer in path]
        d_union = [to_dev(u) for u in unions]
        ctx = Context(n, g0, E, aniso=True, n_diffuse=9, specular=True)
        ctx.set_stream(st.cuda_stream)
        ctx.voxelize_device(*d_static)
        gb = tuple(torch.empty((h, w, 4), device=dev) for _ in range(3))
        diff, spec = (torch.empty((h, w, 4), device=dev) for _ in range(2))
        step = [0]

        def nxt():
            step[0] = (step[0] + 1) % len(path)
            return step[0]

        def light_and_trace():
            ctx.inject_lights([sun])
            ctx.build_mips()
            ctx.trace_device(*gb, w, h, eye, diff, spec)

        def frame_layer():
            ctx.voxelize_dynamic_device(*d_path[nxt()])
            light_and_trace()

        def frame_full():
            ctx.voxelize_device(*d_union[nxt()])
            light_and_trace()

        row = {"static_triangles": int(static[1].size // 3), "layer_triangles": int(path[0][1].size // 3)}
        vox = []
        for layer in d_path:
            ctx.voxelize_dynamic_device(*layer)
            vox.append(ctx.dynamic_voxels())
        row["layer_voxels"] = vox
        ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
        for _ in range(64):                  # K4 settles on its form for this frame first
            light_and_trace()
        torch.cuda.synchronize()
        row["layer_device"] = timed(lambda: ctx.voxelize_dynamic_device(*d_path[nxt()]))
        row["layer_host"] = timed(lambda: ctx.voxelize_dynamic(*path[nxt()]))
        row["frame_layer"] = timed(frame_layer)
        light_and_trace()
        row["frame_relight"] = timed(light_and_trace)
        last = step[0]
        ctx.voxelize_dynamic_device(*d_path[last])
        sums, counts = ctx.download_accum()
        # the parent's way: every move is a voxelization of the whole concatenated mesh
        row["full_device"] = timed(lambda: ctx.voxelize_device(*d_union[nxt()]))
        row["full_host"] = timed(lambda: ctx.voxelize(*unions[nxt()]))
        row["static_device"] = timed(lambda: ctx.voxelize_device(*d_static))
        row["frame_full"] = timed(frame_full)
        ctx.voxelize_device(*d_union[last])
        ref = ctx.download_accum()
        row["check"] = bool(np.array_equal(sums, ref[0]) and np.array_equal(counts, ref[1]))
        ok = ok and row["check"]
        row["layer_over_full"] = round(row["layer_device"]["ms"] / row["full_device"]["ms"], 4)
        row["frame_layer_over_frame_full"] = round(row["frame_layer"]["ms"] / row["frame_full"]["ms"], 4)
        row["trace_form"] = ctx.trace_form
        out["scenes"][name] = row
        ctx.close()
        del ctx, d_static, d_path, d_union, gb, diff, spec
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    if not ok:
        raise SystemExit("the layer's grid differs from a voxelization of the concatenated mesh")


if __name__ == "__main__":
    main()
