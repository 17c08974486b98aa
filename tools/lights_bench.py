"""vct_inject_lights on one GPU: the atrium at 256^3 (or --scene / --n).  One JSON line, also
written to profiles/lights_bench.json.  Device events on the context's stream, warmed; every
line is `--blocks` blocks of `--reps` back-to-back launches (at least 200 launches), reported
as the median block's ms per launch with the fastest and slowest block beside it.

  (a)  vct_inject_directional, the reference point, measured twice (before and after the
       rest: its run-to-run spread in the same process)
  (b)  the same light through vct_inject_lights (routed to the same kernels)
  (b') the same light through the light kernels (routing off; not the shipped path)
  (c)  one point light in the court, its range covering the grid
  (d)  8 point lights under the galleries, range 0.6
  (e)  (d) plus the directional light
For (c) to (e): both forms -- one light per pass (plain) and batched pairs -- alternated
block by block, with the pairs walked, the cells the walks test and cells per second, and
a check that the two forms give the same level 0.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "voxel-based-global-illumination_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--scene", default="atrium")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lights_bench.json"))
    a = ap.parse_args()
    import torch
    import vct
    from vct import Context, _lib, scenes
    n = a.n
    g0, E = scenes.grid_for_unit_box(n)
    ctx = Context(n, g0, E)
    st = torch.cuda.current_stream()
    ctx.set_stream(st.cuda_stream)
    ctx.voxelize(*scenes.SCENES[a.scene]().arrays())
    lib = ctx.lib

    sun = vct.directional_light(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    court = vct.point_light((0.0, -0.3, 0.0), (6.0, 6.0, 5.0), 4.0)
    lamps = [vct.point_light((x, -0.1, z), (1.0, 0.8, 0.5), 0.6) for x in (-0.78, 0.78) for z in (-0.7, -0.25, 0.2, 0.65)]

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    def summary(ms):
        return {"ms": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5),
                "launches": len(ms) * a.reps}

    def timed(fns):
        """Alternate the callables block by block; -> one summary per callable."""
        for fn in fns:
            for _ in range(a.reps):
                fn()
        torch.cuda.synchronize()
        ms = [[] for _ in fns]
        for _ in range(a.blocks):
            for k, fn in enumerate(fns):
                ms[k].append(block(fn))
        return [summary(m) for m in ms]

    def digest():
        return hashlib.sha256(ctx.download_level(0).tobytes()).hexdigest()[:16]

    def counted(lights, form):
        _lib.debug_lights(lib, form=form, count=True, route=False)
        ctx.inject_lights(lights)
        pairs, cells = _lib.debug_lights_stats(lib, ctx.h)
        h = digest()
        _lib.debug_lights(lib)
        return pairs, cells, h

    def with_form(lights, form, route=True):
        def fn():
            _lib.debug_lights(lib, form=form, route=route)
            ctx.inject_lights(lights)
        return fn

    out = {"scene": a.scene, "n": n, "device": torch.cuda.get_device_name(0), "reps": a.reps, "blocks": a.blocks}
    directional = lambda: ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    a1, b, b_kernels = timed([directional, with_form([sun], -1), with_form([sun], -1, route=False)])
    out["a_inject_directional"] = a1
    out["b_inject_lights_directional"] = b
    pairs, cells, h_dir = counted([sun], 1)
    b_kernels.update(pairs=pairs, cells=cells, cells_per_s=round(cells / (b_kernels["ms"] * 1e-3), 0))
    out["b_through_light_kernels"] = b_kernels
    directional()
    out["directional_level0_equal"] = digest() == h_dir
    for key, lights in (("c_court_point_light", [court]), ("d_8_gallery_lamps", lamps),
                        ("e_8_lamps_and_directional", lamps + [sun])):
        plain, batched = timed([with_form(lights, 0), with_form(lights, 1)])
        p0, c0, h0 = counted(lights, 0)
        p1, c1, h1 = counted(lights, 1)
        for row, (p, c) in ((plain, (p0, c0)), (batched, (p1, c1))):
            row.update(pairs=p, cells=c, cells_per_s=round(c / (row["ms"] * 1e-3), 0))
        out[key] = {"lights": len(lights), "plain": plain, "batched": batched, "level0_equal": h0 == h1,
                    "batched_over_plain": round(batched["ms"] / plain["ms"], 4)}
    _lib.debug_lights(lib)
    (a2,) = timed([directional])
    out["a_inject_directional_again"] = a2
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
