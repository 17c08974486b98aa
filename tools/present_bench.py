"""The HDR present (include/vct_present.h) on one GPU at the bench's 1080p frame: the atrium,
traced and composited at 256^3, and a constant frame (every pixel in one bin: the meter's worst
case).  One JSON line, also written to profiles/present_bench.json.  Device events on the
context's stream, warmed; every figure is the median of `--blocks` blocks of back-to-back calls,
each block grown until its calls fill `--window` seconds, with the fastest and slowest block
beside it (tools/shading_bench.py's method).  No counters are collected here.

  float4_copy:   a device-to-device copy of one plane in this session: bytes written per second
  meter:         vct_luminance_meter_device on both frames, in both forms of the kernel (`per_lane`,
                 the default: one LDS atomic per lane; `folded`: the wave's first live key is
                 added once), beside the compulsory traffic (one float4 read of the frame) at the
                 copy rate
  exposure:      vct_exposure_update_device
  bloom:         levels 1 (the prefilter alone) and 5; chain = the difference; the prefilter's
                 compulsory traffic is one read of the frame and one write of a quarter of it
  present:       the identity configuration beside vct_fog_apply_device with out_rgba8 on the same
                 frame (T = 1, F = 0: the same tone-and-pack, one plane more to read and one to
                 write), then ACES + sRGB + dither + bloom
"""
import argparse
import ctypes as C
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
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per block")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "present_bench.json"))
    a = ap.parse_args()
    import torch
    from vct import Context, _lib, scenes
    from vct.camera import Camera
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
        return {"ms": round(statistics.median(ms), 5), "min": round(min(ms), 5), "max": round(max(ms), 5),
                "calls": reps * a.blocks, "window_s": round(reps * min(ms) * 1e-3, 3)}

    ctx = Context(n, g0, E)
    ctx.set_stream(st.cuda_stream)
    ctx.voxelize(*scenes.SCENES[a.scene]().arrays())
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    ctx.build_mips()
    z = lambda: torch.zeros((h, w, 4), device=dev)
    pos, nrm, alb, diff, spec, lin, src, dst = z(), z(), z(), z(), z(), z(), z(), z()
    ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, pos, nrm, alb)
    ctx.trace_device(pos, nrm, alb, w, h, cam.position, diff, spec)
    ctx.composite_device(pos, nrm, alb, diff, spec, w, h, scenes.LIGHT_DIR, scenes.LIGHT_COLOR, out_linear4=lin)
    torch.cuda.synchronize()
    del pos, nrm, alb, diff, spec
    flat = torch.ones((h, w, 4), device=dev)
    flat[..., :3] = torch.tensor([3.0, 2.0, 0.5], device=dev)
    frames = {a.scene: lin, "constant": flat}

    fn = {name: _lib.bind_present_extension(ctx.lib, name) for name in _lib.PRESENT_EXTENSIONS}
    hist = torch.zeros(512, dtype=torch.int32, device=dev)
    counts = torch.zeros(4, dtype=torch.int32, device=dev)
    state = torch.zeros(4, device=dev)
    rgba = torch.zeros((h, w), dtype=torch.int32, device=dev)
    nbytes = C.c_size_t()
    assert fn["vct_bloom_scratch_bytes"](w, h, 5, C.byref(nbytes)) == 0
    scratch = torch.zeros(nbytes.value // 4, device=dev)

    def ok(status):
        assert status == 0, ctx.lib.vct_last_error(ctx.h)

    out = {"tool": "present_bench", "n": n, "scene": a.scene, "width": w, "height": h, "device": torch.cuda.get_device_name(0),
           "blocks": a.blocks, "counters": "none: device-event times only"}
    copy = timed(lambda: dst.copy_(src))
    plane_bytes = w * h * 16
    rate = plane_bytes / (copy["ms"] * 1e-3)
    out["float4_copy"] = dict(copy, plane_bytes=plane_bytes, written_GBps=round(rate / 1e9, 1))
    read_floor = plane_bytes / rate * 1e3
    out["valid_pixels"] = int((lin[..., 3] != 0).sum().item())

    out["meter"] = {"one_read_floor_ms": round(read_floor, 5)}
    for form, agg in (("per_lane", 0), ("folded", 1)):
        _lib.debug_present(ctx.lib, agg)
        row = {}
        for name, frame in frames.items():
            row[name] = timed(lambda: ok(fn["vct_luminance_meter_device"](ctx.h, frame.data_ptr(), w, h, hist.data_ptr(), counts.data_ptr())))
            row[name]["over_floor"] = round(row[name]["ms"] / read_floor, 3)
        row["constant_over_scene"] = round(row["constant"]["ms"] / row[a.scene]["ms"], 3)
        out["meter"][form] = row
    _lib.debug_present(ctx.lib, 0)
    ok(fn["vct_luminance_meter_device"](ctx.h, lin.data_ptr(), w, h, hist.data_ptr(), counts.data_ptr()))

    ep = _lib.VctExposureParams(0.18, 2.0 ** -12, 2.0 ** 12, 100, 20, 0.1, 0.05, 0)
    out["exposure"] = timed(lambda: ok(fn["vct_exposure_update_device"](ctx.h, hist.data_ptr(), counts.data_ptr(), C.byref(ep),
                                                                          state.data_ptr(), state.data_ptr())))
    torch.cuda.synchronize()
    out["exposure"]["state"] = [round(float(v), 6) for v in state[:3].tolist()]

    bloom = {}
    for levels in (1, 5):
        bp = _lib.VctBloomParams(1.0, levels, 1.0, 0)
        bloom[f"levels_{levels}"] = timed(lambda: ok(fn["vct_bloom_device"](ctx.h, lin.data_ptr(), w, h, C.byref(bp), state.data_ptr(),
                                                                             scratch.data_ptr(), scratch.numel() * 4)))
    pre_floor = (plane_bytes + plane_bytes / 4) / rate * 1e3     # bytes moved at the copy's written-bytes rate, as the meter's floor
    bloom["prefilter_ms"] = bloom["levels_1"]["ms"]
    bloom["chain_ms"] = round(bloom["levels_5"]["ms"] - bloom["levels_1"]["ms"], 5)
    bloom["prefilter_floor_ms"] = round(pre_floor, 5)
    bloom["prefilter_over_floor"] = round(bloom["levels_1"]["ms"] / pre_floor, 3)
    out["bloom"] = bloom

    fog4 = torch.zeros((h, w, 4), device=dev)
    fog4[..., 3] = 1.0                                            # T = 1, F = 0: the frame stays what it is
    present = {"fog_apply_rgba8": timed(lambda: ctx.fog_apply_device(fog4, w, h, lin, rgba))}
    ident = _lib.VctPresentParams(0, 0, 0, 1.0, 1.0, 0.0)
    present["identity"] = timed(lambda: ok(fn["vct_present_device"](ctx.h, lin.data_ptr(), w, h, C.byref(ident), None, None, None,
                                                                     rgba.data_ptr())))
    full = _lib.VctPresentParams(_lib.VCT_CURVE_ACES, _lib.VCT_TRANSFER_SRGB, 1, 1.0, 4.0, 0.25)
    present["aces_srgb_dither_bloom"] = timed(lambda: ok(fn["vct_present_device"](ctx.h, lin.data_ptr(), w, h, C.byref(full), state.data_ptr(),
                                                                                   scratch.data_ptr(), None, rgba.data_ptr())))
    present["identity_over_fog_apply"] = round(present["identity"]["ms"] / present["fog_apply_rgba8"]["ms"], 3)
    present["full_over_identity"] = round(present["aces_srgb_dither_bloom"]["ms"] / present["identity"]["ms"], 3)
    out["present"] = present
    ctx.close()
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
