"""include/vct_fog.h on the GPU against tests/fog_ref.py (the numpy restatement of vct_spec.h
"volumetric fog").  Every comparison is bit for bit unless stated: the kernels run the spec's
float operations in the spec's order, every cell and every ray is one lane's own, and the only
atomic is the integer sample counter.  The cases, their G-buffers (cast on the CPU, so both
sides see the same positions) and the restatement's results are tests/fog_inputs.py's; the
coverage of those inputs is asserted in tests/test_fog.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fog_inputs as I
import fog_ref as R
import sky_ref
from lights_ref import bits_equal

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 5
F = np.float32
PATTERN = 7.25                    # what the outputs of a refused call are prefilled with


def _ctx(scene, n, aniso=True, nd=9, mips=True, **kw):
    import torch
    from vct import Context
    sc = R.scene(scene, n, aniso)
    ctx = Context(n, sc["g0"], sc["E"], aniso=aniso, n_diffuse=nd, **kw)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.voxelize(*sc["arrays"])
    sc["inject"](ctx)
    if mips:
        ctx.build_mips()
    return ctx, sc


def _case_ctx(case, **kw):
    return _ctx(case.scene, case.n, case.aniso, case.nd, **kw)


def _build(ctx, sc, f):
    ctx.build_fog(R.to_ctypes(f), sc["lights"], [R.TAN] * len(sc["lights"]))


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _filled(h, w, v=float("nan")):
    import torch
    return torch.full((h, w, 4), v, device="cuda")


def _frame(ctx, case, f, cam, pos):
    """rays -> march on the GPU: (ray4, fog4 as numpy, samples)."""
    import torch
    ray, fog4 = _filled(case.h, case.w), _filled(case.h, case.w)
    steps = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.fog_rays_device(cam, case.eye, pos, case.w, case.h, ray)
    ctx.fog_march_device(R.to_ctypes(f), case.eye, ray, case.w, case.h, fog4, steps)
    torch.cuda.synchronize()
    return ray.cpu().numpy(), fog4.cpu().numpy(), int(steps.item())


@pytest.mark.parametrize("name", [c.name for c in I.CASES])
def test_volume_rays_march_apply(gpu_ready, oracle_mod, name):
    """Build: vct_download_fog against the restatement (ambient > 0: fed the oracle's K4, so the
    forced-form launch equals the oracle on the synthetic records).  Rays: cam NULL and not NULL,
    a hostile row in two of the cases.  March: fog4 and the sample counter against the
    restatement fed the GPU's own volume and rays, and fed its own.  Apply: linear4 bit for bit,
    RGBA8 within 1 (the composite tests' bar: the GPU's powf)."""
    import torch
    case = I.BY_NAME[name]
    ref = I.reference(case)
    ctx, sc = _case_ctx(case)
    f = I.fog_of(case)
    _build(ctx, sc, f)
    assert ctx.fog_dims() == case.n >> case.level
    vol = ctx.download_fog()
    d = vol.view(np.uint32) != ref["build"]["S"].view(np.uint32)
    print(name, "cells", vol.shape[0] ** 3, "differing", int(d.any(-1).sum()))
    assert bits_equal(vol, ref["build"]["S"])
    assert (vol[..., :3] > 0).any() and not vol[..., 3].view(np.uint32).any()

    pos = _dev(ref["pos"])
    cam = I.camera(case) if case.cam else None
    ray, fog4, steps = _frame(ctx, case, f, cam, pos)
    print(name, "rays differing", int((ray.view(np.uint32) != ref["rays"].view(np.uint32)).any(-1).sum()))
    assert bits_equal(ray, ref["rays"])
    if case.cam:                                   # the other camera mode on the same frame
        ray0 = _filled(case.h, case.w)
        ctx.fog_rays_device(None, case.eye, pos, case.w, case.h, ray0)
        assert bits_equal(ray0.cpu().numpy(), R.rays(case.n, sc["g0"], sc["E"], case.eye, ref["pos"], None))
    own = R.march(case.n, sc["g0"], sc["E"], f, case.eye, ray, vol)
    print(name, "samples", steps, "restatement", own["steps"], ref["march"]["steps"])
    assert bits_equal(fog4, own["fog4"]) and steps == own["steps"]
    assert bits_equal(fog4, ref["march"]["fog4"]) and steps == ref["march"]["steps"]
    assert np.isfinite(fog4).all()

    rng = np.random.default_rng(11)
    lin0 = (rng.random((case.h, case.w, 4)) * 4).astype(F)
    lin0[..., 3] = ref["pos"][..., 3] != 0          # alpha as a composite leaves it: 0 marks the background
    lin = _dev(lin0)
    rgba = torch.zeros((case.h, case.w), dtype=torch.int32, device="cuda")
    ctx.fog_apply_device(_dev(fog4), case.w, case.h, lin, rgba)
    torch.cuda.synchronize()
    want_lin, want8 = R.apply(fog4, lin0)
    assert bits_equal(lin.cpu().numpy(), want_lin)
    got8 = rgba.cpu().numpy().view(np.uint32)
    for sh in (0, 8, 16, 24):
        dd = np.abs(((got8 >> sh) & 255).astype(np.int64) - ((want8 >> sh) & 255).astype(np.int64))
        assert dd.max() <= 1, (sh, int(dd.max()))
    only8 = torch.zeros((case.h, case.w), dtype=torch.int32, device="cuda")      # the fog layer alone
    ctx.fog_apply_device(_dev(fog4), case.w, case.h, None, only8)
    torch.cuda.synchronize()
    layer = R.apply(fog4, None)[1]
    assert np.abs(((only8.cpu().numpy().view(np.uint32) >> 8) & 255).astype(np.int64)
                  - ((layer >> 8) & 255).astype(np.int64)).max() <= 1
    ctx.close()


def test_hostile_rows_reach_the_gpu(gpu_ready, oracle_mod):
    """Both hostile rows hold every class of tests/fog_inputs.py (NaN on each axis, +-inf, 1e30,
    denormal, hostile pos.w, far and near outside, P == eye), and the GPU's record of each is the
    restatement's: +0 in all four channels for what is not a ray."""
    import torch
    for case in (c for c in I.CASES if c.hostile):
        cls = I.hostile_classes(case)
        assert set(cls) == set(I.HOSTILE_CLASSES)
        ref = I.reference(case)
        sc = R.scene(case.scene, case.n, case.aniso)
        from vct import Context
        ctx = Context(case.n, sc["g0"], sc["E"])                 # the rays need no grid state
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ray = _filled(case.h, case.w)
        ctx.fog_rays_device(I.camera(case), case.eye, _dev(ref["pos"]), case.w, case.h, ray)
        torch.cuda.synchronize()
        got = ray.cpu().numpy()
        ctx.close()
        assert bits_equal(got[0], ref["rays"][0])
        for x, k in enumerate(cls):
            if k in ("eye", "nan_x", "nan_y", "nan_z", "posinf", "neginf", "big"):
                assert not got[0, x].view(np.uint32).any(), (case.name, x, k, got[0, x])


def test_march_of_hand_made_rays(gpu_ready, oracle_mod):
    """Records a G-buffer cannot produce, straight into the march: components whose reciprocal
    overflows (|d_c| <= 2^-128, treated as 0 by the slab), exact zeros, an axis ray from outside,
    o outside a non-clipping axis' slab, NaN and infinite d, len 0, negative and NaN."""
    import torch
    case = I.BY_NAME["cornell_in_l1"]
    ctx, sc = _case_ctx(case)
    f = I.fog_of(case)
    _build(ctx, sc, f)
    vol = ctx.download_fog()
    tiny, inf, nan = float(F(2.0 ** -130)), float("inf"), float("nan")
    rows = [[1, tiny, -tiny, inf], [1, 0, 0, inf], [-1, 0, 0, inf], [0, 1, 0, 7.5], [0, tiny, 1, inf],
            [float(F(2.0 ** -127)), 0, -1, inf], [0.6, 0.8, 0, inf], [0, 0, 0, 5.0], [0, 0, 0, inf],
            [nan, 0, 1, 3.0], [0, inf, 0, 3.0], [1, 0, 0, 0.0], [1, 0, 0, -2.0], [1, 0, 0, nan], [0, 0, 0, 0]]
    ray = np.array(rows, F).reshape(1, len(rows), 4)
    for eye in (R.EYE_IN, (-3.0, 0.1, 0.2), (0.1, 5.0, 0.2)):        # inside; outside along x; outside along y
        fog4 = _filled(1, len(rows))
        steps = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.fog_march_device(R.to_ctypes(f), eye, _dev(ray), len(rows), 1, fog4, steps)
        torch.cuda.synchronize()
        want = R.march(case.n, sc["g0"], sc["E"], f, eye, ray, vol)
        print(eye, "samples", int(steps.item()), "ends", want["end"][0].tolist())
        assert bits_equal(fog4.cpu().numpy(), want["fog4"]) and int(steps.item()) == want["steps"]
        assert np.isfinite(want["fog4"]).all()
    ctx.close()


def test_zero_lights_zero_ambient_only_attenuates(gpu_ready, oracle_mod):
    case = I.BY_NAME["cornell_in_l1"]
    ctx, sc = _case_ctx(case)
    f = R.fog(2.0, level=1)
    ctx.build_fog(R.to_ctypes(f), [], None)
    vol = ctx.download_fog()
    assert not vol.view(np.uint32).any()
    _, fog4, steps = _frame(ctx, case, f, I.camera(case), _dev(I.gbuffer(case)[0]))
    assert steps > 0 and not fog4[..., :3].view(np.uint32).any() and (fog4[..., 3] < 1).any()
    ctx.close()


def test_64_bit_path_and_cone_steps(gpu_ready, oracle_mod):
    """vct_debug_fog(force64) sends the light cones of a 32^3 grid through the path 1024^3 takes:
    the same volume; and the build's light-cone steps are the restatement's on both paths."""
    import torch
    from vct import _lib
    case = I.BY_NAME["atrium_out_l1"]
    ref = I.reference(case)
    ctx, sc = _case_ctx(case)
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.debug_fog(ctx.lib, ctx.h, counters=(cnt.data_ptr(), 0))
    assert _lib.debug_fog(ctx.lib, ctx.h) == 0
    try:
        for force, path in ((0, 32), (1, 64)):
            _lib.debug_fog(ctx.lib, force64=force)
            cnt.zero_()
            _build(ctx, sc, I.fog_of(case))
            assert bits_equal(ctx.download_fog(), ref["build"]["S"])
            assert _lib.debug_fog(ctx.lib, ctx.h) == path
            assert int(cnt[0].item()) == ref["build"]["steps"] > 0
    finally:
        _lib.debug_fog(ctx.lib, force64=0)
    ctx.close()


def test_composite_unchanged_and_shares_the_tone_curve(gpu_ready, oracle_mod):
    """vct_composite_device after the tone curve moved into the shared header: its linear frame
    is the oracle's bit for bit and its RGBA8 within 1, as before; and the identity fog
    (F = 0, T = 1) through vct_fog_apply_device gives the composite's RGBA8 exactly at every
    pixel, the background's clear colour included: one device function serves both."""
    import torch
    from vct import scenes
    O = oracle_mod
    case = I.BY_NAME["cornell_in_l1"]
    ctx, sc = _case_ctx(case)
    pos, nrm, alb = I.gbuffer(I.BY_NAME["cornell_out_l2"])
    h, w = pos.shape[:2]
    gb = [_dev(a) for a in (pos, nrm, alb)]
    d, sp, lin = _filled(h, w), _filled(h, w), _filled(h, w)
    rgba = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    ctx.trace_device(*gb, w, h, R.EYE_OUT, d, sp)
    ctx.composite_device(*gb, d, sp, w, h, scenes.LIGHT_DIR, scenes.LIGHT_COLOR, out_linear4=lin, out_rgba8=rgba)
    torch.cuda.synchronize()
    grid = __import__("lights_ref").cornell(case.n)["grid"]
    want_lin, want8 = O.composite(case.n, sc["g0"], sc["E"], grid["albedo_occ"], pos, nrm, alb, d.cpu().numpy(),
                                  sp.cpu().numpy(), scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    assert bits_equal(lin.cpu().numpy(), want_lin)
    got8 = rgba.cpu().numpy().view(np.uint32)
    for sh in (0, 8, 16, 24):
        assert np.abs(((got8 >> sh) & 255).astype(np.int64) - ((want8 >> sh) & 255).astype(np.int64)).max() <= 1
    ident = torch.zeros((h, w, 4), device="cuda")
    ident[..., 3] = 1.0
    again = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    lin2 = lin.clone()
    ctx.fog_apply_device(ident, w, h, lin2, again)
    torch.cuda.synchronize()
    assert bits_equal(lin2.cpu().numpy(), lin.cpu().numpy())
    assert np.array_equal(again.cpu().numpy(), rgba.cpu().numpy())
    ctx.close()


def test_state_machine(gpu_ready, oracle_mod):
    import torch
    import vct
    from vct import VctError, scenes
    case = I.BY_NAME["cornell_out_l2"]
    ctx, sc = _case_ctx(case)
    f = I.fog_of(case)
    pos = _dev(I.gbuffer(case)[0])
    ray, fog4 = _filled(case.h, case.w), _filled(case.h, case.w, PATTERN)
    ctx.fog_rays_device(None, case.eye, pos, case.w, case.h, ray)      # needs no volume

    def march(ff=f):
        ctx.fog_march_device(R.to_ctypes(ff), case.eye, ray, case.w, case.h, fog4)

    def estate(fn):
        with pytest.raises(VctError) as e:
            fn()
        assert e.value.status == ESTATE
        torch.cuda.synchronize()
        assert (fog4 == PATTERN).all()

    estate(march)                                   # before any build
    estate(ctx.fog_dims)
    estate(ctx.download_fog)
    _build(ctx, sc, f)
    march()
    torch.cuda.synchronize()
    first = fog4.cpu().numpy()
    fog4.fill_(PATTERN)
    estate(lambda: march({**f, "level": 1}))        # another level
    sc["inject"](ctx)                               # a relight without a rebuild: level 0 changed
    estate(march)
    ctx.build_mips()                                # ... and a new pyramid
    estate(march)
    _build(ctx, sc, f)                              # rebuild, then march is fine and gives the same frame
    march()
    torch.cuda.synchronize()
    assert bits_equal(fog4.cpu().numpy(), first)
    fog4.fill_(PATTERN)
    ctx.inject_sky(vct.sky_light((0.2, 0.3, 0.5)))  # a sky inject rebuilds the mips
    estate(march)
    ctx.close()
    # before the mips: the build itself is refused
    ctx, sc = _case_ctx(case, mips=False)
    with pytest.raises(VctError) as e:
        _build(ctx, sc, f)
    assert e.value.status == ESTATE
    ctx.close()


def test_build_on_a_second_stream_after_a_sky_call(gpu_ready, oracle_mod):
    """A build queued on another stream than the previous sky call (both use the context's step
    tables) gives the volume of the one-stream order."""
    import torch
    case = I.BY_NAME["cornell_in_l1"]
    ref = I.reference(case)
    ctx, sc = _case_ctx(case)
    f = I.fog_of(case)
    pos, nrm, _ = (_dev(a) for a in I.gbuffer(I.BY_NAME["cornell_out_l2"]))
    h, w = pos.shape[:2]
    sky4 = _filled(h, w)
    ctx.sky_cones_device(pos, nrm, w, h, sky_ref.to_ctypes(sky_ref.SKY), sky4)
    s2 = torch.cuda.Stream()
    ctx.set_stream(s2.cuda_stream)
    _build(ctx, sc, f)
    vol = ctx.download_fog()
    assert bits_equal(vol, ref["build"]["S"])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.close()


def test_errors_leave_everything_untouched(gpu_ready, oracle_mod):
    """Every VCT_EINVAL of the library itself (the raw entry points, past the binding's own
    validator) leaves the outputs (prefilled with a pattern) and the current volume as they were."""
    import torch
    import vct
    from vct import _lib
    case = I.BY_NAME["cornell_out_l2"]
    ctx, sc = _case_ctx(case)
    f = I.fog_of(case)
    _build(ctx, sc, f)
    before = ctx.download_fog()
    lib = ctx.lib
    build, rays, march, apply = (_lib.bind_fog_extension(lib, "vct_" + k) for k in
                                 ("build_fog", "fog_rays_device", "fog_march_device", "fog_apply_device"))
    h, w = case.h, case.w
    pos = _dev(I.gbuffer(case)[0])
    ray, fog4, lin = _filled(h, w, PATTERN), _filled(h, w, PATTERN), _filled(h, w, PATTERN)
    rgba = torch.full((h, w), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    good = R.to_ctypes(f)
    eye = (C.c_float * 3)(*case.eye)
    arr = (vct.VctLight * 3)(*sc["lights"])
    tans = (C.c_float * 3)(R.TAN, R.TAN, R.TAN)
    P = lambda t: C.c_void_p(t.data_ptr())
    n_bad = 0
    import test_fog
    for bad in test_fog.ILLEGAL:
        ff = R.to_ctypes({**f, **bad})
        assert build(ctx.h, C.byref(ff), arr, 3, tans) == EINVAL, bad
        assert march(ctx.h, C.byref(ff), eye, P(ray), w, h, P(fog4), None) == EINVAL, bad
        n_bad += 1
    for t in (0.0, -0.1, float("nan"), float("inf")):
        assert build(ctx.h, C.byref(good), arr, 3, (C.c_float * 3)(R.TAN, t, R.TAN)) == EINVAL, t
    assert build(ctx.h, C.byref(good), arr, 65, tans) == EINVAL
    assert build(ctx.h, C.byref(good), arr, 3, None) == EINVAL
    assert build(ctx.h, None, arr, 3, tans) == EINVAL
    dark = (vct.VctLight * 1)(vct.directional_light((0.0, 0.0, 0.0)))
    assert build(ctx.h, C.byref(good), dark, 1, tans) == EINVAL          # the light list's own rule
    for e in ((float("nan"), 0, 0), (0, float("inf"), 0), (3e38, 0, 0)):  # the last: finite, o overflows
        ee = (C.c_float * 3)(*e)
        assert march(ctx.h, C.byref(good), ee, P(ray), w, h, P(fog4), None) == EINVAL, e
        assert rays(ctx.h, None, ee, P(pos), w, h, P(ray)) == EINVAL, e
    assert rays(ctx.h, None, eye, P(pos), w, h, C.c_void_p(ray.data_ptr() + 4)) == EINVAL       # misaligned
    assert rays(ctx.h, None, eye, None, w, h, P(ray)) == EINVAL
    assert rays(ctx.h, None, eye, P(pos), 0, h, P(ray)) == EINVAL
    assert march(ctx.h, C.byref(good), eye, P(ray), w, h, C.c_void_p(fog4.data_ptr() + 8), None) == EINVAL
    assert march(ctx.h, C.byref(good), eye, P(ray), w, h, P(fog4), C.c_void_p(fog4.data_ptr() + 4)) == EINVAL
    assert march(ctx.h, C.byref(good), eye, None, w, h, P(fog4), None) == EINVAL
    assert apply(ctx.h, P(fog4), w, h, None, None) == EINVAL
    assert apply(ctx.h, None, w, h, P(lin), P(rgba)) == EINVAL
    assert apply(ctx.h, P(fog4), w, h, C.c_void_p(lin.data_ptr() + 4), P(rgba)) == EINVAL
    assert apply(ctx.h, P(fog4), w, h, P(lin), C.c_void_p(rgba.data_ptr() + 2)) == EINVAL
    torch.cuda.synchronize()
    assert n_bad == len(test_fog.ILLEGAL)
    for t in (ray, fog4, lin):
        assert (t == PATTERN).all()
    assert (rgba == 0x5a5a5a5a).all()
    assert bits_equal(ctx.download_fog(), before)            # still current, and unchanged
    ctx.close()


def test_multi_device_context(gpu_ready, oracle_mod):
    """A vct_create_multi context of 2 ranks on the one device: device 0 builds and keeps the
    volume, and the frame is the single context's."""
    case = I.BY_NAME["cornell_in_l1"]
    ref = I.reference(case)
    f = I.fog_of(case)
    ctx, sc = _case_ctx(case, devices=2, device=0)
    _build(ctx, sc, f)
    assert bits_equal(ctx.download_fog(), ref["build"]["S"])
    _, fog4, steps = _frame(ctx, case, f, I.camera(case), _dev(ref["pos"]))
    ctx.close()
    assert bits_equal(fog4, ref["march"]["fog4"]) and steps == ref["march"]["steps"]


def test_cpp_host_fog_flag(gpu_ready, tmp_path):
    """vct_headless --fog 1.5 writes the frame the binding's build_fog / fog_rays / fog_march /
    fog_apply give on the host's own geometry, grid, camera and composite, and it differs from
    the frame without the flag -- which is the surface composite, as before."""
    import re
    import torch
    import host_lib
    import vct
    from helpers import write_obj
    from vct import Context, VctCamera, _lib, scenes
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "voxel-based-global-illumination_amd", "build", "vct_headless")
    assert os.path.exists(exe), "build the host with `make -C voxel-based-global-illumination_amd host`"
    obj = write_obj(scenes.cornell(), str(tmp_path))
    n, w, h = 32, 96, 64
    light = ["--light", "point:0,0.6,0.1:4,4,3:2.5"]
    frames = {}
    for name, flags in (("plain", []), ("fog", ["--fog", "1.5"])):
        lin = str(tmp_path / f"{name}.f32")
        p = subprocess.run([exe, obj, str(n), str(w), str(h), "2", str(tmp_path / f"{name}.ppm"),
                            "--model=identity", "--grid=unit", f"--linear={lin}"] + light + flags,
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        frames[name] = np.fromfile(lin, np.float32).reshape(h, w, 4)
        grid = re.search(r"aabb_min (\S+) (\S+) (\S+) extent (\S+)", p.stdout)
    assert not np.array_equal(frames["plain"], frames["fog"])
    g0 = tuple(float.fromhex(grid.group(j)) for j in (1, 2, 3))
    E = float.fromhex(grid.group(4))
    v, i, m, k, _, _ = host_lib.load_placed(obj)
    ctx = Context(n, g0, E)
    ctx.voxelize(v, i, m, k)
    lights = [vct.point_light((0.0, 0.6, 0.1), (4.0, 4.0, 3.0), 2.5)]
    ctx.inject_lights(lights)
    ctx.build_mips()
    c = host_lib.camera_eval((0.0, 0.0, 3.0, -90.0, 0.0), [])  # the host's float camera (main.cpp)
    cam = VctCamera()
    f3 = lambda a: (C.c_float * 3)(*[float(t) for t in a])
    cam.position, cam.front, cam.right, cam.up = f3(c[0:3]), f3(c[3:6]), f3(c[6:9]), f3(c[9:12])
    cam.zoom_deg, cam.near_plane, cam.far_plane = float(c[14]), 0.1, 100.0
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    gb = [torch.empty((h, w, 4), device="cuda") for _ in range(3)]
    ctx.gbuffer_raster_device(cam, w, h, 0.1, *gb)
    d, sp, lin = (torch.empty((h, w, 4), device="cuda") for _ in range(3))
    eye = tuple(c[0:3])
    ctx.trace_device(*gb, w, h, eye, d, sp)
    ctx.composite_lights_device(*gb, d, sp, w, h, lights, out_linear4=lin)
    torch.cuda.synchronize()
    assert bits_equal(lin.cpu().numpy(), frames["plain"])       # without the flag: the surface composite
    fog = vct.fog(1.5)                                          # the header defaults
    ctx.build_fog(fog, lights, [_lib.VCT_FOG_DEFAULT_TAN])
    ray, fog4 = torch.empty((h, w, 4), device="cuda"), torch.empty((h, w, 4), device="cuda")
    ctx.fog_rays_device(cam, eye, gb[0], w, h, ray)
    ctx.fog_march_device(fog, eye, ray, w, h, fog4)
    ctx.fog_apply_device(fog4, w, h, lin)
    torch.cuda.synchronize()
    assert bits_equal(lin.cpu().numpy(), frames["fog"])
    assert (fog4[..., 3] < 1).any() and (fog4[..., :3] > 0).any()
    ctx.close()
