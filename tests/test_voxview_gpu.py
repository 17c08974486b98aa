"""vct_voxel_pick_device / vct_voxel_view_device on the GPU against tests/voxview_ref.py (a numpy
restatement of vct_spec.h "voxel view", pinned in tests/test_voxview.py to the shadow walk, to a
float64 caster and to hand-written records).  Every comparison is bit for bit -- the kernel runs
the spec's float operations in the spec's order, every ray is one lane's own, and the only
atomic is the integer counter of tested cells -- except the RGBA8 frame, which is within one
step, as the composites' is (the GPU's powf).  Grids are the Cornell box of lights_ref.cornell
with light set S.  The kernels take the plain walk only, so there is no second form to compare.
"""
import numpy as np
import pytest

import dynamic_ref as D
import light_inputs as LI
import lights_ref
import query_ref
import shadow_ref
import sky_view_ref
import voxview_ref as VV
from test_voxview import HAND, f32bits, hand_grid, inside_rays

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 5
F = np.float32
INF = F(np.inf)
NAN_FILL = 0x7FC00000


def _ctx(n, lit=True, **kw):
    import torch
    from vct import Context
    ref = lights_ref.cornell(n)
    ctx = Context(n, ref["g0"], ref["E"], **kw)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.voxelize(*ref["arrays"])
    if lit:
        ctx.inject_lights(ref["lights"])
        ctx.build_mips()
    return ctx


def _pick(ctx, org, dirv, lim=INF, level=0, solid=VV.OCCUPANCY):
    """-> (hit4 [R, 4] uint32, counter) of one call, hit4 pre-filled with NaN bits."""
    import torch
    org = np.asarray(org, F).reshape(-1, 3)
    R = org.shape[0]
    o4 = np.zeros((R, 4), F)
    d4 = np.zeros((R, 4), F)
    o4[:, :3] = org
    d4[:, :3] = np.asarray(dirv, F).reshape(-1, 3)
    d4[:, 3] = lim
    hit = torch.full((R, 4), NAN_FILL, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.voxel_pick_device(torch.from_numpy(o4).cuda(), torch.from_numpy(d4).cuda(), R, hit, level, solid, cnt)
    torch.cuda.synchronize()
    return hit.cpu().numpy().view(np.uint32), int(cnt.item())


def _view(ctx, cam, w, h, level, mode, shade):
    """-> dict(linear4, rgba8, hit4, cells) of one call, the outputs pre-filled with NaN."""
    import torch
    lin = torch.full((h, w, 4), float("nan"), device="cuda")
    q = torch.full((h, w), NAN_FILL, dtype=torch.int32, device="cuda")
    hit = torch.full((h, w, 4), NAN_FILL, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.voxel_view_device(cam, w, h, level, mode, shade, lin, q, hit, cnt)
    torch.cuda.synchronize()
    return {"linear4": lin.cpu().numpy(), "rgba8": q.cpu().numpy().view(np.uint32),
            "hit4": hit.cpu().numpy().view(np.uint32), "cells": int(cnt.item())}


def _same_records(got, ref, what=""):
    bad = np.flatnonzero((got.reshape(-1, 4) != ref.reshape(-1, 4)).any(-1))
    assert not bad.size, f"{what}: {bad.size} records differ, first {bad[:6]}: {got.reshape(-1, 4)[bad[:3]]} != " \
                         f"{ref.reshape(-1, 4)[bad[:3]]}"


def _same_view(got, ref, what):
    _same_records(got["hit4"], ref["hit4"], what)
    assert got["cells"] == ref["cells"], what
    assert lights_ref.bits_equal(got["linear4"], ref["linear4"]), what
    assert sky_view_ref.bytes_within_one(got["rgba8"], ref["rgba8"]), what
    miss = ref["hit4"][..., 0] == VV.CELL_MISS
    assert not got["rgba8"][miss].any(), what


def _solid(n, aniso, level, solid):
    c = lights_ref.cornell(n)
    if solid == VV.OCCUPANCY:
        return VV.solid_occupancy(c["grid"]["albedo_occ"])
    return VV.solid_alpha(query_ref.cornell_pyramid(n, aniso), level)


# ---- n = 4: one ray, then a wave and one lane ----------------------------------------------------
@pytest.mark.parametrize("count", [1, 65])
def test_small_grid(gpu_ready, oracle_mod, count):
    n = 4
    c = lights_ref.cornell(n)
    org, d = VV.view_rays(VV.cameras()["oblique"], 13, 5)
    org, d = org[27:27 + count], d[27:27 + count]
    ctx = _ctx(n)
    try:
        for level, solid in ((0, VV.OCCUPANCY), (0, VV.ALPHA), (1, VV.ALPHA), (2, VV.ALPHA)):
            ref = VV.pick(n, c["g0"], c["E"], _solid(n, True, level, solid), level, org, d)
            got, cells = _pick(ctx, org, d, INF, level, solid)
            _same_records(got, ref["hit4"], f"level {level} solid {solid}")
            assert cells == int(ref["steps"].sum()) and ref["steps"][-1] > 0
            assert ref["hit"].any()
    finally:
        ctx.close()


# ---- n = 16: every mode, level and shade from the three cameras -----------------------------------
@pytest.mark.parametrize("aniso", [True, False])
@pytest.mark.parametrize("name", ["outside", "inside", "oblique"])
def test_cornell_views(gpu_ready, oracle_mod, name, aniso):
    n, L = 16, 4
    c = lights_ref.cornell(n)
    w, h = shadow_ref.FRAMES[n]
    cam = VV.cameras()[name]
    kw = dict(pyr=query_ref.cornell_pyramid(n, aniso), aniso=aniso, albedo_occ=c["grid"]["albedo_occ"],
              normal=c["grid"]["normal"])
    cases = [(0, VV.ALBEDO), (0, VV.NORMAL)] + [(l, m) for l in range(L + 1) for m in (VV.RADIANCE, VV.MODE_ALPHA)]
    ctx = _ctx(n, aniso=aniso)
    try:
        assert np.array_equal(ctx.download_level(0), c["level0"])
        for level, mode in cases:
            for shade in (0, 1):
                ref = VV.view(n, c["g0"], c["E"], cam, w, h, level, mode, shade, **kw)
                got = _view(ctx, cam, w, h, level, mode, shade)
                _same_view(got, ref, f"{name} level {level} mode {VV.MODE_NAMES[mode]} shade {shade}")
    finally:
        ctx.close()


def test_view_equals_pick_and_permutation(gpu_ready, oracle_mod):
    """hit4 of the view equals hit4 of the pick on rays built on the host from the same camera,
    in every bit; a fixed permutation of the list gives the permuted records."""
    n = 16
    w, h = shadow_ref.FRAMES[n]
    ctx = _ctx(n)
    try:
        for name, cam in VV.cameras().items():
            org, d = VV.view_rays(cam, w, h)
            for level, mode, solid in ((0, VV.ALBEDO, VV.OCCUPANCY), (0, VV.RADIANCE, VV.ALPHA), (2, VV.MODE_ALPHA, VV.ALPHA)):
                v = _view(ctx, cam, w, h, level, mode, 1)
                p, cells = _pick(ctx, org, d, INF, level, solid)
                _same_records(p, v["hit4"], f"{name} level {level}")
                assert cells == v["cells"]
                perm = np.random.default_rng(5).permutation(w * h)
                q, cells_q = _pick(ctx, org[perm], d[perm], INF, level, solid)
                _same_records(q, p[perm], f"{name} level {level} permuted")
                assert cells_q == cells
    finally:
        ctx.close()


# ---- hostile and hand-written rays -----------------------------------------------------------------
def test_hostile_rays(gpu_ready, oracle_mod):
    """The hostile list, and the hostile direction catalogue (legal and illegal) from origins
    inside the grid, with limits, over a NaN-filled output: every record is written."""
    n = 16
    c = lights_ref.cornell(n)
    names, org, d, lim = VV.hostile_rays(n, c["g0"], c["E"])
    q, v = inside_rays(n)
    bad = np.array([e.d for e in LI.illegal_directions()], F)
    hh = F(c["E"]) / F(n)
    org2 = (np.asarray(c["g0"], F) + np.concatenate([q, q[:bad.shape[0]]]) * hh).astype(F)
    d2 = np.concatenate([v, bad])
    lim2 = np.where(np.arange(org2.shape[0]) % 3 == 0, F(2.75), INF).astype(F)
    org, d, lim = np.concatenate([org, org2]), np.concatenate([d, d2]), np.concatenate([lim, lim2])
    ctx = _ctx(n)
    try:
        for level, solid in ((0, VV.OCCUPANCY), (0, VV.ALPHA), (1, VV.ALPHA), (3, VV.ALPHA)):
            ref = VV.pick(n, c["g0"], c["E"], _solid(n, True, level, solid), level, org, d, lim)
            got, cells = _pick(ctx, org, d, lim, level, solid)
            _same_records(got, ref["hit4"], f"level {level} solid {solid}")
            assert cells == int(ref["steps"].sum())
            assert not (got == NAN_FILL).all(-1).any()
    finally:
        ctx.close()


def test_hand_written_rays(gpu_ready):
    """tests/test_voxview.py's hand grid as an uploaded level 0 (no voxelization): the records
    written out by hand there, from the kernel."""
    import torch
    from vct import Context
    solid = hand_grid()
    r0 = np.zeros((8, 8, 8, 4), F)
    r0[solid] = (0.25, 0.5, 0.75, 0.5)
    ctx = Context(8, (0.0, 0.0, 0.0), 8.0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.upload_level0(r0)
        org = np.array([r[1] for r in HAND], F)
        d = np.array([r[2] for r in HAND], F)
        lim = np.array([r[3] for r in HAND], F)
        ref = VV.pick(8, (0.0, 0.0, 0.0), 8.0, solid, 0, org, d, lim)
        got, cells = _pick(ctx, org, d, lim, 0, VV.ALPHA)
        _same_records(got, ref["hit4"], "hand-written")
        assert cells == int(ref["steps"].sum())
        for k, (name, _, _, _, cell, face, steps, t) in enumerate(HAND):
            assert tuple(int(x) for x in got[k][:3]) == (cell, face, steps), name
            if t is not None:
                assert int(got[k][3]) == f32bits(t), name
        # K1's state is missing: the occupancy source is VCT_ESTATE, the alpha source at a level >= 1 too
        from vct import VctError
        for level, sol in ((0, VV.OCCUPANCY), (1, VV.ALPHA)):
            with pytest.raises(VctError) as e:
                _pick(ctx, org, d, lim, level, sol)
            assert e.value.status == ESTATE
    finally:
        ctx.close()


# ---- n = 64: the longest walks ---------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 3])
def test_long_walks(gpu_ready, oracle_mod, level):
    n = 64
    c = lights_ref.cornell(n)
    w, h = shadow_ref.FRAMES[n]
    cam = VV.cameras()["oblique"]
    ref = VV.view(n, c["g0"], c["E"], cam, w, h, level, VV.RADIANCE, 1, pyr=query_ref.cornell_pyramid(n, True), aniso=True)
    assert int(ref["res"]["steps"].max()) >= (n >> level)
    ctx = _ctx(n)
    try:
        _same_view(_view(ctx, cam, w, h, level, VV.RADIANCE, 1), ref, f"n = 64 level {level}")
    finally:
        ctx.close()


# ---- the dynamic layer, and K1's planes before any inject ------------------------------------------
def test_dynamic_layer_and_voxelize_alone(gpu_ready, oracle_mod):
    """ALBEDO and NORMAL need a voxelization only; after vct_voxelize_dynamic moves a box the
    ALBEDO view is the reference's on the voxels of the concatenated mesh."""
    import torch
    from vct import Context, VctError, scenes
    n = 16
    g0, E = scenes.grid_for_unit_box(n)
    w, h = shadow_ref.FRAMES[n]
    cam = VV.cameras()["inside"]
    ctx = Context(n, g0, E)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.voxelize(*D.static_arrays())
        ref = D.reference(n, D.layers()["empty"])
        for mode in (VV.ALBEDO, VV.NORMAL):
            want = VV.view(n, g0, E, cam, w, h, 0, mode, 1, albedo_occ=ref["albedo_occ"], normal=ref["normal"])
            _same_view(_view(ctx, cam, w, h, 0, mode, 1), want, f"voxelize alone, mode {mode}")
        with pytest.raises(VctError) as e:                      # no level 0 yet
            _view(ctx, cam, w, h, 0, VV.RADIANCE, 0)
        assert e.value.status == ESTATE
        cam = VV.cameras()["outside"]                           # looks through the open front at both boxes
        views = {"static": _view(ctx, cam, w, h, 0, VV.ALBEDO, 0)}
        for name in ("air", "floor"):                           # the box appears, then moves
            ctx.voxelize_dynamic(*D.layers()[name])
            ref = D.reference(n, D.layers()[name])
            want = VV.view(n, g0, E, cam, w, h, 0, VV.ALBEDO, 0, albedo_occ=ref["albedo_occ"], normal=ref["normal"])
            views[name] = _view(ctx, cam, w, h, 0, VV.ALBEDO, 0)
            _same_view(views[name], want, f"dynamic layer {name}")
        assert not np.array_equal(views["air"]["hit4"], views["floor"]["hit4"])
        assert not np.array_equal(views["air"]["hit4"], views["static"]["hit4"])
        assert not np.array_equal(views["floor"]["hit4"], views["static"]["hit4"])
    finally:
        ctx.close()


# ---- statuses --------------------------------------------------------------------------------------
def test_statuses(gpu_ready, oracle_mod):
    """Every VCT_EINVAL case leaves its buffers untouched; every VCT_ESTATE case of the table;
    NULL optional outputs; count = 0."""
    import torch
    from vct import Context, VctError
    from vct.camera import Camera
    n = 16
    c = lights_ref.cornell(n)
    w, h = 16, 8
    cam = VV.cameras()["outside"]
    ctx = _ctx(n)
    lin = torch.full((h, w, 4), float("nan"), device="cuda")
    q = torch.full((h, w), NAN_FILL, dtype=torch.int32, device="cuda")
    hit = torch.full((h * w + 1, 4), NAN_FILL, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    ray = torch.zeros((h * w + 1, 4), device="cuda")
    ray[:, 2] = -1.0

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(lin).all()) and bool((q == NAN_FILL).all()) and bool((hit == NAN_FILL).all()) \
            and int(cnt.sum().item()) == 0

    def refused(status, fn, *a, **kw):
        with pytest.raises(VctError) as e:
            fn(*a, **kw)
        assert e.value.status == status, e.value
        assert untouched()

    try:
        V, P = ctx.voxel_view_device, ctx.voxel_pick_device
        off4 = lin.data_ptr() + 4
        # the view's EINVAL cases
        bad_cam = Camera((0.0, 0.0, 4.0))
        bad_cam.front = bad_cam.front * 1.01
        nan_cam = Camera((float("nan"), 0.0, 4.0))
        zoom_cam = Camera((0.0, 0.0, 4.0))
        zoom_cam.zoom = 179.5
        far_cam = Camera((0.0, 0.0, 4.0))
        far_cam.near, far_cam.far = 2.0, 1.0
        for bc in (bad_cam, nan_cam, zoom_cam, far_cam):
            refused(EINVAL, V, bc, w, h, 0, VV.RADIANCE, 0, lin, q, hit, cnt)
        refused(EINVAL, V, cam, w, h, 0, VV.RADIANCE, 0, None, None, None, cnt)            # every output NULL
        refused(EINVAL, V, cam, 0, h, 0, VV.RADIANCE, 0, lin, q, hit, cnt)
        refused(EINVAL, V, cam, w, 0, 0, VV.RADIANCE, 0, lin, q, hit, cnt)
        refused(EINVAL, V, cam, w, h, 5, VV.RADIANCE, 0, lin, q, hit, cnt)                 # level > L
        refused(EINVAL, V, cam, w, h, 0, 4, 0, lin, q, hit, cnt)                           # mode outside the table
        refused(EINVAL, V, cam, w, h, 1, VV.ALBEDO, 0, lin, q, hit, cnt)                   # occupancy above level 0
        refused(EINVAL, V, cam, w, h, 1, VV.NORMAL, 0, lin, q, hit, cnt)
        refused(EINVAL, V, cam, w, h, 0, VV.RADIANCE, 0, off4, q, hit, cnt)                # misaligned
        refused(EINVAL, V, cam, w, h, 0, VV.RADIANCE, 0, lin, q.data_ptr() + 2, hit, cnt)
        refused(EINVAL, V, cam, w, h, 0, VV.RADIANCE, 0, lin, q, hit.data_ptr() + 8, cnt)
        refused(EINVAL, V, cam, w, h, 0, VV.RADIANCE, 0, lin, q, hit, cnt.data_ptr() + 4)
        # the pick's
        R = h * w
        refused(EINVAL, P, None, ray, R, hit)
        refused(EINVAL, P, ray, None, R, hit)
        refused(EINVAL, P, ray, ray, R, None)
        refused(EINVAL, P, ray.data_ptr() + 4, ray, R, hit)
        refused(EINVAL, P, ray, ray.data_ptr() + 8, R, hit)
        refused(EINVAL, P, ray, ray, R, hit.data_ptr() + 4)
        refused(EINVAL, P, ray, ray, R, hit, 0, VV.OCCUPANCY, cnt.data_ptr() + 4)
        refused(EINVAL, P, ray, ray, R, hit, 5, VV.ALPHA)
        refused(EINVAL, P, ray, ray, R, hit, 0, 2)
        refused(EINVAL, P, ray, ray, R, hit, 1, VV.OCCUPANCY)
        # count = 0 is VCT_OK and writes nothing
        P(ray, ray, 0, hit, 0, VV.ALPHA, cnt)
        assert untouched()
        # NULL optional outputs: each output alone equals the full call's
        full = _view(ctx, cam, w, h, 2, VV.RADIANCE, 1)
        V(cam, w, h, 2, VV.RADIANCE, 1, lin, None, None, None)
        V(cam, w, h, 2, VV.RADIANCE, 1, None, q, None, None)
        V(cam, w, h, 2, VV.RADIANCE, 1, None, None, hit, None)
        torch.cuda.synchronize()
        assert lights_ref.bits_equal(lin.cpu().numpy(), full["linear4"])
        assert np.array_equal(q.cpu().numpy().view(np.uint32), full["rgba8"])
        assert np.array_equal(hit.cpu().numpy().view(np.uint32)[:R].reshape(h, w, 4), full["hit4"])
        assert int(cnt.sum().item()) == 0
        lin.fill_(float("nan")); q.fill_(NAN_FILL); hit.fill_(NAN_FILL)
        # ESTATE: a new level 0 without mips leaves level 0 viewable, the levels above not
        ctx.inject_lights(c["lights"])
        refused(ESTATE, V, cam, w, h, 1, VV.RADIANCE, 0, lin, q, hit, cnt)
        refused(ESTATE, V, cam, w, h, 3, VV.MODE_ALPHA, 0, lin, q, hit, cnt)
        refused(ESTATE, P, ray, ray, R, hit, 2, VV.ALPHA)
        V(cam, w, h, 0, VV.RADIANCE, 0, lin, q, hit[:R], cnt)
        torch.cuda.synchronize()
        assert not untouched()
        lin.fill_(float("nan")); q.fill_(NAN_FILL); hit.fill_(NAN_FILL); cnt.zero_()
    finally:
        ctx.close()
    # ESTATE: nothing voxelized, nothing injected
    ctx = Context(n, c["g0"], c["E"])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        for level, mode in ((0, VV.RADIANCE), (0, VV.MODE_ALPHA), (0, VV.ALBEDO), (0, VV.NORMAL), (2, VV.RADIANCE)):
            refused(ESTATE, ctx.voxel_view_device, cam, w, h, level, mode, 0, lin, q, hit, cnt)
        for level, sol in ((0, VV.OCCUPANCY), (0, VV.ALPHA), (1, VV.ALPHA)):
            refused(ESTATE, ctx.voxel_pick_device, ray, ray, h * w, hit, level, sol)
        # a voxelization alone: the occupancy source works, the alpha source does not
        ctx.voxelize(*c["arrays"])
        refused(ESTATE, ctx.voxel_pick_device, ray, ray, h * w, hit, 0, VV.ALPHA)
        refused(ESTATE, ctx.voxel_view_device, cam, w, h, 0, VV.RADIANCE, 0, lin, q, hit, cnt)
        ctx.voxel_pick_device(ray, ray, h * w, hit, 0, VV.OCCUPANCY)
        torch.cuda.synchronize()
        assert not bool((hit[:h * w] == NAN_FILL).any())
    finally:
        ctx.close()


def test_python_helpers(gpu_ready, oracle_mod):
    """vct.voxview.view / pick return the calls' tensors."""
    from vct import voxview
    n = 16
    c = lights_ref.cornell(n)
    w, h = shadow_ref.FRAMES[n]
    cam = VV.cameras()["oblique"]
    ctx = _ctx(n)
    try:
        ref = VV.view(n, c["g0"], c["E"], cam, w, h, 1, VV.RADIANCE, 1, pyr=query_ref.cornell_pyramid(n, True), aniso=True)
        got = voxview.view(ctx, cam, w, h, level=1, mode="radiance", shade=True)
        assert lights_ref.bits_equal(got["linear"].cpu().numpy(), ref["linear4"]) and got["cells"] == ref["cells"]
        org, d = VV.view_rays(cam, w, h)
        p = voxview.pick(ctx, org, d, level=1, solid="alpha", count_cells=True)
        _same_records(p["record"].cpu().numpy().view(np.uint32), ref["hit4"], "voxview.pick")
        assert p["cells"] == ref["cells"]
        assert np.array_equal(p["hit"].cpu().numpy(), ref["res"]["hit"])
        assert lights_ref.bits_equal(p["t"].cpu().numpy(), ref["res"]["t"])
    finally:
        ctx.close()


# ---- the host ------------------------------------------------------------------------------------
def _read_png_rgb(path):
    """The host's encoder writes 8-bit RGB, filter None, one IDAT: -> [h, w, 3] uint8."""
    import struct
    import zlib
    with open(path, "rb") as f:
        b = f.read()
    assert b[:8] == bytes([137, 80, 78, 71, 13, 10, 26, 10])
    at, idat, w, h = 8, b"", 0, 0
    while at < len(b):
        n, typ = struct.unpack(">I4s", b[at:at + 8])
        data = b[at + 8:at + 8 + n]
        assert zlib.crc32(typ + data) == struct.unpack(">I", b[at + 8 + n:at + 12 + n])[0]
        if typ == b"IHDR":
            w, h, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", data)
            assert (depth, colour, interlace) == (8, 2, 0)
        elif typ == b"IDAT":
            idat += data
        at += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3)


def test_cpp_host_voxels_flag(gpu_ready, tmp_path):
    """vct_headless --voxels LEVEL[:MODE] writes the voxel view of the frame's camera as a PNG next
    to the frame: the same cells as the Python view from the same camera (the host's float32 GLM
    camera differs from vct.camera.Camera in the last bits, so silhouette pixels may differ)."""
    import os
    import subprocess
    import torch
    from helpers import write_obj
    from vct import Context, scenes, voxview
    from vct.camera import Camera
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "voxel-based-global-illumination_amd", "build", "vct_headless")
    assert os.path.exists(exe), "build the host with `make -C voxel-based-global-illumination_amd host`"
    s = scenes.cornell()
    obj = write_obj(s, str(tmp_path))
    n, w, h = 32, 96, 64
    ppm = str(tmp_path / "frame.ppm")
    p = subprocess.run([exe, obj, str(n), str(w), str(h), "1", ppm, "--model=identity", "--grid=unit",
                        "--voxels", "0", "--voxels=3:alpha", "--voxels", "0:albedo"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    g0, E = scenes.grid_for_unit_box(n)
    ctx = Context(n, g0, E)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        ctx.voxelize(*s.arrays())
        ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
        ctx.build_mips()
        for level, mode in ((0, "radiance"), (3, "alpha"), (0, "albedo")):
            png = str(tmp_path / f"frame.voxels{level}-{mode}.png")
            assert f"wrote {png}" in p.stdout
            img = _read_png_rgb(png)
            assert img.shape == (h, w, 3)
            ref = voxview.view(ctx, Camera(), w, h, level=level, mode=mode, shade=True)["rgba8"].cpu().numpy().view(np.uint32)
            want = np.stack([(ref >> (8 * k)) & 255 for k in range(3)], axis=-1).astype(np.int16)
            hit = (ref >> 24) == 255
            assert 0.2 < hit.mean() < 1.0
            close = (np.abs(img.astype(np.int16) - want) <= 1).all(-1)
            assert close.mean() >= 0.97, (level, mode, close.mean())
            assert len(np.unique(img.reshape(-1, 3), axis=0)) >= 4
    finally:
        ctx.close()
    bad = subprocess.run([exe, obj, "--voxels", "1:albedo"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "malformed --voxels" in bad.stderr
    deep = subprocess.run([exe, obj, str(n), str(w), str(h), "1", ppm, "--model=identity", "--grid=unit", "--voxels", "9"],
                          capture_output=True, text=True, timeout=120)
    assert deep.returncode == 1 and "level above L" in deep.stderr
