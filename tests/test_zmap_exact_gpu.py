"""K4's exact empty-space test: maps D_0..D_zm_levels (Grid::zmap) against their definition,
and frames traced with them against the oracle, the coarse test (VCT_ZMAP_EXACT=0) and no
test at all (VCT_ZMAP=0).

D_m, bit of padded position P (p = P - 1 in [-1, n_m - 1]^3): OR over the level-m texels
p + {0,1}^3 of "some level-0 descendant is not +0 by bit pattern"; texels outside the level
are zero.  A level-l trilinear footprint at corner c is the texels c + {0,1}^3, so the
kernel reads D_l at c + 1 (exact) or D_{l+1} at (c >> 1) + 1 (coarse).  Every comparison
here is bit for bit.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import bounce_ref
from helpers import gpu_pipeline, gpu_pyramid_flat

pytestmark = pytest.mark.gpu

GRIDS = [16, 32, 64]          # zm_levels = 2, 3, 4
W, H = 96, 64
EYE = (0.5, 0.6, 2.5)
KEYS = ("diffuse", "spec", "steps_px")
# default, forced union, forced occupancy, reordered
VARIANTS = (0, 0x1000000, 0x2000000, 0x8000)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _level0(n):
    """The adversarial level 0 of test_parity_gpu.test_empty_space_maps_exact: sparse signed
    values, -0.0, denormals, colour with alpha 0."""
    rng = np.random.default_rng(17 + n)
    occ = rng.random((n, n, n)) < 0.02
    r0 = np.zeros((n, n, n, 4), np.float32)
    r0[occ] = rng.standard_normal((int(occ.sum()), 4)).astype(np.float32)
    free = np.argwhere(~occ)
    pick = free[rng.choice(len(free), 60, replace=False)]
    r0[tuple(pick[:20].T)] = -0.0                                   # negative zero: not +0
    r0[tuple(pick[20:40].T)] = np.float32(1e-40)                    # denormal
    r0[tuple(pick[40:].T)] = np.array([0.5, -0.25, 0.125, 0.0], np.float32)   # colour with alpha 0
    r0.setflags(write=False)
    return r0


@functools.lru_cache(maxsize=None)
def _gbuffer(n):
    """Random surface points, normals and roughness; rows 0..23 hold points within one voxel
    of each grid face (two rows per face and normal sign), with the normal along the face's
    axis pointing in / out (rows 0..11) or tilted off it (rows 12..23): the cone origins
    P / h + n then reach corners -1 and n - 1."""
    rng = np.random.default_rng(29 + n)
    pos = np.zeros((H, W, 4), np.float32)
    pos[..., :3] = rng.uniform(0.05, 0.95, (H, W, 3))
    pos[..., 3] = (rng.random((H, W)) < 0.9).astype(np.float32)
    nv = rng.standard_normal((H, W, 3))
    nv /= np.linalg.norm(nv, axis=-1, keepdims=True)
    row = 0
    for tilt in (0.0, 0.35):
        for axis in range(3):
            for side in (0, 1):
                for sign in (-1.0, 1.0):
                    p = rng.uniform(0.0, 1.0, (W, 3))
                    d = rng.uniform(0.0, 1.0 / n, W)
                    d[:4] = (0.0, 1.0 / n, 0.5 / n, 1e-7)
                    p[:, axis] = d if side == 0 else 1.0 - d
                    v = tilt * rng.standard_normal((W, 3))
                    v[:, axis] = sign
                    pos[row, :, :3] = p
                    pos[row, :, 3] = 1.0
                    nv[row] = v / np.linalg.norm(v, axis=-1, keepdims=True)
                    row += 1
    assert row == 24
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., :3] = nv
    alb = np.zeros((H, W, 4), np.float32)
    alb[..., :3] = rng.random((H, W, 3))
    alb[..., 3] = rng.uniform(0.0, 1.0, (H, W))
    for a in (pos, nrm, alb):
        a.setflags(write=False)
    return pos, nrm, alb


def _maps_ref(r0, levels):
    """numpy restatement of D_0..D_levels: {m: uint32 [dim, dim, rw]}."""
    n = r0.shape[0]
    occ = (_bits(r0) != 0).any(axis=-1)                      # [z, y, x]: not +0 by bit pattern
    out = {}
    for m in range(levels + 1):
        nm = n >> m
        o = occ.reshape(nm, 1 << m, nm, 1 << m, nm, 1 << m).any(axis=(1, 3, 5))
        pad = np.zeros((nm + 2,) * 3, bool)
        pad[1:-1, 1:-1, 1:-1] = o
        dim = nm + 1
        d = np.zeros((dim,) * 3, bool)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    d |= pad[dz:dz + dim, dy:dy + dim, dx:dx + dim]
        rw = (dim + 31) // 32
        row = np.zeros((dim, dim, rw * 32), np.uint64)
        row[..., :dim] = d
        sh = (np.arange(rw * 32, dtype=np.uint64) % np.uint64(32))
        out[m] = (row << sh).reshape(dim, dim, rw, 32).sum(axis=-1).astype(np.uint32)
    return out


def _check_maps(ctx, r0, what):
    from vct import _lib
    levels = int(np.log2(r0.shape[0])) - 2
    levels = min(levels, 5)
    ref = _maps_ref(r0, levels)
    for m in range(levels + 1):
        got = _lib.debug_zmap(ctx.lib, ctx.h, m)
        assert got is not None, f"{what}: no map {m}"
        assert got.shape == ref[m].shape, (what, m, got.shape, ref[m].shape)
        dim, rw = got.shape[1], got.shape[2]
        spare = rw * 32 - dim
        if spare:                                            # spare bits of a row's last dword
            assert not (got[..., -1] >> np.uint32(32 - spare)).any(), f"{what}: map {m} spare bits"
        assert np.array_equal(got, ref[m]), f"{what}: map {m} differs in {int((got != ref[m]).sum())} dwords"
    assert _lib.debug_zmap(ctx.lib, ctx.h, levels + 1) is None


@pytest.mark.parametrize("n", GRIDS)
def test_maps_equal_definition(gpu_ready, n, monkeypatch):
    from vct import Context, _lib
    monkeypatch.delenv("VCT_ZMAP", raising=False)
    monkeypatch.delenv("VCT_ZMAP_EXACT", raising=False)
    r0 = _level0(n)
    ctx = Context(n, (0, 0, 0), 1.0)
    ctx.upload_level0(r0)
    ctx.build_mips()
    _check_maps(ctx, r0, f"n = {n}")
    # a second, different level 0 through the same context: every map follows it
    r1 = np.ascontiguousarray(r0[::-1, :, ::-1])
    ctx.upload_level0(r1)
    assert _lib.debug_zmap(ctx.lib, ctx.h, 0) is None       # the upload invalidates the maps
    ctx.build_mips()
    _check_maps(ctx, r1, f"n = {n}, second level 0")
    # the coarse test reads the same maps
    monkeypatch.setenv("VCT_ZMAP_EXACT", "0")
    ctx.build_mips()
    _check_maps(ctx, r1, f"n = {n}, VCT_ZMAP_EXACT=0")
    monkeypatch.setenv("VCT_ZMAP", "0")
    ctx.build_mips()
    assert _lib.debug_zmap(ctx.lib, ctx.h, 0) is None
    ctx.close()


def test_maps_of_a_voxelized_scene(gpu_ready, monkeypatch):
    """K2's level 0 (n = 64: the one-launch map build with live blocks), then a relight
    build, which skips the maps: they still describe the level-0 pattern."""
    from vct import scenes
    monkeypatch.delenv("VCT_ZMAP", raising=False)
    monkeypatch.delenv("VCT_ZMAP_EXACT", raising=False)
    ctx, _, _, _ = gpu_pipeline(64, "atrium")
    _check_maps(ctx, ctx.download_level(0), "atrium 64")
    ctx.inject_directional((-0.4, 1.0, 0.3), scenes.LIGHT_COLOR)
    ctx.build_mips()
    _check_maps(ctx, ctx.download_level(0), "atrium 64, relit")
    ctx.close()


def _frames(ctx, gb, dev):
    """Every form of every variant: the counting form (per-pixel steps and the step total),
    the counter-free form, and the counting form without counters (0x4000)."""
    import torch
    out = {}
    for variant in VARIANTS:
        d, sp = (torch.full((H, W, 4), -1.0, device=dev) for _ in range(2))
        st = torch.zeros((H, W), dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        ctx.trace_device(*gb, W, H, EYE, d, sp, steps_px=st, cone_steps=cnt, variant=variant)
        torch.cuda.synchronize()
        out[(variant, "counting")] = {"diffuse": d.cpu().numpy(), "spec": sp.cpu().numpy(),
                                      "steps_px": st.cpu().numpy().astype(np.uint32), "cone_steps": int(cnt[0])}
        for extra, name in ((0, "counter-free"), (0x4000, "0x4000")):
            d, sp = (torch.full((H, W, 4), -1.0, device=dev) for _ in range(2))
            ctx.trace_device(*gb, W, H, EYE, d, sp, variant=variant | extra)
            torch.cuda.synchronize()
            out[(variant, name)] = {"diffuse": d.cpu().numpy(), "spec": sp.cpu().numpy()}
    return out


@pytest.mark.parametrize("n", GRIDS)
def test_trace_parity(gpu_ready, oracle_mod, n, monkeypatch):
    import torch
    from vct import Context, _lib
    monkeypatch.delenv("VCT_ZMAP", raising=False)
    monkeypatch.delenv("VCT_ZMAP_EXACT", raising=False)
    r0 = _level0(n)
    pos, nrm, alb = _gbuffer(n)
    ctx = Context(n, (0, 0, 0), 1.0)
    ctx.upload_level0(r0)
    ctx.build_mips()
    assert _lib.debug_zmap(ctx.lib, ctx.h, 0) is not None
    ref = oracle_mod.trace(n, (0, 0, 0), 1.0, r0, gpu_pyramid_flat(ctx), pos, nrm, alb, EYE)
    assert ref["steps_px"][:24].any() and _bits(ref["diffuse"][:24]).any()   # the face rows do march and see light
    dev = torch.device("cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    gb = [torch.from_numpy(np.array(a)).to(dev) for a in (pos, nrm, alb)]
    exact = _frames(ctx, gb, dev)
    for form, f in exact.items():
        for key in KEYS:
            if key in f:
                assert np.array_equal(_bits(f[key]), _bits(ref[key])), f"exact maps, {form}: {key} vs the oracle"
        if "cone_steps" in f:
            assert f["cone_steps"] == ref["cone_steps"], form
    for env, what in (("VCT_ZMAP_EXACT", "coarse maps"), ("VCT_ZMAP", "no maps")):
        monkeypatch.setenv(env, "0")
        ctx.build_mips()
        assert (_lib.debug_zmap(ctx.lib, ctx.h, 0) is None) == (env == "VCT_ZMAP")
        other = _frames(ctx, gb, dev)
        for form, f in other.items():
            for key, a in f.items():
                b = exact[form][key]
                same = a == b if key == "cone_steps" else np.array_equal(_bits(a), _bits(b))
                assert same, f"{what}, {form}: {key} differs from the frame traced with the exact maps"
    ctx.close()


def test_bounce_equals_reference(gpu_ready, oracle_mod, monkeypatch):
    """One vct_inject_bounces bounce at n = 32 (the gather is K4 with the maps), as in
    test_bounce_gpu; the maps then describe the bounced level 0."""
    from vct import Context, scenes
    monkeypatch.delenv("VCT_ZMAP", raising=False)
    monkeypatch.delenv("VCT_ZMAP_EXACT", raising=False)
    n = 32
    ref = bounce_ref.cornell(n, True, 9, 2)
    ctx = Context(n, ref["g0"], ref["E"], aniso=True, n_diffuse=9, specular=True)
    ctx.voxelize(*ref["arrays"])
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    ctx.build_mips()
    _check_maps(ctx, ctx.download_level(0), "before the bounce")
    ctx.inject_bounces(1)
    want = ref["bounces"][1]
    assert bounce_ref.bits_equal(ctx.download_level(0), want["level0"]), "level 0 after 1 bounce"
    assert bounce_ref.pyramid_equal(ctx, want["pyr"]), "pyramid after 1 bounce"
    _check_maps(ctx, want["level0"], "after the bounce")
    ctx.close()


def test_exact_maps_skip_more(gpu_ready, monkeypatch):
    """Debug-counter build, atrium 64 at 192 x 128, forced forms in screen order (the same
    launch every time): with the exact maps, counter 32 (level-A misses skipped as empty)
    does not fall and counter 4 (level-0 gathers) does not rise against VCT_ZMAP_EXACT=0.
    No timing."""
    import torch
    from vct import Context, _lib, scenes
    from vct.camera import Camera
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvct_hip_dbg.so")
    if not os.path.exists(path):
        pytest.skip("no debug-counter library (make -C voxel-based-global-illumination_amd dbg)")
    lib = _lib.bind(C.CDLL(path))
    lib.vct_debug_counters.restype = C.c_int
    lib.vct_debug_counters.argtypes = [C.c_void_p, C.c_int]
    monkeypatch.delenv("VCT_ZMAP", raising=False)
    n, w, h = 64, 192, 128
    g0, E = scenes.grid_for_unit_box(n)
    ctx = Context(n, g0, E, lib=lib)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.voxelize(*scenes.SCENES["atrium"]().arrays())
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    dev = torch.device("cuda")
    cam = Camera()
    gb = [torch.empty((h, w, 4), device=dev) for _ in range(3)]
    d, sp = torch.empty((h, w, 4), device=dev), torch.empty((h, w, 4), device=dev)
    ctr = (C.c_ulonglong * 56)()
    counts, frames = {}, {}
    for exact in ("1", "0"):
        monkeypatch.setenv("VCT_ZMAP_EXACT", exact)
        ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
        ctx.build_mips()
        if exact == "1":
            ctx.gbuffer_raster_device(cam, w, h, scenes.ROUGHNESS, *gb)
        for variant in (0x5000000, 0x6000000):
            torch.cuda.synchronize()
            assert lib.vct_debug_counters(ctr, 1) == 0
            ctx.trace_device(*gb, w, h, cam.position, d, sp, variant=variant)
            torch.cuda.synchronize()
            assert lib.vct_debug_counters(ctr, 1) == 0
            c = list(ctr)
            # vct_debug_counters: counters 0..31, eight clocks, counters 32..47
            counts[(exact, variant)] = {"skipped": c[40], "gathers0": c[4], "wave_steps": c[44] + c[46]}
            frames[(exact, variant)] = (d.cpu().numpy(), sp.cpu().numpy())
    for variant in (0x5000000, 0x6000000):
        e, o = counts[("1", variant)], counts[("0", variant)]
        print(f"variant {variant:#x}: exact {e}, coarse {o}")
        assert e["wave_steps"] == o["wave_steps"] > 0
        assert o["skipped"] > 0, "the coarse test skipped nothing: the counters are not live"
        assert e["skipped"] >= o["skipped"], (variant, e, o)
        assert e["gathers0"] <= o["gathers0"], (variant, e, o)
        for a, b in zip(frames[("1", variant)], frames[("0", variant)]):
            assert np.array_equal(_bits(a), _bits(b))
    ctx.close()
