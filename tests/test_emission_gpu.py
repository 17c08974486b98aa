"""include/vct_emission.h on the GPU against tests/emission_ref.py (a composition of CPU-oracle
calls and a numpy restatement of vct_spec.h "emissive surfaces").  Every comparison is
bit-exact: the sums are integers (no arrival order), and the float steps are the spec's, in
the spec's order.
"""
import ctypes as C

import numpy as np
import pytest

import bounce_ref
import emission_ref as R
import lights_ref
import shadow_ref
import test_emission as T
from emission_ref import bits_equal

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 5
F = np.float32


def _ctx(n, g0, E, arrays, **kw):
    import torch
    from vct import Context
    ctx = Context(n, g0, E, **kw)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.voxelize(*arrays)
    return ctx


def _lamp_ctx(n, emit=True, **kw):
    L = R.lamp(n)
    ctx = _ctx(n, L["g0"], L["E"], L["arrays"], **kw)
    if emit:
        v, i, m, _ = L["arrays"]
        ctx.voxelize_emission(v, i, m, L["ke"])
    return ctx


def _emit(ctx, form, verts, idx, mat, ke):
    """vct_voxelize_emission in its host or its device form."""
    import torch
    if form == "host":
        ctx.voxelize_emission(verts, idx, mat, ke)
        return
    dev = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()
    ctx.voxelize_emission_device(dev(np.asarray(verts, F), F), dev(np.asarray(idx, np.uint32), np.int32),
                                 dev(None if mat is None else np.asarray(mat, np.uint32), np.int32),
                                 dev(np.asarray(ke, F), F))


def _assert_emission(ctx, em, what):
    got = ctx.download_emission()
    assert bits_equal(got, em["E"]), f"{what}: {int((got.view(np.uint32) != em['E'].view(np.uint32)).any(-1).sum())} voxels differ"
    assert ctx.emission_voxels() == int(em["emissive"].sum()), what


def _assert_grid(ctx, oracle_mod, n, level0, what):
    assert bits_equal(ctx.download_level(0), level0), f"{what}: level 0"
    assert bounce_ref.pyramid_equal(ctx, oracle_mod.build_mips(n, level0, True)), f"{what}: pyramid"


# ---- 1. the emission grid ------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("n", [16, 32, 64])
def test_lamp_grid_equals_reference(gpu_ready, oracle_mod, n, form):
    """16: rows shorter than a wave, four rows per bitmask word; 64: full 64-bit rows, two lamp layers."""
    L = R.lamp(n)
    assert L["classes"]["emissive"] == T.LAMP[n]["emissive"]
    ctx = _lamp_ctx(n, emit=False)
    assert ctx.emission_voxels() == 0 and not ctx.download_emission().view(np.uint32).any()   # never built: empty
    v, i, m, _ = L["arrays"]
    _emit(ctx, form, v, i, m, L["ke"])
    _assert_emission(ctx, L["em"], f"lamp {n} {form}")
    sums, counts = ctx.download_accum()                                   # K1's state is untouched
    assert np.array_equal(counts, L["grid"]["counts"]) and np.array_equal(sums, L["grid"]["sums"])
    ctx.close()


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("n", [32, 64])
def test_giant_triangles(gpu_ready, oracle_mod, n, form):
    """Material 0's wall-sized triangles emit: one triangle's candidates over many lanes and bucket starts."""
    arrays, ke, counts, g0, E = T.giant_case(n)
    em = R.emission(oracle_mod, n, g0, E, counts, arrays[0], arrays[1], arrays[2], ke)
    assert int(em["emissive"].sum()) == T.GIANT[n]
    ctx = _ctx(n, g0, E, arrays)
    _emit(ctx, form, arrays[0], arrays[1], arrays[2], ke)
    _assert_emission(ctx, em, f"giant {n} {form}")
    ctx.close()


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("n", [16, 32])
def test_random_soup(gpu_ready, oracle_mod, n, form):
    """300 overlapping triangles, three emitting materials of four: contended atomics, mixed voxels."""
    arrays, counts, mat, ke, g0, E = T.soup_case(n, oracle_mod)
    em = R.emission(oracle_mod, n, g0, E, counts, arrays[0], arrays[1], mat, ke)
    assert R.classes(em, counts)["multi"] == T.SOUP[n]["multi"]
    ctx = _ctx(n, g0, E, arrays)
    _emit(ctx, form, arrays[0], arrays[1], mat, ke)
    _assert_emission(ctx, em, f"soup {n} {form}")
    ctx.close()


# ---- 2. emitter geometry that is not (all) part of the voxelized mesh -----------------------
@pytest.mark.parametrize("n", [16, 32])
def test_subset_and_floating_triangle(gpu_ready, oracle_mod, n):
    L = R.lamp(n)
    arrays, counts, emit = T.subset_case(n, oracle_mod)
    em = R.emission(oracle_mod, n, L["g0"], L["E"], counts, *emit)
    assert (int(em["emissive"].sum()), em["dropped"]) == T.SUBSET[n]
    ctx = _ctx(n, L["g0"], L["E"], arrays)
    ctx.voxelize_emission(*emit)
    _assert_emission(ctx, em, f"subset {n}")                              # the hits over the open hole are dropped
    fl = T.floating_case()
    ref = R.emission(oracle_mod, n, L["g0"], L["E"], counts, *fl)
    assert ref["dropped"] == T.FLOATING[n] and not ref["emissive"].any()
    ctx.voxelize_emission(*fl)                                            # tri_material NULL: material 0
    assert ctx.emission_voxels() == 0 and not ctx.download_emission().view(np.uint32).any()
    ctx.inject_lights([])
    before = ctx.download_level(0)
    ctx.inject_emission(1.0)                                              # an empty grid: a no-op that succeeds
    assert bits_equal(ctx.download_level(0), before)
    ctx.close()


# ---- 3. the hostile catalogue ------------------------------------------------------------
@pytest.mark.parametrize("placement", ["exact", "unit"])
@pytest.mark.parametrize("n", [16, 32])
def test_hostile_catalogue(gpu_ready, oracle_mod, n, placement):
    mesh, counts, ke = T.hostile_case(n, placement, oracle_mod)
    em = R.emission(oracle_mod, n, mesh.g0, mesh.E, counts, mesh.verts, mesh.idx, mesh.mat, ke)
    assert int(em["emissive"].sum()) == T.HOSTILE[(n, placement)]
    ctx = _ctx(n, mesh.g0, mesh.E, (mesh.verts, mesh.idx, mesh.mat, mesh.kd))
    assert np.array_equal(ctx.download_accum()[1], counts)
    for form in ("host", "device"):
        _emit(ctx, form, mesh.verts, mesh.idx, mesh.mat, ke)
        _assert_emission(ctx, em, f"hostile {n} {placement} {form}")
    assert np.isfinite(ctx.download_emission()).all()
    ctx.close()


# ---- 4. level 0 and the pyramid ------------------------------------------------------------
def test_level0_and_pyramid(gpu_ready, oracle_mod):
    import vct
    from vct import scenes
    n = 32
    L = R.lamp(n)
    g = L["grid"]
    E_grid = L["em"]["E"]
    lights = lights_ref.light_set_s(n)
    k2 = lambda ls: lights_ref.inject(n, L["g0"], L["E"], g["albedo_occ"], g["normal"], ls)
    ctx = _lamp_ctx(n)
    ctx.inject_lights(lights)
    ctx.inject_emission(1.0)
    ctx.build_mips()
    want = R.add_to_level0(k2(lights), E_grid, 1.0)
    assert not bits_equal(want, k2(lights))
    _assert_grid(ctx, oracle_mod, n, want, "lights + emission")
    other = [vct.point_light((-0.5, 0.3, 0.2), (3.0, 2.0, 1.0), 1.5), lights[2]]
    ctx.inject_lights(other)                                              # the relight build
    ctx.inject_emission(0.5)
    ctx.build_mips()
    _assert_grid(ctx, oracle_mod, n, R.add_to_level0(k2(other), E_grid, 0.5), "relight + 0.5 x emission")
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)           # K2's own kernels
    ctx.inject_emission(2.0)
    ctx.build_mips()
    _assert_grid(ctx, oracle_mod, n, R.add_to_level0(g["r0"], E_grid, 2.0), "K2 + 2 x emission")
    ctx.inject_lights([])                                                  # the closed box, lit by the lamp alone
    ctx.inject_emission(1.0)
    ctx.build_mips()
    only = np.zeros((n, n, n, 4), F)
    only[..., 3] = g["albedo_occ"][..., 3] != 0
    only[L["em"]["emissive"], :3] = E_grid[L["em"]["emissive"], :3]
    _assert_grid(ctx, oracle_mod, n, only, "emission only")
    ctx.upload_level0(k2(other))                                           # a dense level 0 takes it too
    ctx.inject_emission(1.0)
    ctx.build_mips()
    _assert_grid(ctx, oracle_mod, n, R.add_to_level0(k2(other), E_grid, 1.0), "upload + emission")
    ctx.close()


# ---- 5. bounces ------------------------------------------------------------------------------
def test_bounce_carries_the_lamp(gpu_ready, oracle_mod):
    n = 32
    L = R.lamp(n)
    g = L["grid"]
    dark = np.zeros((n, n, n, 4), F)
    dark[..., 3] = g["albedo_occ"][..., 3] != 0
    r0 = R.add_to_level0(dark, L["em"]["E"], 1.0)
    ref = bounce_ref.bounce(oracle_mod, n, L["g0"], L["E"], g["albedo_occ"], g["normal"], r0, 1)
    ctx = _lamp_ctx(n)
    ctx.inject_lights([])
    ctx.inject_emission(1.0)
    ctx.build_mips()
    _assert_grid(ctx, oracle_mod, n, r0, "before the bounce")
    ctx.inject_bounces(1)
    got = ctx.download_level(0)
    assert bits_equal(got, ref[1]["level0"])
    assert bounce_ref.pyramid_equal(ctx, ref[1]["pyr"])
    # the floor (the two lowest occupied layers) sees nothing but the lamp: +0 before, lit after
    floor = np.zeros((n, n, n), bool)
    floor[:, :2, :] = g["albedo_occ"][:, :2, :, 3] != 0
    assert floor.sum() > 500 and not r0[floor, :3].view(np.uint32).any()
    assert (got[floor, :3] > 0).all(axis=-1).sum() > 400
    ctx.close()


# ---- 6. the composite ------------------------------------------------------------------------
def _frame(ctx, w, h, position=(0.0, -0.5, 0.6), pitch=70.0):
    """A ray-cast G-buffer looking up at the lamp (some rays leave through the open front)."""
    import torch
    from vct.camera import Camera
    gb = [torch.empty((h, w, 4), device="cuda") for _ in range(3)]
    ctx.gbuffer_raycast_device(Camera(position=position, pitch=pitch), w, h, 0.1, *gb)
    gen = torch.Generator(device="cpu").manual_seed(3)
    D = torch.rand((h, w, 4), generator=gen).cuda()
    S = (torch.rand((h, w, 4), generator=gen) * 0.2).cuda()
    torch.cuda.synchronize()
    return gb, D, S


def _emissive(ctx, gb, D, S, lights, vis, scale):
    import torch
    h, w = gb[0].shape[:2]
    lin = torch.full((h, w, 4), float("nan"), device="cuda")
    px = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    ctx.composite_emissive_device(*gb, D, S, w, h, lights, vis, scale, out_linear4=lin, out_rgba8=px)
    torch.cuda.synchronize()
    return lin.cpu().numpy(), px.cpu().numpy().view(np.uint32)


def test_composite(gpu_ready, oracle_mod):
    import torch
    n, w, h = 32, 80, 48
    L = R.lamp(n)
    g = L["grid"]
    lights = lights_ref.light_set_s(n)
    ctx = _lamp_ctx(n, emit=False)
    ctx.inject_lights(lights)
    ctx.build_mips()
    gb, D, S = _frame(ctx, w, h)
    pos, nrm, alb = (t.cpu().numpy() for t in gb)
    Dn, Sn = D.cpu().numpy(), S.cpu().numpy()
    Em, hit = R.lookup(n, L["g0"], L["E"], L["em"]["E"], pos)
    fg = pos[..., 3] != 0
    print("pixels in emissive voxels", int(hit.sum()), "in others", int((fg & ~hit).sum()))
    assert hit.sum() >= 50 and (fg & ~hit).sum() >= 50
    assert (~fg).sum() >= 50
    hard = lights_ref.composite(n, L["g0"], L["E"], g["albedo_occ"], pos, nrm, alb, Dn, Sn, lights)
    plain = torch.empty((h, w, 4), device="cuda")
    plain_px = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    ctx.composite_lights_device(*gb, D, S, w, h, lights, out_linear4=plain, out_rgba8=plain_px)
    torch.cuda.synchronize()
    assert bits_equal(plain.cpu().numpy(), hard)
    # an empty emission grid, and scale +0 on a built one: vct_composite_lights_device bit for bit
    lin, px = _emissive(ctx, gb, D, S, lights, None, 1.0)
    assert bits_equal(lin, hard) and np.array_equal(px, plain_px.cpu().numpy().view(np.uint32))
    v, i, m, _ = L["arrays"]
    ctx.voxelize_emission(v, i, m, L["ke"])
    lin, px = _emissive(ctx, gb, D, S, lights, None, 0.0)
    assert bits_equal(lin, hard) and np.array_equal(px, plain_px.cpu().numpy().view(np.uint32))
    # vis = NULL: the walk, plus the term
    for scale in (1.0, 0.25):
        lin, px = _emissive(ctx, gb, D, S, lights, None, scale)
        want = R.composite(hard, pos, Em, scale)
        assert bits_equal(lin, want), scale
        assert not bits_equal(lin[hit], hard[hit]) and bits_equal(lin[~hit], hard[~hit])
    assert np.array_equal(px[~hit], plain_px.cpu().numpy().view(np.uint32)[~hit]) and (px >> 24 == 255).all()
    # a vis plane from the shadow cones
    tan_half = [0.05, 0.2, 0.1, 0.05, 0.3, 0.02, 0.0]
    vis = torch.full((len(lights), h, w), float("nan"), device="cuda")
    ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, tan_half, vis)
    torch.cuda.synchronize()
    soft = shadow_ref.composite(n, L["g0"], L["E"], pos, nrm, alb, Dn, Sn, lights, vis.cpu().numpy())
    assert not bits_equal(soft, hard)
    shadowed = torch.empty((h, w, 4), device="cuda")
    ctx.composite_shadowed_device(*gb, D, S, w, h, lights, vis, out_linear4=shadowed)
    torch.cuda.synchronize()
    assert bits_equal(shadowed.cpu().numpy(), soft)
    lin, _ = _emissive(ctx, gb, D, S, lights, vis, 1.0)
    assert bits_equal(lin, R.composite(soft, pos, Em, 1.0))
    lin, _ = _emissive(ctx, gb, D, S, lights, vis, 0.0)
    assert bits_equal(lin, soft)
    # no lights at all: only the indirect terms and the emitter
    lin, _ = _emissive(ctx, gb, D, S, [], None, 1.0)
    none = lights_ref.composite(n, L["g0"], L["E"], g["albedo_occ"], pos, nrm, alb, Dn, Sn, [])
    assert bits_equal(lin, R.composite(none, pos, Em, 1.0))
    ctx.close()


def test_composite_small_and_hostile_frames(gpu_ready, oracle_mod):
    """A 1 x 1 frame, an all-background frame, and a G-buffer whose positions are outside the
    grid, on its faces, or NaN / Inf (Em = +0 there).  Light set S with its directional light, and
    a second directional light that the frame's normal (0, -1, 0) faces: a receiver with a NaN q
    skips the point and spot lights (r2 > 0 fails), and its hard walk toward a directional light
    gives V = 1 by the shadow-walk receiver rule of vct_spec.h, so every output is a defined number."""
    import torch
    n = 32
    L = R.lamp(n)
    g = L["grid"]
    import vct
    lights = lights_ref.light_set_s(n) + [vct.directional_light((0.3, -1.0, 0.2), (0.5, 0.25, 0.75))]
    assert sum(l.type == 0 for l in lights) == 2
    ctx = _lamp_ctx(n)
    z, y, x = (a[0] for a in np.nonzero(L["em"]["emissive"]))
    hh = F(L["E"]) / F(n)
    inside = [float(F(L["g0"][c]) + (F(v) + F(0.5)) * hh) for c, v in enumerate((x, y, z))]
    top = float(F(L["g0"][1]) + F(L["E"]))
    nan, inf = float("nan"), float("inf")
    rows = [(inside[0], inside[1], inside[2], 1.0), (inside[0], inside[1], inside[2], 0.0),
            (inside[0], top + 0.5, inside[2], 1.0), (inside[0], top, inside[2], 1.0), (-7.0, inside[1], inside[2], 1.0),
            (nan, inside[1], inside[2], 1.0), (inside[0], inf, inside[2], 1.0), (inside[0], inside[1], -inf, 1.0),
            (1e30, 1e30, 1e30, 1.0), (0.1, 0.2, 0.3, 1.0)]
    for w, h, sel in ((1, 1, [0]), (1, 1, [1]), (5, 2, list(range(10))), (3, 1, [1, 1, 1])):
        pos = np.array([rows[k] for k in sel], F).reshape(h, w, 4)
        nrm = np.zeros((h, w, 4), F)
        nrm[..., 1] = -1.0
        alb = np.full((h, w, 4), 0.5, F)
        rng = np.random.default_rng(w * 10 + h)
        Dn, Sn = rng.random((h, w, 4)).astype(F), (rng.random((h, w, 4)) * 0.2).astype(F)
        gb = [torch.from_numpy(a).cuda() for a in (pos, nrm, alb)]
        lin, px = _emissive(ctx, gb, torch.from_numpy(Dn).cuda(), torch.from_numpy(Sn).cuda(), lights, None, 1.5)
        Em, hit = R.lookup(n, L["g0"], L["E"], L["em"]["E"], pos)
        base = lights_ref.composite(n, L["g0"], L["E"], g["albedo_occ"], pos, nrm, alb, Dn, Sn, lights)
        assert np.isfinite(base).all()
        if len(sel) == 10:        # the second directional light reaches the non-finite rows with V = 1
            lit = lights_ref.composite(n, L["g0"], L["E"], g["albedo_occ"], pos, nrm, alb, Dn, Sn, lights[:-1])
            assert (base[1, 0:4, :3] > lit[1, 0:4, :3]).all()      # rows 5..8: NaN x, +inf y, -inf z, 1e30
        assert bits_equal(lin, R.composite(base, pos, Em, 1.5)), (w, h, sel)
        assert hit.reshape(-1).tolist() == [k == 0 for k in sel]
        bg = pos[..., 3] == 0
        assert np.all(px[bg] == (51 | (77 << 8) | (77 << 16) | (255 << 24)))
    ctx.close()


def test_composite_identities_on_a_partial_block(gpu_ready, oracle_mod):
    """The three light-list composites are one kernel: with scale +0 the emissive one equals
    vct_composite_lights_device (vis NULL) and vct_composite_shadowed_device (vis V), bit for bit in
    both outputs.  n = 16, a 13 x 7 frame (91 lanes of one 256-lane block) with background pixels
    and one non-finite position, one directional, one point and one spot light.  test_composite has
    the first identity on a clean 80 x 48 frame and the second through the reference, linear only."""
    import torch
    n, w, h = 16, 13, 7
    L = R.lamp(n)
    S7 = lights_ref.light_set_s(n)
    lights = [next(l for l in S7 if l.type == t) for t in (0, 1, 2)]
    ctx = _lamp_ctx(n)
    assert ctx.emission_voxels() > 0                                       # a live grid: only scale +0 switches the term off
    ctx.inject_lights(lights)
    ctx.build_mips()
    gb, D, S = _frame(ctx, w, h)
    vis = torch.full((len(lights), h, w), float("nan"), device="cuda")
    ctx.shadow_cones_device(gb[0], gb[1], w, h, lights, [0.1, 0.0, 0.2], vis)   # V of the clean frame
    torch.cuda.synchronize()
    pos = gb[0].cpu().numpy()
    pos[0, :3, 3] = 0.0                                                    # background, whatever the rays met
    fg = np.argwhere(pos[..., 3] != 0)
    assert len(fg) >= 20 and (pos[..., 3] == 0).sum() >= 3
    pos[fg[7][0], fg[7][1], 0] = np.nan
    gb[0] = torch.from_numpy(pos).cuda()

    def other(call, *tail):
        lin = torch.full((h, w, 4), float("nan"), device="cuda")
        px = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        call(*gb, D, S, w, h, lights, *tail, out_linear4=lin, out_rgba8=px)
        torch.cuda.synchronize()
        return lin.cpu().numpy(), px.cpu().numpy().view(np.uint32)

    lin, px = _emissive(ctx, gb, D, S, lights, None, 0.0)
    want, want_px = other(ctx.composite_lights_device)
    assert bits_equal(lin, want) and np.array_equal(px, want_px)
    lin, px = _emissive(ctx, gb, D, S, lights, vis, 0.0)
    soft, soft_px = other(ctx.composite_shadowed_device, vis)
    assert bits_equal(lin, soft) and np.array_equal(px, soft_px)
    assert not bits_equal(soft, want)                                      # V is not the walk's
    ctx.close()


# ---- 7. state and errors -----------------------------------------------------------------
def test_errors_and_state(gpu_ready, oracle_mod, tmp_path):
    import torch
    from vct import Context, VctError, _lib, dump
    n = 16
    L = R.lamp(n)
    v, i, m, _ = L["arrays"]
    ke = L["ke"]
    lib = _lib.load()
    bind = lambda name: _lib.bind_emission_extension(lib, name)
    vox, vox_dev, inject = bind("vct_voxelize_emission"), bind("vct_voxelize_emission_device"), bind("vct_inject_emission")
    count = C.c_uint32(7)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    host_args = lambda kk: (P(v), 56, v.shape[0], P(i), i.size, P(m), None if kk is None else P(kk), ke.shape[0])

    ctx = Context(n, L["g0"], L["E"])
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    assert vox(ctx.h, *host_args(ke)) == ESTATE                            # before a voxelization
    assert inject(ctx.h, 1.0) == ESTATE
    assert bind("vct_emission_voxels")(ctx.h, C.byref(count)) == ESTATE
    ctx.voxelize(*L["arrays"])
    assert ctx.emission_voxels() == 0
    assert inject(ctx.h, 1.0) == ESTATE                                    # no level 0 yet
    ctx.voxelize_emission(v, i, m, ke)
    assert ctx.emission_voxels() == T.LAMP[n]["emissive"]
    assert inject(ctx.h, 1.0) == ESTATE                                    # still none

    def refused(status, call, *args):
        """The call fails with `status` and leaves an empty emission grid; a good one rebuilds it."""
        assert call(ctx.h, *args) == status
        assert lib.vct_last_error(ctx.h)
        assert ctx.emission_voxels() == 0 and not ctx.download_emission().view(np.uint32).any()
        ctx.voxelize_emission(v, i, m, ke)
        assert ctx.emission_voxels() == T.LAMP[n]["emissive"]

    nan, inf = float("nan"), float("inf")
    refused(EINVAL, vox, *host_args(None))                                 # NULL material_ke4
    bad_m = m.copy()
    bad_m[3] = ke.shape[0]
    refused(EINVAL, vox, P(v), 56, v.shape[0], P(i), i.size, P(bad_m), P(ke), ke.shape[0])
    bad_i = i.copy()
    bad_i[5] = v.shape[0]
    refused(EINVAL, vox, P(v), 56, v.shape[0], P(bad_i), i.size, P(m), P(ke), ke.shape[0])
    refused(EINVAL, vox, P(v), 56, v.shape[0], P(i), i.size - 1, P(m), P(ke), ke.shape[0])
    refused(EINVAL, vox, P(v), 10, v.shape[0], P(i), i.size, P(m), P(ke), ke.shape[0])
    dv, di = torch.from_numpy(v).cuda(), torch.from_numpy(i.view(np.int32)).cuda()
    dm = torch.from_numpy(m.view(np.int32)).cuda()
    dev_args = lambda dk, off=0: (dv.data_ptr(), 56, v.shape[0], di.data_ptr(), i.size, dm.data_ptr(),
                                  dk.data_ptr() + off, ke.shape[0])
    for bad in (nan, inf, -inf, -0.0, -1.0, 32768.0):
        for ch in (0, 2):
            kk = ke.copy()
            kk[L["lamp"], ch] = bad
            refused(EINVAL, vox, *host_args(kk))
            refused(EINVAL, vox_dev, *dev_args(torch.from_numpy(kk).cuda()))
    kk = np.vstack([ke, np.array([[nan, -1.0, inf, 0.0]], F)])             # a material no triangle uses is not read
    kk[L["lamp"], 3] = nan                                                 # and Ke.a never is
    ctx.voxelize_emission(v, i, m, kk)
    assert bits_equal(ctx.download_emission(), L["em"]["E"])
    ctx.voxelize_emission_device(dv, di, dm, torch.from_numpy(kk).cuda())
    assert bits_equal(ctx.download_emission(), L["em"]["E"])
    pad = torch.zeros(ke.size + 4, device="cuda")
    refused(EINVAL, vox_dev, *dev_args(pad, 4))                            # material_ke4 not 16-byte aligned
    assert np.array_equal(ctx.download_accum()[1], L["grid"]["counts"])    # the voxel grid was never refused
    ctx.inject_lights([])                                                  # ... and is still usable

    # scale
    before = ctx.download_level(0)
    for bad in (nan, inf, -inf, -0.0, -1.0, 2.0 ** 112):
        assert inject(ctx.h, bad) == EINVAL, bad
        assert bind("vct_composite_emissive_device")(ctx.h, dv.data_ptr(), dv.data_ptr(), dv.data_ptr(), dv.data_ptr(),
                                                     dv.data_ptr(), 4, 4, None, 0, None, bad, dv.data_ptr(), None) == EINVAL
    assert bits_equal(ctx.download_level(0), before)
    ctx.inject_emission(2.0 ** 111)                                        # the limit itself is accepted
    assert np.isfinite(ctx.download_level(0)).all()
    # once per level 0
    ctx.inject_lights([])
    ctx.inject_emission(1.0)
    once = ctx.download_level(0)
    assert bits_equal(once, R.add_to_level0(before, L["em"]["E"], 1.0))
    assert inject(ctx.h, 1.0) == ESTATE
    assert bits_equal(ctx.download_level(0), once)
    ctx.build_mips()
    assert inject(ctx.h, 1.0) == ESTATE                                    # a mip build is not a new level 0
    ctx.inject_bounces(1)
    assert inject(ctx.h, 1.0) == ESTATE
    ctx.inject_lights([])                                                  # re-armed by a new level 0 ...
    ctx.build_mips()
    ctx.inject_bounces(1)
    bounced = ctx.download_level(0)
    assert inject(ctx.h, 1.0) == ESTATE                                    # ... but not after its bounces
    assert bits_equal(ctx.download_level(0), bounced)
    for renew in (lambda: ctx.inject_lights([]), lambda: ctx.upload_level0(before),
                  lambda: ctx.inject_directional((0.3, 1.0, 0.2))):
        renew()
        ctx.inject_emission(1.0)
        with pytest.raises(VctError) as e:
            ctx.inject_emission(1.0)
        assert e.value.status == ESTATE

    # the same inputs twice on one context and once on a fresh one: no accumulator state leaks
    ctx.voxelize_emission(v, i, m, ke)
    a = ctx.download_emission()
    ctx.voxelize_emission(v, i, m, ke)
    b = ctx.download_emission()
    fresh = _lamp_ctx(n)
    c = fresh.download_emission()
    fresh.close()
    assert bits_equal(a, b) and bits_equal(a, c) and bits_equal(a, L["em"]["E"])

    # a voxelization and a load empty the grid; a dump does not hold it
    stem = str(tmp_path / "lamp")
    ctx.inject_lights([])
    dump.save_grid(ctx, stem)
    ctx.voxelize(*L["arrays"])
    assert ctx.emission_voxels() == 0 and not ctx.download_emission().view(np.uint32).any()
    ctx.voxelize_emission(v, i, m, ke)
    assert ctx.emission_voxels() == T.LAMP[n]["emissive"]
    dump.load_grid(stem, ctx=ctx)
    assert ctx.emission_voxels() == 0
    ctx.inject_emission(1.0)                                               # empty: succeeds, changes nothing
    assert bits_equal(ctx.download_level(0), before)
    ctx.voxelize_emission(v, i, m, ke)                                     # the loaded grid takes a new one
    assert bits_equal(ctx.download_emission(), L["em"]["E"])
    ctx.close()


# ---- 8. a multi-device context ---------------------------------------------------------------
def test_multi_device_context_equals_single(gpu_ready, oracle_mod):
    """vct_create_multi(cfg, 2) (the ranks share the device on a one-GPU host): device 0 adds the
    emission, the other device receives level 0 with the build's peer copy."""
    from vct import scenes
    from vct.camera import Camera
    n = 32
    L = R.lamp(n)
    g = L["grid"]
    lights = lights_ref.light_set_s(n)
    want = R.add_to_level0(lights_ref.inject(n, L["g0"], L["E"], g["albedo_occ"], g["normal"], lights), L["em"]["E"], 1.0)
    cam = Camera()
    pos, nrm, alb = scenes.raycast_numpy(L["scene"], cam, 160, 72)         # 3 x 2 tiles: both ranks trace
    single, multi = _lamp_ctx(n), _lamp_ctx(n, devices=2)
    assert multi.num_devices == 2
    for c in (single, multi):
        c.inject_lights(lights)
        c.build_mips()                                                     # level 0 is on the peers ...
        c.inject_emission(1.0)                                             # ... and is marked stale again here
        c.build_mips()
    _assert_grid(multi, oracle_mod, n, want, "2 devices")
    a, b = single.trace(pos, nrm, alb, cam.position), multi.trace(pos, nrm, alb, cam.position)
    dark = _lamp_ctx(n, emit=False)
    dark.inject_lights(lights)
    dark.build_mips()
    d = dark.trace(pos, nrm, alb, cam.position)
    dark.close()
    assert not np.array_equal(a["diffuse"], d["diffuse"])                  # the lamp reaches the frame
    for key in ("diffuse", "spec", "steps_px"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    single.close()
    multi.close()
