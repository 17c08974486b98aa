"""include/vct_dynamic.h on the GPU.  The reference of every comparison is a fresh context's
vct_voxelize of union(static, layer) (tests/dynamic_ref.py) and the CPU oracle on the same
mesh; every comparison is bit for bit: K1's sums are integers, so retracting a layer and adding
another leaves exactly what a voxelization of the union leaves, and everything after K1 is a
function of that state.  Static scene: the Cornell box; layers: dynamic_ref's catalogue.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dynamic_ref as D
import voxel_inputs as VI
from helpers import gpu_pyramid_flat

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 5
F = np.float32
W, H = 64, 48
EYE = (0.0, 0.0, 4.0)
KD_MESSAGE = "material_kd4: Kd not finite or |Kd| >= 32768"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def _grid(n):
    from vct import scenes
    return scenes.grid_for_unit_box(n)


def _ctx(n, static=None, grid=None, **kw):
    import torch
    from vct import Context
    g0, E = grid or _grid(n)
    ctx = Context(n, g0, E, **kw)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    if static is not False:
        ctx.voxelize(*(static or D.static_arrays()))
    return ctx


def _packed(ctx):
    from vct import _lib
    return _lib.debug_accum_packed(ctx.lib, ctx.h)


def _k1(ctx):
    sums, counts = ctx.download_accum()
    ao, nm = ctx.download_voxels()
    return {"sums": sums, "counts": counts, "ao": ao, "nm": nm}


def _gbuffers(ctx):
    import torch
    from vct.camera import Camera
    cam = Camera(position=EYE)
    out = {}
    for name, fn in (("raycast", ctx.gbuffer_raycast_device), ("raster", ctx.gbuffer_raster_device)):
        gb = [torch.full((H, W, 4), float("nan"), device="cuda") for _ in range(3)]
        fn(cam, W, H, 0.1, *gb)
        torch.cuda.synchronize()
        out[name] = [g.cpu().numpy() for g in gb]
    return out


def _snap(ctx, n, frame=True):
    """Everything the issue lists, from the context as it stands after a voxelization or a layer
    update: K1's state, level 0 of both injects, every mip face, the bounce sources, both
    G-buffer passes and K4 on the raster pass's frame."""
    import lights_ref
    from vct import scenes
    out = _k1(ctx)
    ctx.inject_lights(lights_ref.light_set_s(n))
    out["l0_lights"] = ctx.download_level(0)
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    out["l0"] = ctx.download_level(0)
    ctx.build_mips()
    out["pyr"] = gpu_pyramid_flat(ctx)
    out["sources"] = np.array([ctx.bounce_sources()])
    if frame:
        gb = _gbuffers(ctx)
        for k, planes in gb.items():
            for j, p in enumerate(planes):
                out[f"{k}{j}"] = p
        t = ctx.trace(*gb["raster"], EYE)
        out.update(diffuse=t["diffuse"], spec=t["spec"], steps_px=t["steps_px"], cone_steps=np.array([t["cone_steps"]]))
    return out


def _assert_same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert _same(got[k], want[k]), f"{what}: {k} differs"


def _assert_k1(ctx, want, what):
    got = _k1(ctx)
    for k in ("counts", "sums", "ao", "nm"):
        assert _same(got[k], want[k]), f"{what}: {k} differs"


_union = {}


def _union_snap(n, name, layer=None, static=None, grid=None, frame=True, key=True):
    """The snapshot of a fresh context voxelized with union(static, layer), once per key."""
    k = (n, name, frame)
    if key and k in _union:
        return _union[k]
    st = static or D.static_arrays()
    ctx = _ctx(n, D.union(st, layer if layer is not None else D.layers()[name]), grid)
    snap = _snap(ctx, n, frame)
    ctx.close()
    if key:
        _union[k] = snap
    return snap


def _assert_oracle(O, n, snap, mesh, what, grid=None):
    from vct import scenes
    g0, E = grid or _grid(n)
    ref = O.pipeline(n, g0, E, *mesh, scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    for k, r in (("counts", "counts"), ("sums", "sums"), ("ao", "albedo_occ"), ("nm", "normal"), ("l0", "r0"), ("pyr", "pyr")):
        assert _same(snap[k], ref[r]), f"{what}: {k} differs from the oracle"
    if "diffuse" in snap:
        t = O.trace(n, g0, E, ref["r0"], ref["pyr"], snap["raster0"], snap["raster1"], snap["raster2"], EYE)
        for k in ("diffuse", "spec", "steps_px"):
            assert _same(snap[k], t[k]), f"{what}: K4 {k} differs from the oracle"
        assert int(snap["cone_steps"][0]) == t["cone_steps"] > 0


# ---- 1. add ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", D.ADD)
@pytest.mark.parametrize("n", D.GRIDS)
def test_add_a_layer(gpu_ready, oracle_mod, n, name):
    """A layer in empty space, overlapping static voxels, cutting into the short box, through
    the grid's +x face, wholly outside (no candidates) and empty."""
    layer = D.layers()[name]
    ctx = _ctx(n)
    ctx.voxelize_dynamic(*layer)
    got = _snap(ctx, n)
    assert ctx.dynamic_voxels() == int((D.layer_coverage(n, name)[1] > 0).sum())
    ctx.close()
    _assert_same(got, _union_snap(n, name), f"{name} at {n}")
    _assert_oracle(oracle_mod, n, got, D.union(D.static_arrays(), layer), f"{name} at {n}")
    if name in ("outside", "empty"):
        _assert_same(got, _union_snap(n, "empty"), "a layer without candidates leaves the static grid")
    else:
        assert not _same(got["counts"], _union_snap(n, "empty")["counts"])
        if name == "floor":                                   # in front of the camera: both passes see the layer
            assert not _same(got["raycast0"], _union_snap(n, "empty")["raycast0"])
            assert not _same(got["raster2"], _union_snap(n, "empty")["raster2"])


def test_add_at_64(gpu_ready, oracle_mod):
    """64^3: K2's coarse bits and a K3 live-block list that is not the whole grid."""
    n, name = 64, "floor"
    ctx = _ctx(n)
    ctx.voxelize_dynamic(*D.layers()[name])
    got = _snap(ctx, n)
    ctx.voxelize_dynamic(*D.layers()["empty"])
    back = _snap(ctx, n)
    ctx.close()
    _assert_same(got, _union_snap(n, name), "floor at 64")
    _assert_same(back, _union_snap(n, "empty"), "removed at 64")
    _assert_oracle(oracle_mod, n, got, D.union(D.static_arrays(), D.layers()[name]), "floor at 64")


# ---- 2. replace and remove ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", D.GRIDS)
def test_replace_and_remove(gpu_ready, oracle_mod, n):
    """floor -> tet (beside it) -> over (overlapping tet) -> none.  After every step the
    context equals the union's; at the end the static grid alone, with all-zero records and a
    +0 level 0 at every voxel a layer had occupied."""
    S = D.static_coverage(n)[1] > 0
    ctx = _ctx(n)
    seen = np.zeros_like(S)
    for name in D.REPLACE:
        ctx.voxelize_dynamic(*D.layers()[name])
        hit = D.layer_coverage(n, name)[1] > 0
        assert ctx.dynamic_voxels() == int(hit.sum())
        if name == "empty":                                   # before anything is injected again
            sums, counts = ctx.download_accum()
            assert not counts[~S].any() and not sums[~S].any()
            vac = (seen & ~S).reshape(n, n, n)
            assert vac.sum() >= 1
            assert not ctx.download_level(0)[vac].view(np.uint32).any()      # +0, not -0
            ao, nm = ctx.download_voxels()
            assert not ao[vac].view(np.uint32).any() and not nm[vac].view(np.uint32).any()
        seen |= hit
        got = _snap(ctx, n)
        _assert_same(got, _union_snap(n, name), f"step {name} at {n}")
        ref = D.coverage(n, D.union(D.static_arrays(), D.layers()[name]))
        assert _same(got["sums"], ref[0]) and _same(got["counts"], ref[1]), name
    ctx.close()
    static = _ctx(n)
    _assert_same(got, _snap(static, n), "after the last step: the static grid alone")
    static.close()


# ---- 3. no drift ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", D.GRIDS)
def test_no_drift_over_24_steps(gpu_ready, oracle_mod, n):
    path = D.path()
    ctx = _ctx(n)
    for layer in path:
        ctx.voxelize_dynamic(*layer)
    got = _snap(ctx, n)
    ctx.voxelize_dynamic(*D.layers()["empty"])
    back = _snap(ctx, n, frame=False)
    ctx.close()
    _assert_same(got, _union_snap(n, "path23", path[-1]), f"24 steps at {n}")
    ref = D.coverage(n, D.union(D.static_arrays(), path[-1]))
    assert _same(got["sums"], ref[0]) and _same(got["counts"], ref[1])
    _assert_same(back, _union_snap(n, "empty", frame=False), "and removed")


# ---- 4. the packed layout cannot hold the union --------------------------------------------------------
def _kd_max_triangle(y):
    """One tiny triangle of Kd 32767.99 (tests/voxel_inputs.py's value) at height y."""
    v = np.zeros((3, 14), F)
    v[:, :3] = [(0.5, y, 0.5), (0.52, y, 0.5), (0.5, y + 0.01, 0.52)]
    return v, np.arange(3, dtype=np.uint32), np.zeros(1, np.uint32), np.array([[32767.99, -32767.99, 32767.99, 1.0]], F)


def _layout_case(O, n, static, layer, grid, packed_before, packed_after, what):
    ctx = _ctx(n, static, grid)
    assert _packed(ctx) == packed_before, what
    ctx.voxelize_dynamic(*layer)
    assert _packed(ctx) == packed_after, what
    mesh = D.union(static, layer)
    ref = O.voxelize(n, *grid, *mesh)
    ao, nm = O.resolve(n, *ref)
    _assert_k1(ctx, {"sums": ref[0], "counts": ref[1], "ao": ao, "nm": nm}, what + ": the oracle")
    got = _snap(ctx, n, frame=False)
    _assert_same(got, _union_snap(n, what, layer, static, grid, frame=False, key=False), what + ": the union")
    ctx.voxelize_dynamic(*D.layers()["empty"])                # d. remove it again
    assert _packed(ctx) == packed_after
    back = _snap(ctx, n, frame=False)
    fresh = _ctx(n, static, grid)
    _assert_same(back, _snap(fresh, n, frame=False), what + ": removed")
    fresh.close()
    ctx.close()
    return ref


def test_layout_packed_static_large_kd_layer(gpu_ready, oracle_mod):
    """a. The layer's one triangle lands in a floor voxel: count 2 x 2^31 cannot be packed, the
    records are converted in place.  Alone in an empty voxel the same triangle keeps the packed
    layout (count 1 x max|value| < 2^31) and is exact there too."""
    n, grid = 16, _grid(16)
    ref = _layout_case(oracle_mod, n, D.static_arrays(), _kd_max_triangle(-0.99), grid, True, False, "kd_max on the floor")
    assert ref[0][:, 0].max() > 2 ** 31 - 1024 and ref[1].max() >= 2
    _layout_case(oracle_mod, n, D.static_arrays(), _kd_max_triangle(0.4), grid, True, True, "kd_max in the air")


def test_layout_unpacked_static_plain_layer(gpu_ready, oracle_mod):
    """b. The static scene itself was forced unpacked by that Kd; a plain layer on top."""
    n, grid = 16, _grid(16)
    static = D.union(D.static_arrays(), _kd_max_triangle(-0.99))
    _layout_case(oracle_mod, n, static, D.layers()["floor"], grid, False, False, "unpacked static")


def test_layout_union_count_overflows(gpu_ready, oracle_mod):
    """c. test_parity_gpu.py's 40 000 triangles in one voxel, split 20 000 / 20 000: neither
    part reaches count x 65 536 >= 2^31, the union does."""
    n, T, grid = 8, 40000, ((0.0, 0.0, 0.0), 1.0)
    rng = np.random.default_rng(11)
    c = np.array([4.5, 4.5, 4.5], F) / n
    v = (c + rng.uniform(-0.3, 0.3, (T, 3, 3)).astype(F) / n).reshape(-1, 3)
    kd = np.array([[0.9, 0.2, 1.0, 1.0], [0.3, 1.0, 0.1, 1.0]], F)
    half = lambda a, b: (v[3 * a:3 * b], np.arange(3 * (b - a), dtype=np.uint32), (np.arange(a, b) % 2).astype(np.uint32), kd)
    ref = _layout_case(oracle_mod, n, half(0, T // 2), half(T // 2, T), grid, True, False, "20 000 + 20 000")
    assert ref[1].max() == T and T // 2 * 65536 < 2 ** 31 <= T * 65536


# ---- 5. input rule and state --------------------------------------------------------------------------
@pytest.mark.parametrize("family", VI.FAMILIES)
def test_hostile_families_as_layers(gpu_ready, oracle_mod, family):
    """tests/voxel_inputs.py's catalogue, one family per layer, over the Cornell box (12-byte
    vertices on both sides): K1's input rule, word for word."""
    n = 16
    mesh = VI.build((family,), n, "unit")
    sv, si, sm, sk = D.static_arrays()
    static = (np.ascontiguousarray(sv[:, :3]), si, sm, sk)
    layer = (mesh.verts, mesh.idx, mesh.mat, mesh.kd)
    grid = (mesh.g0, mesh.E)
    ctx = _ctx(n, static, grid)
    ctx.voxelize_dynamic(*layer)
    ref = oracle_mod.voxelize(n, *grid, *D.union(static, layer))
    ao, nm = oracle_mod.resolve(n, *ref)
    _assert_k1(ctx, {"sums": ref[0], "counts": ref[1], "ao": ao, "nm": nm}, family)
    got = _snap(ctx, n, frame=False)
    _assert_same(got, _union_snap(n, family, layer, static, grid, frame=False, key=False), family)
    ctx.voxelize_dynamic(*D.layers()["empty"])
    fresh = _ctx(n, static, grid)
    _assert_k1(ctx, _k1(fresh), family + " removed")
    fresh.close()
    ctx.close()


def _lit_frame(ctx, n):
    from vct import scenes
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    ctx.build_mips()
    return _frame(ctx)


def _frame(ctx):
    gb = _gbuffers(ctx)["raster"]
    t = ctx.trace(*gb, EYE)
    return {"pos": gb[0], "diffuse": t["diffuse"], "spec": t["spec"], "steps_px": t["steps_px"]}


def test_host_errors_leave_everything_as_it_was(gpu_ready, oracle_mod):
    from vct import VctError, _lib
    n = 16
    ctx = _ctx(n)
    ctx.voxelize_dynamic(*D.layers()["floor"])
    before, k1, vox = _lit_frame(ctx, n), _k1(ctx), ctx.dynamic_voxels()
    v, i, m, k = D.layers()["tet"]
    bad = k.copy()
    fn = _lib.bind_dynamic_extension(ctx.lib, "vct_voxelize_dynamic")
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for value in (32768.0, -32768.0, np.inf, np.nan):
        bad[0, 1] = value
        with pytest.raises(VctError) as e:
            ctx.voxelize_dynamic(v, i, m, bad)
        assert e.value.status == EINVAL and KD_MESSAGE in str(e.value)
    raw = [(p(v), 56, v.shape[0], None, i.size, p(m), p(k), 1),       # NULL idx
           (None, 56, v.shape[0], p(i), i.size, p(m), p(k), 1),       # NULL verts
           (p(v), 8, v.shape[0], p(i), i.size, p(m), p(k), 1),        # stride < 12
           (p(v), 58, v.shape[0], p(i), i.size, p(m), p(k), 1),       # stride % 4
           (p(v), 56, v.shape[0], p(i), i.size - 1, p(m), p(k), 1),   # n_idx % 3
           (p(v), 56, v.shape[0], p(i), i.size, p(m), p(k), 0)]       # material_kd4 with n_materials == 0
    for args in raw:
        assert fn(ctx.h, *args) == EINVAL, args[1:]
    # nothing was invalidated: the trace runs and is the one before; the layer is still floor
    after = _frame(ctx)
    for key in before:
        assert _same(before[key], after[key]), key
    _assert_k1(ctx, k1, "after refused calls")
    assert ctx.dynamic_voxels() == vox
    ctx.voxelize_dynamic(*D.layers()["empty"])                # and floor can still be retracted exactly
    fresh = _ctx(n)
    _assert_k1(ctx, _k1(fresh), "floor removed after refused calls")
    fresh.close()
    ctx.close()


@pytest.mark.parametrize("form", ["index", "material", "kd_device"])
def test_device_errors_refuse_the_grid(gpu_ready, oracle_mod, form):
    import torch
    from vct import VctError, scenes
    n = 16
    ctx = _ctx(n)
    ctx.voxelize_dynamic(*D.layers()["floor"])
    v, i, m, k = (a.copy() for a in D.layers()["tet"])
    with pytest.raises(VctError) as e:
        if form == "index":
            i[4] = v.shape[0]
            ctx.voxelize_dynamic(v, i, m, k)
        elif form == "material":
            m[1] = k.shape[0]
            ctx.voxelize_dynamic(v, i, m, k)
        else:
            k[0, 2] = 40000.0
            dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()
            ctx.voxelize_dynamic_device(dev(v, F), dev(i, np.int32), dev(m, np.int32), dev(k, F))
    assert e.value.status == EINVAL
    assert (KD_MESSAGE in str(e.value)) == (form == "kd_device")
    for call in (lambda: ctx.inject_directional(scenes.LIGHT_DIR), lambda: ctx.voxelize_dynamic(*D.layers()["tet"]),
                 lambda: ctx.download_accum(), lambda: ctx.dynamic_voxels(), lambda: _frame(ctx)):
        with pytest.raises(VctError) as e:
            call()
        assert e.value.status == ESTATE
    ctx.voxelize(*D.static_arrays())                           # a voxelization ends the refusal
    assert ctx.dynamic_voxels() == 0
    ctx.voxelize_dynamic(*D.layers()["tet"])
    _assert_same(_snap(ctx, n, frame=False), _union_snap(n, "tet", frame=False), "after the refusal")
    ctx.close()


def test_state_rules(gpu_ready, oracle_mod):
    from vct import VctError, scenes
    n = 16
    ctx = _ctx(n, static=False)
    for call in (lambda: ctx.voxelize_dynamic(*D.layers()["floor"]), lambda: ctx.dynamic_voxels()):
        with pytest.raises(VctError) as e:                     # before any voxelization
            call()
        assert e.value.status == ESTATE
    ctx.voxelize(*D.static_arrays())
    assert ctx.dynamic_voxels() == 0
    _lit_frame(ctx, n)
    ctx.voxelize_dynamic(*D.layers()["floor"])
    gb = _gbuffers(ctx)["raster"]                              # the G-buffer needs no light
    for call in (lambda: ctx.trace(*gb, EYE), lambda: ctx.build_mips(), lambda: ctx.inject_bounces(1)):
        with pytest.raises(VctError) as e:                     # level 0 and the mips are the old grid's
            call()
        assert e.value.status == ESTATE
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    with pytest.raises(VctError) as e:
        ctx.trace(*gb, EYE)
    assert e.value.status == ESTATE
    ctx.build_mips()
    ctx.trace(*gb, EYE)
    # a new voxelization drops the layer record: the grid it leaves is the static grid
    ctx.voxelize(*D.static_arrays())
    assert ctx.dynamic_voxels() == 0
    ctx.voxelize_dynamic(*D.layers()["tet"])
    _assert_same(_snap(ctx, n, frame=False), _union_snap(n, "tet", frame=False), "a layer after a new voxelization")
    ctx.close()


def test_emission_grid_of_the_previous_epoch_is_not_applied(gpu_ready, oracle_mod):
    from vct import scenes
    n = 16
    v, i, m, k = D.static_arrays()
    ke = np.zeros_like(k)
    ke[0, :3] = (2.0, 1.0, 0.5)
    ctx = _ctx(n)
    ctx.voxelize_emission(v, i, m, ke)
    assert ctx.emission_voxels() > 0
    ctx.voxelize_dynamic(*D.layers()["floor"])
    assert ctx.emission_voxels() == 0
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    ctx.inject_emission(1.0)                                   # empty: succeeds, adds nothing
    assert _same(ctx.download_level(0), _union_snap(n, "floor")["l0"])
    ctx.close()


# ---- 6. the device form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["floor", "straddle", "empty"])
def test_device_form_equals_host_form(gpu_ready, oracle_mod, name):
    import torch
    n = 32
    v, i, m, k = D.layers()[name]
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()
    ctx = _ctx(n)
    ctx.voxelize_dynamic_device(dev(v, F), dev(i, np.int32), dev(m, np.int32), dev(k, F))
    assert ctx.dynamic_voxels() == int((D.layer_coverage(n, name)[1] > 0).sum())
    _assert_same(_snap(ctx, n), _union_snap(n, name), f"device form, {name}")
    ctx.voxelize_dynamic_device(dev(v, F), dev(i, np.int32), None, None)      # material 0, albedo 1
    white = (v, i, np.zeros_like(m), np.ones((1, 4), F))
    _assert_same(_snap(ctx, n, frame=False), _union_snap(n, name + " white", white, frame=False), "NULL materials")
    ctx.close()


# ---- 7. a multi-device context ----------------------------------------------------------------------------------
def test_multi_device_context_equals_single(gpu_ready, oracle_mod):
    """vct_create_multi(cfg, 2) (the ranks share the device on a one-GPU host): device 0 runs
    the update, the other rank receives the new level 0 with the build's peer copy."""
    from vct import scenes
    from vct.camera import Camera
    n = 32
    cam = Camera()
    multi = _ctx(n, devices=2)
    assert multi.num_devices == 2
    multi.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    multi.build_mips()                                         # level 0 is on the peers; the update must retire it
    frames = []
    for name in ("floor", "over"):
        multi.voxelize_dynamic(*D.layers()[name])
        got = _snap(multi, n, frame=False)
        _assert_same(got, _union_snap(n, name, frame=False), f"2 devices, {name}")
        single = _ctx(n, D.union(D.static_arrays(), D.layers()[name]))
        single.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
        single.build_mips()
        gb = _gbuffers(single)["raster"]
        big = [np.tile(p, (2, 3, 1)) for p in gb]              # 192 x 96: 3 x 2 tiles, both ranks trace
        a, b = single.trace(*big, EYE), multi.trace(*big, EYE)
        for key in ("diffuse", "spec", "steps_px"):
            assert _same(a[key], b[key]), (name, key)
        frames.append(a["diffuse"])
        single.close()
    assert not _same(frames[0], frames[1])
    multi.close()


# ---- 8. dumps ---------------------------------------------------------------------------------------------------------
def test_dump_saves_the_union(gpu_ready, oracle_mod, tmp_path):
    from vct import dump, scenes
    n = 16
    ctx = _ctx(n)
    ctx.voxelize_dynamic(*D.layers()["tet"])
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    ctx.build_mips()
    dump.save_grid(ctx, tmp_path / "union", pyramid=True)
    ctx.close()
    want = _union_snap(n, "tet", frame=False)
    loaded = dump.load_grid(tmp_path / "union")
    assert _same(loaded.download_level(0), want["l0"]) and _same(gpu_pyramid_flat(loaded), want["pyr"])
    assert loaded.dynamic_voxels() == 0
    _assert_same(_snap(loaded, n, frame=False), want, "loaded")
    loaded.voxelize_dynamic(*D.layers()["empty"])              # no layer record came with the dump: nothing to retract
    _assert_same(_snap(loaded, n, frame=False), want, "loaded, then an empty layer")
    loaded.voxelize_dynamic(*D.layers()["air"])                # the loaded union is the static grid now
    both = D.union(D.union(D.static_arrays(), D.layers()["tet"]), D.layers()["air"])
    ref = D.coverage(n, both)
    got = loaded.download_accum()
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    loaded.close()


# ---- 9. features on top -------------------------------------------------------------------------------------------------
def _feature(ctx, which, n):
    import sky_ref
    from vct import scenes
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    if which == "emission":
        v, i, m, k = D.union(D.static_arrays(), D.layers()["floor"])
        ke = np.zeros_like(k)
        ke[-1, :3] = (3.0, 2.0, 1.0)                          # the layer's material glows
        ctx.voxelize_emission(v, i, m, ke)
        assert ctx.emission_voxels() > 0
        ctx.inject_emission(1.5)
    ctx.build_mips()
    if which == "sky":
        ctx.inject_sky(sky_ref.to_ctypes(sky_ref.SKY_TILTED))
    if which == "bounce":
        ctx.inject_bounces(1)
    return {"l0": ctx.download_level(0), "pyr": gpu_pyramid_flat(ctx), **_frame(ctx)}


@pytest.mark.parametrize("which", ["bounce", "emission", "sky"])
def test_features_on_top_of_a_layer(gpu_ready, oracle_mod, which):
    n = 16
    ctx = _ctx(n)
    ctx.voxelize_dynamic(*D.layers()["tet"])                   # a step before, so that something is retracted
    ctx.voxelize_dynamic(*D.layers()["floor"])
    got = _feature(ctx, which, n)
    ctx.close()
    ref_ctx = _ctx(n, D.union(D.static_arrays(), D.layers()["floor"]))
    want = _feature(ref_ctx, which, n)
    plain = _lit_frame(ref_ctx, n)
    ref_ctx.close()
    _assert_same(got, want, which)
    assert not _same(want["diffuse"], plain["diffuse"])        # the feature reaches the frame


# ---- 10. the host ----------------------------------------------------------------------------------------------------------
def _write_box_obj(directory, name, lo, hi, kd):
    from helpers import write_obj
    from vct import scenes
    s = scenes.Scene(name)
    s.box(lo, hi, s.material(kd))
    return write_obj(s, directory, name)


def test_headless_dynamic_flag(gpu_ready, oracle_mod, tmp_path):
    """vct_headless --dynamic box.obj --dynamic-offset ... writes the linear frame the Python
    binding computes from the arrays the host loader returns for the two files (the box moved
    by the host's own Transform): the static file voxelized, the box as the layer; and that is
    the frame of a context voxelized with the union of those arrays.  (One OBJ holding the
    static file's text followed by the moved box is not the same input before K1: the host
    loader, which follows assimp's material rules, gives the box's triangles its default Kd
    there, so that comparison would test the loader, not the flag.)"""
    import torch
    import host_lib
    from helpers import write_obj
    from vct import VctCamera, scenes
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "voxel-based-global-illumination_amd", "build", "vct_headless")
    assert os.path.exists(exe), "build the host with `make -C voxel-based-global-illumination_amd host`"
    obj = write_obj(scenes.cornell(), str(tmp_path))
    box = _write_box_obj(str(tmp_path), "box", (-0.15, -0.15, -0.15), (0.15, 0.15, 0.15), (0.2, 0.3, 0.9))
    n, w, h = 32, 64, 48
    off = (-0.05, -0.85, 0.65)
    frames = {}
    for name, flags in (("plain", []), ("dyn", ["--dynamic", box, "--dynamic-offset", "%.9g,%.9g,%.9g" % off]),
                        ("dyn0", [f"--dynamic={box}"])):
        lin = str(tmp_path / f"{name}.f32")
        p = subprocess.run([exe, obj, str(n), str(w), str(h), "2", str(tmp_path / f"{name}.ppm"), "--model=identity",
                            "--grid=unit", f"--linear={lin}"] + flags, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        frames[name] = np.fromfile(lin, F).reshape(h, w, 4)
        grid = re.search(r"aabb_min (\S+) (\S+) (\S+) extent (\S+)", p.stdout)
    assert not _same(frames["plain"], frames["dyn"]) and not _same(frames["dyn"], frames["dyn0"])
    g0 = tuple(float.fromhex(grid.group(j)) for j in (1, 2, 3))
    E = float.fromhex(grid.group(4))
    m = np.eye(4, dtype=F)
    m[3, :3] = off                                             # column-major: elements 12..14
    sv, si, sm, sk, _, _ = host_lib.load_placed(obj)
    bv, bi, bm, bk, _, _ = host_lib.load_placed(box, m.reshape(-1))
    ctx = _ctx(n, (sv, si, sm, sk), (g0, E))
    ctx.voxelize_dynamic(bv, bi, bm, bk)
    ctx.inject_directional((0.3, 1.0, 0.2), (1.0, 1.0, 1.0))  # ConeTraceSettings defaults
    ctx.build_mips()
    c = host_lib.camera_eval((0.0, 0.0, 3.0, -90.0, 0.0), [])  # the host's float camera (main.cpp)
    cam = VctCamera()
    f3 = lambda a: (C.c_float * 3)(*[float(t) for t in a])
    cam.position, cam.front, cam.right, cam.up = f3(c[0:3]), f3(c[3:6]), f3(c[6:9]), f3(c[9:12])
    cam.zoom_deg, cam.near_plane, cam.far_plane = float(c[14]), 0.1, 100.0
    gb = [torch.empty((h, w, 4), device="cuda") for _ in range(3)]
    ctx.gbuffer_raster_device(cam, w, h, 0.1, *gb)
    d, sp, lin = (torch.empty((h, w, 4), device="cuda") for _ in range(3))
    ctx.trace_device(*gb, w, h, tuple(c[0:3]), d, sp)
    ctx.composite_device(*gb, d, sp, w, h, (0.3, 1.0, 0.2), (1.0, 1.0, 1.0), out_linear4=lin)
    torch.cuda.synchronize()
    assert _same(lin.cpu().numpy(), frames["dyn"])
    # and the union's context gives that frame too
    u = _ctx(n, D.union((sv, si, sm, sk), (bv, bi, bm, bk)), (g0, E))
    u.inject_directional((0.3, 1.0, 0.2), (1.0, 1.0, 1.0))
    u.build_mips()
    u.gbuffer_raster_device(cam, w, h, 0.1, *gb)
    u.trace_device(*gb, w, h, tuple(c[0:3]), d, sp)
    u.composite_device(*gb, d, sp, w, h, (0.3, 1.0, 0.2), (1.0, 1.0, 1.0), out_linear4=lin)
    torch.cuda.synchronize()
    assert _same(lin.cpu().numpy(), frames["dyn"])
    u.close()
    ctx.close()
