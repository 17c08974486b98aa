"""Point and spot lights without a GPU: the boundary declares and binds the two functions
of include/vct_lights.h, a library without them (the CPU oracle backend) still loads, and
the reference the GPU tests compare against (tests/lights_ref.py, a numpy restatement of
vct_spec.h "local lights") reproduces the oracle for one directional light, closed-form
answers, and the input classes the GPU tests rely on.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lights_ref
from lights_ref import bits_equal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# lights_ref.cornell(n)["stats"] as found when the tests were written: per light of set S
# (back, culled, walked, blocked, left, reached, zero_l).  Literals, so that an edit of the
# reference cannot quietly empty a class the GPU tests are meant to cover.
STATS = {
    16: [(248, 0, 858, 258, 0, 600, 0), (248, 669, 189, 70, 0, 119, 0), (396, 477, 233, 71, 0, 162, 0),
         (173, 0, 933, 282, 651, 0, 0), (241, 27, 838, 837, 0, 1, 0), (298, 0, 808, 428, 0, 380, 102),
         (463, 0, 643, 558, 85, 0, 0)],
    32: [(1403, 0, 4291, 1077, 0, 3214, 103), (1426, 3341, 927, 233, 0, 694, 0), (2153, 2451, 1090, 224, 0, 866, 0),
         (1060, 0, 4634, 963, 3671, 0, 90), (1420, 384, 3890, 3889, 0, 1, 89), (1742, 0, 3952, 2010, 0, 1942, 231),
         (2352, 0, 3342, 2755, 587, 0, 0)],
}
OCCUPIED = {16: 1106, 32: 5694}
KEYS = ("back", "culled", "walked", "blocked", "left", "reached", "zero_l")
# (light, class) pairs the GPU tests must see: at least 50 at 32^3, at least 1 at 16^3
COVERED = [(1, "reached"), (1, "blocked"), (2, "culled"), (3, "culled"), (3, "reached"), (4, "left"), (4, "blocked"),
           (5, "blocked"), (6, "zero_l"), (7, "blocked"), (7, "left")]


def check_coverage(n):
    c = lights_ref.cornell(n)
    got = [tuple(s[k] for k in KEYS) for s in c["stats"]]
    print(n, got)
    assert int((c["grid"]["counts"] > 0).sum()) == OCCUPIED[n]
    assert got == STATS[n]
    for s in c["stats"]:
        assert s["zero"] == 0
        assert s["back"] + s["culled"] + s["walked"] == OCCUPIED[n]
        assert s["blocked"] + s["left"] + s["reached"] == s["walked"]
    for light, cls in COVERED:
        assert c["stats"][light - 1][cls] >= (50 if n == 32 else 1), (n, light, cls)
    five = c["stats"][4]
    assert five["walked"] - five["blocked"] >= 1              # the light inside the short box: one walk escapes


def test_header_declares_light_functions():
    src = open(os.path.join(REPO, "include", "vct_lights.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"vct_status\s+vct_inject_lights\s*\(\s*vct_ctx\s*\*\s*\w*\s*,\s*const\s+vct_light\s*\*\s*\w+\s*,"
                     r"\s*uint32_t\s+\w+\s*\)\s*;", code)
    assert re.search(r"vct_status\s+vct_composite_lights_device\s*\(", code)
    for name, value in (("VCT_LIGHT_DIRECTIONAL", "0u"), ("VCT_LIGHT_POINT", "1u"), ("VCT_LIGHT_SPOT", "2u"),
                        ("VCT_MAX_LIGHTS", "64u")):
        assert re.search(rf"#define\s+{name}\s+{value}\b", code)
    vct_h = open(os.path.join(REPO, "include", "vct.h")).read()
    assert '#include "vct_lights.h"' in vct_h and '#include "vct_bounce.h"' in vct_h
    assert re.search(r"#define\s+VCT_ABI_VERSION\s+1\b", vct_h)
    assert "local lights" in open(os.path.join(REPO, "include", "vct_spec.h")).read()


def test_binding_lists_them_and_hip_library_exports_them():
    from vct import Context, VctLight, _lib
    assert set(_lib.LIGHT_EXTENSIONS) == {"vct_inject_lights", "vct_composite_lights_device"}
    assert set(_lib.EXTENSIONS) == {"vct_inject_bounces", "vct_bounce_sources"}      # unchanged
    assert not set(_lib.LIGHT_EXTENSIONS) & (set(_lib.EXPORTS) | set(_lib.EXTENSIONS))
    assert callable(Context.inject_lights) and callable(Context.composite_lights_device)
    assert C.sizeof(VctLight) == 60 and _lib.VCT_MAX_LIGHTS == 64
    assert (VctLight.position.offset, VctLight.direction.offset, VctLight.color.offset, VctLight.range.offset,
            VctLight.cos_inner.offset, VctLight.cos_outer.offset, VctLight.reserved.offset) == (4, 16, 28, 40, 44, 48, 52)
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vct_[a-z0-9_]+)", out))
    assert set(_lib.LIGHT_EXTENSIONS) <= exported
    assert lib.vct_abi_version() == 1
    # VCT_EINVAL for a NULL ctx, no device needed
    assert _lib.bind_light_extension(lib, "vct_inject_lights")(None, None, 0) == 1
    one = (VctLight * 1)()
    assert _lib.bind_light_extension(lib, "vct_inject_lights")(None, one, 1) == 1
    assert _lib.bind_light_extension(lib, "vct_composite_lights_device")(None, None, None, None, None, None, 4, 4,
                                                                          None, 0, None, None) == 1


def test_constructors():
    import vct
    from vct import _lib
    d = vct.directional_light((0.0, 2.0, 0.0), (1.0, 0.5, 0.25))
    assert d.type == _lib.VCT_LIGHT_DIRECTIONAL and tuple(d.direction) == (0.0, 2.0, 0.0)
    assert tuple(d.color) == (1.0, 0.5, 0.25) and tuple(d.reserved) == (0, 0)
    p = vct.point_light((1.0, 2.0, 3.0), range=2.5)
    assert p.type == _lib.VCT_LIGHT_POINT and tuple(p.position) == (1.0, 2.0, 3.0) and p.range == 2.5
    s = vct.spot_light((0, 1, 0), (0, -1, 0), range=3.0, inner_deg=20.0, outer_deg=35.0)
    assert s.type == _lib.VCT_LIGHT_SPOT
    # degrees -> cosines in float32
    assert F(s.cos_inner) == np.cos(np.deg2rad(F(20.0))) and F(s.cos_outer) == np.cos(np.deg2rad(F(35.0)))
    assert np.cos(np.deg2rad(F(20.0))).dtype == np.float32
    s2 = vct.spot_light((0, 1, 0), (0, -1, 0), cos_inner=0.9397, cos_outer=0.8192)
    assert F(s2.cos_inner) == F(0.9397) and F(s2.cos_outer) == F(0.8192)


def test_library_without_them_still_loads(oracle_mod):
    """The CPU backend exports vct.h only: it binds, runs, and refuses a light list by name."""
    import vct
    from helpers import scene_arrays
    from vct import Context, _lib, scenes
    cpu = _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))
    for name in _lib.LIGHT_EXTENSIONS:
        assert not hasattr(cpu, name)
        with pytest.raises(AttributeError, match=name):
            _lib.bind_light_extension(cpu, name)
    s, (v, i, m, k) = scene_arrays("cornell")
    g0, E = scenes.grid_for_unit_box(16)
    ctx = Context(16, g0, E, lib=cpu)
    ctx.voxelize(v, i, m, k)
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    before = ctx.download_level(0)
    with pytest.raises(AttributeError, match="vct_inject_lights"):
        ctx.inject_lights([vct.point_light((0, 0, 0))])
    with pytest.raises(AttributeError, match="vct_composite_lights_device"):
        ctx.composite_lights_device(0, 0, 0, 0, 0, 4, 4, [])
    assert np.array_equal(ctx.download_level(0), before)
    ctx.close()


@pytest.mark.parametrize("n", [16, 32])
def test_one_directional_light_is_the_oracle(oracle_mod, n):
    """lights_ref with [directional] = oracle.inject and oracle.composite, bit for bit."""
    import vct
    from vct import scenes
    from vct.camera import Camera
    c = lights_ref.cornell(n)
    g = c["grid"]
    one = [vct.directional_light(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)]
    assert bits_equal(lights_ref.inject(n, c["g0"], c["E"], g["albedo_occ"], g["normal"], one), g["r0"])
    pos, nrm, alb = scenes.raycast_numpy(c["scene"], Camera(position=(0.0, 0.0, 4.0)), 32, 24)
    rng = np.random.default_rng(5)
    D, S = rng.random((24, 32, 4)).astype(F), (rng.random((24, 32, 4)) * 0.2).astype(F)
    want, _ = oracle_mod.composite(n, c["g0"], c["E"], g["albedo_occ"], pos, nrm, alb, D, S, scenes.LIGHT_DIR,
                                   scenes.LIGHT_COLOR)
    stats = []
    got = lights_ref.composite(n, c["g0"], c["E"], g["albedo_occ"], pos, nrm, alb, D, S, one, stats)
    bg = pos[..., 3] == 0
    assert bg.any() and (~bg).sum() > 300 and stats[0]["walked"] > 100
    assert bits_equal(got, want)


def _floor(n=8):
    """An 8^3 grid of unit voxels at the origin with a floor at y = 1 (normal +y, albedo 0.5)."""
    ao = np.zeros((n, n, n, 4), F)
    nm = np.zeros((n, n, n, 4), F)
    ao[:, 1, :, :] = (0.5, 0.5, 0.5, 1.0)
    nm[:, 1, :, 1] = 1.0
    return n, (0.0, 0.0, 0.0), float(n), ao, nm


def test_known_answers():
    """The voxel (3, 1, 3) of a floor under a light straight above its centre: q = (3.5, 2.5, 3.5),
    d = (0, 4, 0), r = 4, l = (0, 1, 0), ndl = 1; range 8 -> u = 1/4, w = 3/4,
    f = (9/16) / (1 + 16) with h2 = 1; the walk passes y = 2 .. 6 and reaches the light (t_e = 4.5 >= 4)."""
    import vct
    n, g0, E, ao, nm = _floor()
    above = (3.5, 6.5, 3.5)
    stats = []
    r0 = lights_ref.inject(n, g0, E, ao, nm, [vct.point_light(above, (2.0, 2.0, 2.0), 8.0)], stats)
    f = F(0.5625) / F(17.0)
    assert bits_equal(r0[3, 1, 3], np.array([f, f, f, 1.0], F))            # ((0.5 * 2) * 1) * f * 1
    # every floor voxel sees the light; the 15 with x = 3 or z = 3 have an exact-zero component of l
    assert stats[0]["reached"] == 64 and stats[0]["blocked"] == 0 and stats[0]["zero_l"] == 15
    assert not r0[ao[..., 3] == 0].view(np.uint32).any()                   # empty voxels: +0
    # beyond the range: u = 16 / 9 > 1, w = 0
    far = lights_ref.inject(n, g0, E, ao, nm, [vct.point_light(above, (2.0, 2.0, 2.0), 3.0)])
    assert far[3, 1, 3].view(np.uint32).tolist() == [0, 0, 0, F(1.0).view(np.uint32)]
    # outside the outer cone: the spot shines along +x, the voxel is straight below (cd = 0)
    spot = vct.spot_light(above, (1.0, 0.0, 0.0), (2.0, 2.0, 2.0), 8.0, cos_inner=0.9, cos_outer=0.8)
    out = lights_ref.inject(n, g0, E, ao, nm, [spot])
    assert out[3, 1, 3].view(np.uint32).tolist() == [0, 0, 0, F(1.0).view(np.uint32)]
    # the same spot shining down lights it fully (cd = 1, s = 1)
    down = vct.spot_light(above, (0.0, -1.0, 0.0), (2.0, 2.0, 2.0), 8.0, cos_inner=0.9, cos_outer=0.8)
    assert bits_equal(lights_ref.inject(n, g0, E, ao, nm, [down])[3, 1, 3], np.array([f, f, f, 1.0], F))
    # a wall voxel between them: V = 0
    ao2, nm2 = ao.copy(), nm.copy()
    ao2[3, 4, 3] = (0.5, 0.5, 0.5, 1.0)
    stats = []
    sh = lights_ref.inject(n, g0, E, ao2, nm2, [vct.point_light(above, (2.0, 2.0, 2.0), 8.0)], stats)
    assert sh[3, 1, 3].view(np.uint32).tolist() == [0, 0, 0, F(1.0).view(np.uint32)]
    assert 1 <= stats[0]["blocked"] <= 9                                   # it and at most its 8 neighbours
    assert bits_equal(sh[0, 1, 0], r0[0, 1, 0]) and sh[0, 1, 0, 0] > 0     # a far voxel is still lit
    # a light exactly at a receiver's q: r2 = 0, skipped
    stats = []
    at_q = lights_ref.inject(n, g0, E, ao, nm, [vct.point_light((3.5, 2.5, 3.5), (2.0, 2.0, 2.0), 8.0)], stats)
    assert stats[0]["zero"] == 1 and at_q[3, 1, 3, 0] == 0
    # no light: dark, alpha 1 at the occupied voxels
    dark = lights_ref.inject(n, g0, E, ao, nm, [])
    assert bits_equal(dark[..., 3], (ao[..., 3] != 0).astype(F)) and not dark[..., :3].any()


def test_order_is_part_of_the_result():
    """The sum runs in list order: S reversed differs in the last bit of some voxels."""
    c = lights_ref.cornell(32)
    g = c["grid"]
    rev = lights_ref.inject(32, c["g0"], c["E"], g["albedo_occ"], g["normal"], c["lights"][::-1])
    assert not bits_equal(rev, c["level0"])
    assert np.allclose(rev, c["level0"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("n", [16, 32])
def test_coverage_of_the_gpu_inputs(oracle_mod, n):
    check_coverage(n)
