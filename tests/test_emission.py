"""Emissive surfaces without a GPU: the boundary declares and binds the six functions of
include/vct_emission.h, a library without them (the CPU oracle backend) still loads, and the
reference the GPU tests compare against (tests/emission_ref.py, a composition of oracle calls
and a numpy restatement of vct_spec.h "emissive surfaces") gives closed-form answers and the
input classes the GPU tests rely on.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import emission_ref as R
from emission_ref import bits_equal

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("vct_voxelize_emission", "vct_voxelize_emission_device", "vct_emission_voxels", "vct_download_emission",
         "vct_inject_emission", "vct_composite_emissive_device")

# What the reference gave when the tests were written.  Literals, so that an edit of the
# reference cannot quietly empty a class the GPU tests are meant to cover.
LAMP = {16: {"occupied": 1142, "emissive": 64, "only": 36, "mixed": 28},
        32: {"occupied": 5890, "emissive": 256, "only": 196, "mixed": 60},
        64: {"occupied": 33691, "emissive": 2048, "only": 1800, "mixed": 248}}
GIANT = {16: 830, 32: 4266, 64: 22162}                     # material 0 and the lamp both emit
SUBSET = {16: (28, 36), 32: (60, 196)}                     # the lamp quad alone over the open box: kept, dropped
FLOATING = {16: 9, 32: 28, 64: 86}                         # hit voxels of the floating triangle, none occupied
SOUP = {16: {"emissive": 1664, "multi": 618, "mixed": 396}, 32: {"emissive": 6336, "multi": 896, "mixed": 526}}
HOSTILE = {(16, "exact"): 913, (16, "unit"): 880, (32, "exact"): 3236, (32, "unit"): 3191}
HOSTILE_FAMILIES = ("lattice", "degenerate", "sliver", "outside", "nonfinite", "counts")
GIANT_KE = (1.0, 0.5, 2.0)                                 # Ke of material 0 in the giant-triangle case


# ---- the inputs the CPU and GPU tests share ---------------------------------------------
def giant_case(n):
    """The lamp scene with material 0 (floor, ceiling, back wall, boxes) emitting too."""
    L = R.lamp(n)
    ke = L["ke"].copy()
    ke[0, :3] = GIANT_KE
    return L["arrays"], ke, L["grid"]["counts"], L["g0"], L["E"]


def subset_case(n, O):
    """The open scenes.cornell() voxelized; the lamp quad's two triangles as emitter geometry."""
    from vct import scenes
    L = R.lamp(n)
    arrays = scenes.cornell().arrays()
    _, counts = O.voxelize(n, L["g0"], L["E"], *arrays)
    v, i, m, _ = L["arrays"]
    sel = np.flatnonzero(m == L["lamp"])
    return arrays, counts, (v, i.reshape(-1, 3)[sel].reshape(-1), m[sel], L["ke"])


def floating_case():
    v = np.zeros((3, 14), F)
    v[:, :3] = R.FLOATING
    return v, np.arange(3, dtype=np.uint32), None, np.array([[1.0, 1.0, 1.0, 0.0]], F)


def soup_case(n, O):
    from vct import scenes
    arrays = scenes.random_triangles(300).arrays()
    g0, E = scenes.grid_for_unit_box(n)
    _, counts = O.voxelize(n, g0, E, *arrays)
    ke = np.zeros((4, 4), F)
    ke[:, :3] = R.SOUP_KE
    return arrays, counts, (np.arange(300) % 4).astype(np.uint32), ke, g0, E


def hostile_case(n, placement, O):
    import voxel_inputs
    mesh = voxel_inputs.build(HOSTILE_FAMILIES, n, placement)
    _, counts = O.voxelize(n, mesh.g0, mesh.E, mesh.verts, mesh.idx, mesh.mat, mesh.kd)
    return mesh, counts, R.hostile_ke(mesh.mat.size)


# ---- the boundary ------------------------------------------------------------------------
def test_header_and_spec_declare_the_functions():
    src = open(os.path.join(REPO, "include", "vct_emission.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(rf"vct_status\s+{name}\s*\(\s*vct_ctx\s*\*", code), name
    assert re.search(r"vct_inject_emission\s*\(\s*vct_ctx\s*\*\s*\w*\s*,\s*float\s+\w+\s*\)\s*;", code)
    for text in ("vct_load_grid", "vct_save_grid", "VCT_ESTATE", "VCT_EINVAL", "Call order"):
        assert text in src, text
    vct_h = open(os.path.join(REPO, "include", "vct.h")).read()
    assert vct_h.count('#include "vct_emission.h"') == 1
    assert re.search(r"#define\s+VCT_ABI_VERSION\s+1\b", vct_h)
    assert not any(name in vct_h for name in NAMES)                 # one #include line and nothing else
    spec = open(os.path.join(REPO, "include", "vct_spec.h")).read()
    assert "emissive surfaces" in spec
    m = re.search(r"#define\s+VCT_EMISSION_SCALE_LIMIT\s+(\S+?)f\b", spec)
    assert m and F(m.group(1)) == F(2.0 ** 111)
    for text in ("vct_load_grid", "vct_save_grid", "2^111"):
        assert text in spec.split("emissive surfaces", 1)[1], text


def test_binding_lists_them_and_hip_library_exports_them():
    from vct import Context, VctLight, _lib
    assert _lib.EMISSION_EXTENSIONS == NAMES
    # the other lists are as they were
    assert _lib.EXTENSIONS == ("vct_inject_bounces", "vct_bounce_sources")
    assert _lib.LIGHT_EXTENSIONS == ("vct_inject_lights", "vct_composite_lights_device")
    assert _lib.SHADOW_EXTENSIONS == ("vct_shadow_cones_device", "vct_composite_shadowed_device")
    assert len(_lib.EXPORTS) == 52 and not set(NAMES) & set(_lib.EXPORTS)
    for method in ("voxelize_emission", "voxelize_emission_device", "emission_voxels", "download_emission",
                   "inject_emission", "composite_emissive_device"):
        assert callable(getattr(Context, method)), method
    assert _lib.VCT_EMISSION_SCALE_LIMIT == 2.0 ** 111
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vct_[a-z0-9_]+)", out))
    assert set(NAMES) <= exported
    assert lib.vct_abi_version() == 1
    # VCT_EINVAL for a NULL ctx, no device needed
    bind = _lib.bind_emission_extension
    assert bind(lib, "vct_voxelize_emission")(None, None, 56, 0, None, 0, None, None, 0) == 1
    assert bind(lib, "vct_voxelize_emission_device")(None, None, 56, 0, None, 0, None, None, 0) == 1
    assert bind(lib, "vct_emission_voxels")(None, None) == 1
    assert bind(lib, "vct_download_emission")(None, None) == 1
    assert bind(lib, "vct_inject_emission")(None, 1.0) == 1
    one = (VctLight * 1)()
    assert bind(lib, "vct_composite_emissive_device")(None, None, None, None, None, None, 4, 4, one, 1, None, 1.0,
                                                      None, None) == 1


def test_library_without_them_still_loads(oracle_mod):
    """The CPU backend exports vct.h only: it binds, runs, and refuses the new calls by name."""
    from helpers import scene_arrays
    from vct import Context, _lib, scenes
    cpu = _lib.bind(C.CDLL(oracle_mod.CPU_BACKEND))
    for name in NAMES:
        assert not hasattr(cpu, name)
        with pytest.raises(AttributeError, match=name):
            _lib.bind_emission_extension(cpu, name)
    s, (v, i, m, k) = scene_arrays("cornell")
    g0, E = scenes.grid_for_unit_box(16)
    ctx = Context(16, g0, E, lib=cpu)
    ctx.voxelize(v, i, m, k)
    ctx.inject_directional(scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
    before = ctx.download_level(0)
    with pytest.raises(AttributeError, match="vct_voxelize_emission"):
        ctx.voxelize_emission(v, i, m, np.zeros((3, 4), F))
    with pytest.raises(AttributeError, match="vct_inject_emission"):
        ctx.inject_emission(1.0)
    with pytest.raises(AttributeError, match="vct_composite_emissive_device"):
        ctx.composite_emissive_device(0, 0, 0, 0, 0, 4, 4, [])
    assert np.array_equal(ctx.download_level(0), before)
    ctx.close()


# ---- the reference -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 32, 64])
def test_closed_forms_on_the_lamp(oracle_mod, n):
    """A voxel only lamp triangles touch has E == float32(Ke) per channel (17, 12, 4 are exact);
    a voxel with k lamp hits among count has E == float32(k Ke / count)."""
    L = R.lamp(n)
    em, counts = L["em"], L["grid"]["counts"]
    E = em["E"].reshape(-1, 4)
    e = em["emissive"].reshape(-1)
    only = e & (em["hits"] == counts)
    assert np.all(E[only, :3] == np.array(R.LAMP_KE, F)) and np.all(E[e, 3] == 1.0)
    k = em["hits"][e].astype(np.float64)
    want = (k[:, None] * np.array(R.LAMP_KE, np.float64)[None, :] / counts[e].astype(np.float64)[:, None]).astype(F)
    assert bits_equal(E[e, :3], want)
    mixed = e & (em["hits"] < counts)
    assert np.all(E[mixed, :3] < np.array(R.LAMP_KE, F))
    assert not E[~e].view(np.uint32).any()                                # +0 in all four channels elsewhere
    assert np.all(counts[e] > 0)
    # the emissive voxels are the layer(s) of the ceiling plane over the hole
    z, y, x = np.nonzero(em["emissive"])
    q = (1.0 - L["g0"][1]) * n / L["E"]
    assert set(y.tolist()) <= {int(np.floor(q)) - 1, int(np.floor(q))}


@pytest.mark.parametrize("n", [16, 32, 64])
def test_coverage_of_the_lamp_and_giant_cases(oracle_mod, n):
    L = R.lamp(n)
    got = dict(L["classes"], occupied=int((L["grid"]["counts"] > 0).sum()))
    print(n, got)
    assert {k: got[k] for k in LAMP[n]} == LAMP[n]
    assert got["only"] + got["mixed"] == got["emissive"] and got["dropped"] == 0
    arrays, ke, counts, g0, E = giant_case(n)
    giant = R.classes(R.emission(oracle_mod, n, g0, E, counts, arrays[0], arrays[1], arrays[2], ke), counts)
    print(n, giant)
    assert giant["emissive"] == GIANT[n]
    from vct import scenes
    open_box = scenes.cornell().arrays()
    _, oc = oracle_mod.voxelize(n, g0, E, *open_box)
    fl = R.emission(oracle_mod, n, g0, E, oc, *floating_case())
    assert int((fl["hits"] > 0).sum()) == FLOATING[n] == fl["dropped"] and not fl["emissive"].any()
    if n == 32:                                                           # every class a GPU test relies on
        assert min(got["only"], got["mixed"], giant["mixed"], giant["multi"]) >= 20


@pytest.mark.parametrize("n", [16, 32])
def test_coverage_of_the_subset_soup_and_hostile_cases(oracle_mod, n):
    import voxel_inputs
    arrays, counts, emit = subset_case(n, oracle_mod)
    L = R.lamp(n)
    sub = R.classes(R.emission(oracle_mod, n, L["g0"], L["E"], counts, *emit), counts)
    print(n, sub)
    assert (sub["emissive"], sub["dropped"]) == SUBSET[n]
    arrays, counts, mat, ke, g0, E = soup_case(n, oracle_mod)
    soup = R.classes(R.emission(oracle_mod, n, g0, E, counts, arrays[0], arrays[1], mat, ke), counts)
    print(n, soup)
    assert {k: soup[k] for k in SOUP[n]} == SOUP[n]
    for placement in voxel_inputs.PLACEMENTS:
        mesh, counts, ke = hostile_case(n, placement, oracle_mod)
        assert np.all(ke[2::3] == 0) and np.all(ke[0::3, 0] > 0)
        em = R.emission(oracle_mod, n, mesh.g0, mesh.E, counts, mesh.verts, mesh.idx, mesh.mat, ke)
        print(n, placement, R.classes(em, counts))
        assert int(em["emissive"].sum()) == HOSTILE[(n, placement)]
        assert np.isfinite(em["E"]).all()
    if n == 32:
        assert min(sub["emissive"], sub["dropped"], soup["multi"], soup["mixed"]) >= 20


def test_level0_lookup_and_composite_known_answers():
    """A 4^3 grid of unit voxels with one emissive voxel (x, y, z) = (1, 2, 3), E = (2, 0.5, 0)."""
    n, g0, E = 4, (0.0, 0.0, 0.0), 4.0
    grid = np.zeros((n, n, n, 4), F)
    grid[3, 2, 1] = (2.0, 0.5, 0.0, 1.0)
    r0 = np.zeros((n, n, n, 4), F)
    r0[3, 2, 1] = (0.25, 0.25, 0.25, 1.0)
    r0[0, 0, 0] = (1.0, 1.0, 1.0, 1.0)
    out = R.add_to_level0(r0, grid, 0.5)
    assert out[3, 2, 1].tolist() == [1.25, 0.5, 0.25, 1.0] and bits_equal(out[0, 0, 0], r0[0, 0, 0])
    assert bits_equal(R.add_to_level0(r0, grid, 0.0), r0)
    nan, inf = float("nan"), float("inf")
    pos = np.array([[(1.5, 2.5, 3.5, 1.0), (1.0, 2.0, 3.0, 1.0), (1.999, 2.999, 3.999, 1.0), (2.0, 2.5, 3.5, 1.0),
                     (1.5, 2.5, 4.0, 1.0), (-0.5, 2.5, 3.5, 1.0), (nan, 2.5, 3.5, 1.0), (1.5, inf, 3.5, 1.0),
                     (1.5, 2.5, 3.5, 0.0)]], F)
    Em, hit = R.lookup(n, g0, E, grid, pos)
    assert hit[0].tolist() == [True, True, True, False, False, False, False, False, False]
    assert np.all(Em[0, :3] == np.array([2.0, 0.5, 0.0], F)) and not Em[0, 3:].view(np.uint32).any()
    base = np.full((1, 9, 4), 0.125, F)
    got = R.composite(base, pos, Em, 2.0)
    assert got[0, 0].tolist() == [4.125, 1.125, 0.125, 0.125]
    assert bits_equal(got[0, 3:], base[0, 3:])                            # +0 added, background untouched
    assert bits_equal(R.composite(base, pos, Em, 0.0), base)
