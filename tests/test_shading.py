"""include/vct_shading.h without a GPU: tests/shading_ref.py (the numpy restatement of vct_spec.h
"shading attributes") against gbuffer_ref where no attribute exists, against a float64
evaluation of the same formulas, and against the true normal of a sphere; then the header, the
bindings, vct.shading's host helpers and the loader's new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gbuffer_inputs as GI
import gbuffer_ref as GR
import shading_inputs as SI
import shading_ref as SR
import spec_ref

F = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# float32 reference against float64, largest |N32 - N64| per component over the compared pixels of
# the two anchor cases, as measured by test_float64_anchor (it prints them), and the bound: 4 x
# the larger one.  The float32 normalisation of a short interpolated vector carries the rounding
# of its square into every component, and the float32 barycentrics of a triangle seen at a grazing
# angle (the sphere's silhouette) move the interpolated vector by more than that.  N_BOUND = 7.72e-05.
MEASURED_SPHERE, MEASURED_QUAD = 1.81e-05, 1.93e-05
N_BOUND = 4 * max(MEASURED_SPHERE, MEASURED_QUAD)
LEFT_OUT_MAX = 0.025


def test_fmaf32_is_spec_refs_fmaf():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(4000).astype(F) for _ in range(3))
    c[:2000] = (-a[:2000] * b[:2000]).astype(F) + c[:2000] * F(1e-7)           # cancellation: the ties live here
    a[-4:], b[-4:], c[-4:] = (np.inf, np.nan, 3e38, 1e-30), (1.0, 1.0, 3e38, 1e-30), (-np.inf, 0.0, 0.0, 1e-45)
    got = SR.fmaf32(a, b, c)
    want = np.array([spec_ref.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], F)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all()


def test_identity_without_attributes():
    """With every attribute absent the reference is gbuffer_ref.planes, bit for bit, on the stage;
    alb4.w is the material's roughness (here the call's), ks4 the table's Ks."""
    m = GI.stage()
    verts, idx, tri_mat, kd, _ = m.arrays()
    rec = GR.k1_skip(GR.tri_records(verts, idx), verts, idx, GI.N, GI.G0, GI.E)
    mats = [SI.material(ks=(0.25 + t % 3, 0.5, 1.0 / (1 + t)), roughness=GI.ROUGH) for t in range(m.n_tri)]
    at = SR.Attrs(m.n_tri, mats, tri_mat)
    for cam, w, h in ((GI.look(), 67, 45), (GI.look(position=(0.2, -0.3, 0.5), yaw=-120.0, pitch=20.0), 64, 48)):
        hit, best, d = GR.nearest_hit(rec, cam, w, h)
        want = GR.planes(rec, kd[tri_mat][:, :3], cam, w, h, GI.ROUGH, hit, best, d)
        got = SR.planes(rec, kd[tri_mat][:, :3], cam, w, h, GI.ROUGH, at, hit=hit, best=best, d=d)
        for name, a in zip(("pos", "nrm", "alb"), want):
            assert np.array_equal(got[name].view(np.uint32), a.view(np.uint32)), name
        assert np.array_equal(got["geo"].view(np.uint32), want[1].view(np.uint32))
        lit = want[0][..., 3] != 0
        assert lit.sum() > 1000
        assert np.array_equal(got["tri_id"][lit], hit[lit].astype(np.uint32)) and (got["tri_id"][~lit] == SR.NO_HIT).all()
        ks = np.array([mm.ks for mm in mats], F)[hit[lit]]
        assert np.array_equal(got["ks"][lit][:, :3], ks) and (got["ks"][lit][:, 3] == 1).all() and not got["ks"][~lit].any()


def _anchor(case, thr=1e-4):
    """(largest |N32 - N64| over the compared pixels, the share of lit pixels left out, N32, N64,
    the compared mask) of a case: float32 reference against the float64 evaluation."""
    rec, kd, at = SR.case_arrays(case)
    p32 = SR.case_planes(case)
    p64 = SR.planes64(rec, case.cam, case.w, case.h, SI.ROUGH, at, case.textures)
    lit = p64["valid"]
    keep = lit & GR.robust(p64["r"], thr)
    assert np.array_equal(p32["tri_id"][keep].astype(np.int64), p64["hit"][keep])    # what `robust` promises
    diff = np.abs(p32["nrm"][..., :3].astype(np.float64) - p64["N"])[keep]
    return float(diff.max()), 1.0 - keep.sum() / lit.sum(), p32, p64, keep


@pytest.mark.parametrize("which", ["sphere", "quad"])
def test_float64_anchor(which):
    """The float32 reference against the same formulas in float64, on an icosphere of level 2
    (vertex normals = normalised positions) and on the normal-mapped quads and boxes.  Only the
    pixels gbuffer_ref.robust rejects are left out, at most 2.5 %."""
    case = SI.sphere(2, False, 64, 48) if which == "sphere" else SI.maps_case(70, 45)
    worst, left_out, p32, p64, keep = _anchor(case)
    print(f"{case.name}: max |N32 - N64| = {worst:.3e}, bound {N_BOUND:.3e}, left out {100 * left_out:.2f} %")
    assert left_out <= LEFT_OUT_MAX
    assert keep.sum() > 1000
    assert worst <= N_BOUND
    measured = MEASURED_SPHERE if which == "sphere" else MEASURED_QUAD
    assert worst <= measured * 1.0001, "the recorded measurement is stale"
    assert np.abs(p32["ks"][..., :3].astype(np.float64) - p64["ks"])[keep].max() <= N_BOUND
    assert np.array_equal(p32["alb"][..., 3][keep].astype(np.float64), p64["alb_w"][keep])


def test_smooth_normals_are_nearer_the_true_normal():
    """On the sphere the mean angle between N and the radial normal is strictly smaller shaded
    than flat."""
    for level in (1, 2):
        p = SR.case_planes(SI.sphere(level, False, 64, 48))
        lit = p["pos"][..., 3] != 0
        radial = p["pos"][lit][:, :3].astype(np.float64)
        radial /= np.linalg.norm(radial, axis=-1, keepdims=True)
        ang = lambda n: np.degrees(np.arccos(np.clip((n[lit][:, :3].astype(np.float64) * radial).sum(-1), -1, 1))).mean()
        shaded, flat = ang(p["nrm"]), ang(p["geo"])
        print(f"level {level}: mean angle to the radial normal {shaded:.3f} deg shaded, {flat:.3f} deg flat")
        assert shaded < flat and shaded < 0.25 * flat


def test_hostile_cases_in_the_reference():
    """What each hostile case is about shows in the reference: nothing non-finite is written, the
    fallbacks give Ng, a stale map is no map, the dynamic triangle gets the flat record."""
    by = {c.name: c for c in SI.hostile_cases()}
    for c in by.values():
        p = SR.case_planes(c)
        lit = p["pos"][..., 3] != 0
        assert lit.sum() >= c.min_hits and np.isfinite(p["nrm"]).all() and np.isfinite(p["ks"]).all(), c.name
        assert np.allclose(np.linalg.norm(p["nrm"][lit][:, :3], axis=-1), 1.0, atol=1e-6)
    p = SR.case_planes(by["hostile_normals"])
    for quad in range(5):                       # zero, NaN, Inf, denormal, overflow: N0 = Ng
        px = (p["tri_id"] // 2 == quad)
        assert px.sum() > 100 and np.array_equal(p["nrm"][px], p["geo"][px])
    p = SR.case_planes(by["hostile_frames"])
    for quad in (1, 5):                         # N1 = 0 falls back to N0 = Ng; a normal facing away gives Ng
        px = (p["tri_id"] // 2 == quad)
        assert px.sum() > 100 and np.array_equal(p["nrm"][px], p["geo"][px])
    p = SR.case_planes(by["stale_map"])
    px = (p["tri_id"] // 2 == 1) | (p["tri_id"] // 2 == 4)          # material 1: its map index 2 is stale
    assert px.sum() > 100 and np.array_equal(p["nrm"][px], p["geo"][px])
    px = (p["tri_id"] // 2 == 0)                                    # material 0: normal map 0 lives, specular map 1 is stale
    assert (p["nrm"][px] != p["geo"][px]).any() and (p["ks"][px][:, :3] == np.array((0.9, 0.8, 0.7), F)).all()
    c = by["dynamic_in_front"]
    p = SR.case_planes(c)
    px = p["tri_id"] == c.idx.size // 3
    assert px.sum() > 100 and np.array_equal(p["nrm"][px], p["geo"][px]) and (p["ks"][px] == 1).all()
    assert (p["alb"][px][:, 3] == F(SI.ROUGH)).all()


def test_header_abi_and_bindings():
    from vct import VctShadingDesc, VctShadingMaterial, _lib
    sh = open(os.path.join(REPO, "include", "vct_shading.h")).read()
    vct_h = open(os.path.join(REPO, "include", "vct.h")).read()
    assert vct_h.count('#include "vct_shading.h"') == 1 and re.search(r"#define\s+VCT_ABI_VERSION\s+1\b", vct_h)
    assert int(re.search(r"#define VCT_SHADING_NO_ATTR\s+0x([0-9A-F]+)u", sh).group(1), 16) == _lib.VCT_SHADING_NO_ATTR
    assert int(re.search(r"#define VCT_SHADING_FLIP_GREEN (\d+)u", sh).group(1)) == _lib.VCT_SHADING_FLIP_GREEN == 1
    assert C.sizeof(VctShadingMaterial) == 32 and C.sizeof(VctShadingDesc) == 72
    assert _lib.SHADING_EXTENSIONS == ("vct_set_shading", "vct_gbuffer_shaded_device", "vct_specular_tint_device")
    for name in _lib.SHADING_EXTENSIONS:
        assert re.search(r"\b%s\(" % name, sh), name
        assert name not in _lib.EXPORTS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vct_[a-z0-9_]+)", out))
    assert set(_lib.SHADING_EXTENSIONS) <= exported
    lib = _lib.load()
    assert lib.vct_abi_version() == 1
    for name in _lib.SHADING_EXTENSIONS:
        assert _lib.bind_shading_extension(lib, name).restype is C.c_int32
    # a NULL context is VCT_EINVAL from all three, before anything is touched
    assert _lib.bind_shading_extension(lib, "vct_set_shading")(None, None) == 1
    assert _lib.bind_shading_extension(lib, "vct_specular_tint_device")(None, None, None, 1, 1, None) == 1
    assert _lib.bind_shading_extension(lib, "vct_gbuffer_shaded_device")(None, None, 1, 1, 0.1, *[None] * 7) == 1


def test_roughness_from_ns():
    from vct.shading import roughness_from_ns
    assert roughness_from_ns(0) == 1.0
    assert roughness_from_ns(96.078431) == pytest.approx((2.0 / 98.078431) ** 0.5, rel=1e-12)     # nanosuit.mtl's Ns
    assert roughness_from_ns(96.078431) == pytest.approx(0.14280, abs=1e-5)
    assert 0.0 < roughness_from_ns(1e9) < 5e-5
    assert roughness_from_ns(-1.5) == 1.0 and roughness_from_ns(np.inf) == 0.0


def test_smooth_welds_spheres_and_keeps_boxes():
    from vct.scenes import Scene, _icosphere
    from vct.shading import smooth
    s = Scene("t")
    m = s.material((0.5, 0.5, 0.5))
    T = _icosphere(1) * 0.5 + np.array([0.25, 0.0, 0.0])
    for t in T:
        s.tri(t[0], t[1], t[2], m, uv=[(0, 0), (1, 0), (0, 1)])
    s.box((-1.5, -0.5, -0.5), (-0.75, 0.25, 0.5), m)
    flat, idx, mat, kd = s.arrays()
    v, idx2, mat2, kd2 = smooth(s)
    assert np.array_equal(idx, idx2) and np.array_equal(mat, mat2) and np.array_equal(kd, kd2)
    assert np.array_equal(v[:, :3], flat[:, :3]) and np.array_equal(v[:, 6:8], flat[:, 6:8])
    ns = 3 * T.shape[0]
    radial = (flat[:ns, :3] - np.array([0.25, 0, 0], F)) / 0.5
    assert np.abs(v[:ns, 3:6] - radial).max() < 0.02                      # the sphere: the radial normal
    assert np.abs(v[ns:, 3:6] - flat[ns:, 3:6]).max() < 1e-6               # the box: its face normals
    n, t, b = v[:, 3:6].astype(np.float64), v[:, 8:11].astype(np.float64), v[:, 11:14].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-6) and np.allclose(np.linalg.norm(t, axis=1), 1, atol=1e-6)
    # the box's frames: T = dP/du, B = dP/dv of its [0, 1]^2 faces, orthogonal to N
    assert np.abs((n[ns:] * t[ns:]).sum(1)).max() < 1e-6 and np.abs((n[ns:] * b[ns:]).sum(1)).max() < 1e-6
    assert np.abs((t[ns:] * b[ns:]).sum(1)).max() < 1e-6


def _write_png(path, rgba):
    import importlib.util
    spec = importlib.util.spec_from_file_location("mtg", os.path.join(REPO, "tests", "golden", "make_tex_golden.py"))
    mtg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mtg)
    path.write_bytes(mtg.write_png(rgba.astype(np.int64), 6, 8))


def test_loader_shading_slots(tmp_path):
    """A hand-written OBJ/MTL with Ns, Ks, map_Ks, map_Kn and map_Bump: each slot's path and decoded
    texture, in the list of their own; the diffuse list and its count are what they were."""
    import host_lib
    lib = host_lib.load()
    P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    lib.vcth_material_shininess.argtypes = [P, u32, C.POINTER(C.c_float)]
    lib.vcth_material_shading_map.argtypes = [P, u32, C.c_int, C.POINTER(C.c_char_p), C.POINTER(i32)]
    lib.vcth_num_shading_textures.argtypes = [P]
    lib.vcth_num_shading_textures.restype = u32
    lib.vcth_shading_texture.argtypes = [P, u32, C.POINTER(P), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_char_p)]
    lib.vcth_num_shading_texture_errors.argtypes = [P]
    lib.vcth_num_shading_texture_errors.restype = u32
    lib.vcth_num_textures.argtypes = [P]
    lib.vcth_num_textures.restype = u32
    lib.vcth_num_texture_errors.argtypes = [P]
    lib.vcth_num_texture_errors.restype = u32
    lib.vcth_material_diffuse_map.argtypes = [P, u32, C.POINTER(C.c_char_p), C.POINTER(i32)]
    files = {"d.png": SI.TEX_4x4, "s.png": SI.TEX_3x5, "n.png": SI.TEX_WHITE, "b.png": SI.TEX_4x4[::-1].copy()}
    for name, t in files.items():
        _write_png(tmp_path / name, t)
    (tmp_path / "m.obj").write_text("mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0 1\nvn 0 0 1\n"
                                    "usemtl a\nf 1/1/1 2/2/1 3/3/1\nusemtl b\nf 1/1/1 3/3/1 2/2/1\n")
    (tmp_path / "m.mtl").write_text(
        "newmtl a\nNs 96.078431\nKd 0.64 0.64 0.64\nKs 0.5 0.25 0.125\nmap_Kd d.png\nmap_Ks s.png\nmap_Kn n.png\n"
        "map_Bump -bm 0.5 b.png\n\n"
        "newmtl b\nKs 1 1 1\nmap_Ks s.png\nbump b.png\nmap_Kn missing.png\n")
    h = P()
    err = C.create_string_buffer(256)
    assert lib.vcth_load_obj(str(tmp_path / "m.obj").encode(), C.byref(h), err, 256) == 0, err.value
    try:
        names = {}
        for i in range(lib.vcth_num_materials(h)):
            nm = C.c_char_p()
            ks = np.zeros(4, F)
            lib.vcth_material(h, i, C.byref(nm), None, None, host_lib.fptr(ks))
            names[nm.value.decode()] = (i, ks)
        a, b = names["a"][0], names["b"][0]
        assert np.array_equal(names["a"][1], np.array([0.5, 0.25, 0.125, 1], F))

        def slot(i, s):
            path, tex = C.c_char_p(), i32(-7)
            assert lib.vcth_material_shading_map(h, i, s, C.byref(path), C.byref(tex)) == 0
            return path.value.decode(), tex.value

        def texture(i):
            px, w, hh, path = P(), u32(), u32(), C.c_char_p()
            assert lib.vcth_shading_texture(h, i, C.byref(px), C.byref(w), C.byref(hh), C.byref(path)) == 0
            t = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_uint8)), (hh.value, w.value, 4)).copy()
            return path.value.decode(), t

        ns = C.c_float(-1)
        assert lib.vcth_material_shininess(h, a, C.byref(ns)) == 0 and ns.value == F(96.078431)
        assert lib.vcth_material_shininess(h, b, C.byref(ns)) == 0 and ns.value == 0.0
        SPEC, NORMAL, HEIGHT = 0, 1, 2
        for i, want in ((a, {SPEC: "s.png", NORMAL: "n.png", HEIGHT: "b.png"}), (b, {SPEC: "s.png", NORMAL: "missing.png", HEIGHT: "b.png"})):
            for s, name in want.items():
                path, tex = slot(i, s)
                assert path == name
                if name == "missing.png":
                    assert tex == -1
                else:
                    got_path, t = texture(tex)
                    assert got_path == name and np.array_equal(t, files[name]), (i, s)
        assert slot(a, SPEC)[1] == slot(b, SPEC)[1] and slot(a, HEIGHT)[1] == slot(b, HEIGHT)[1]      # loaded once per path
        assert lib.vcth_num_shading_textures(h) == 3 and lib.vcth_num_shading_texture_errors(h) == 1
        assert lib.vcth_material_shading_map(h, a, 3, None, None) == -1 and lib.vcth_shading_texture(h, 3, None, None, None, None) == -1
        # the diffuse list: one texture, one index, no error, as before
        assert lib.vcth_num_textures(h) == 1 and lib.vcth_num_texture_errors(h) == 0
        path, tex = C.c_char_p(), i32(-7)
        assert lib.vcth_material_diffuse_map(h, a, C.byref(path), C.byref(tex)) == 0 and (path.value, tex.value) == (b"d.png", 0)
        assert lib.vcth_material_diffuse_map(h, b, C.byref(path), C.byref(tex)) == 0 and (path.value, tex.value) == (b"", -1)
    finally:
        lib.vcth_free(h)
