"""The loader's side of the alpha cutouts (include/vct_host.h, vct/cutout.py) on the CPU: `d` and
`map_d` of a hand-written OBJ/MTL with 1-, 3- and 4-channel PNGs, the new getters, the host rule
of vct.cutout.cutouts_from_model, and the existing getters on the golden models, unchanged."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import host_lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "obj_*.npz")))
F = np.float32
P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32


def encode_png(a):
    """vcth_encode_png of an (H, W, comp) uint8 array -> the file's bytes."""
    lib = host_lib.load()
    lib.vcth_encode_png.argtypes = [C.c_void_p, u32, u32, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t),
                                    C.c_char_p, C.c_int]
    lib.vcth_free_image.argtypes = [C.c_void_p]
    a = np.ascontiguousarray(a, np.uint8)
    out, n, err = C.POINTER(C.c_uint8)(), C.c_size_t(), C.create_string_buffer(128)
    assert lib.vcth_encode_png(a.ctypes.data, a.shape[1], a.shape[0], a.shape[2], C.byref(out), C.byref(n), err, 128) == 0, err.value
    data = bytes(bytearray(out[:n.value]))
    lib.vcth_free_image(out)
    return data


def write_model(d):
    """An OBJ/MTL with d, map_d (with options), and masks of 1, 3 and 4 channels -> the .obj path
    and the images by file name."""
    rng = np.random.default_rng(4)
    files = {
        "leaf_rgba.png": rng.integers(0, 256, (4, 4, 4)),        # map_Kd with an alpha channel
        "mask_grey.png": rng.integers(0, 256, (3, 5, 1)),        # map_d, one channel
        "mask_rgb.png": rng.integers(0, 256, (2, 2, 3)),         # map_d, three channels
        "mask_rgba.png": rng.integers(0, 256, (4, 2, 4)),        # map_d, four channels
        "wall_rgb.png": rng.integers(0, 256, (2, 3, 3)),         # map_Kd without alpha
    }
    for name, a in files.items():
        (d / name).write_bytes(encode_png(a))
    faces = "".join(f"usemtl {m}\nf 1/1/1 2/2/1 3/3/1\n" for m in ("leaf", "grey", "rgb", "rgba", "wall", "plain", "gone"))
    # the wall stands behind the masked quad of the headless frame (z = -1 against z = 0)
    (d / "m.obj").write_text("mtllib m.mtl\nv -1 -1 0\nv 1 -1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 0.5 1\nvn 0 0 1\n" + faces)
    (d / "m.mtl").write_text(
        "newmtl leaf\nKd 0.5 0.6 0.7\nd 0.25\nmap_Kd leaf_rgba.png\n\n"
        "newmtl grey\nKd 1 1 1\nmap_d -clamp on -o 0.1 0.2 0.3 mask_grey.png\n\n"
        "newmtl rgb\nmap_d mask_rgb.png\nmap_Kd leaf_rgba.png\n\n"
        "newmtl rgba\nd 1.0\nmap_d -mm 0 1 mask_rgba.png\nmap_Ks mask_grey.png\n\n"
        "newmtl wall\nmap_Kd wall_rgb.png\n\n"
        "newmtl plain\nKd 0.1 0.2 0.3\n\n"
        "newmtl gone\nmap_d missing.png\n")
    return d / "m.obj", files


def expand(a):
    """The loader's expansion to RGBA8: GL_RED / GL_RGB sample as (r, 0, 0, 255) / (r, g, b, 255)."""
    a = np.asarray(a, np.uint8)
    out = np.zeros(a.shape[:2] + (4,), np.uint8)
    out[..., 3] = 255
    out[..., :a.shape[2]] = a
    return out


def test_d_map_d_and_the_host_rule(tmp_path):
    from vct.cutout import HostModel, OPAQUE, cutouts_from_model
    obj, files = write_model(tmp_path)
    m = HostModel.load(obj)
    by = {x.name: x for x in m.materials}
    assert [by[n].dissolve for n in ("leaf", "grey", "rgba", "plain")] == [0.25, 1.0, 1.0, 1.0]     # default 1
    # the diffuse list is what it was: map_Kd only, each path once; channels before expansion
    assert len(m.textures) == 2 and m.channels == [4, 3]
    assert np.array_equal(m.textures[0], expand(files["leaf_rgba.png"])) and np.array_equal(m.textures[1], expand(files["wall_rgb.png"]))
    assert by["leaf"].diffuse_map == by["rgb"].diffuse_map == 0 and by["wall"].diffuse_map == 1 and by["grey"].diffuse_map == -1
    # map_d: the option skipping of the other maps, a slot of the shading list, loaded once per path
    sh = {n: by[n].opacity_map for n in by}
    assert sh["leaf"] == sh["wall"] == sh["plain"] == sh["gone"] == -1                            # missing.png failed to load
    assert sorted((sh["grey"], sh["rgb"], sh["rgba"])) == [0, 1, 2]
    for n, f in (("grey", "mask_grey.png"), ("rgb", "mask_rgb.png"), ("rgba", "mask_rgba.png")):
        assert np.array_equal(m.shading_textures[sh[n]], expand(files[f])), n
        assert m.shading_channels[sh[n]] == files[f].shape[2]
    assert len(m.shading_textures) == 3                      # map_Ks mask_grey.png shares map_d's texture
    # the rule: map_d with 4 channels -> 3; with 1 or 3 -> 0; no map_d, a 4-channel map_Kd -> it, 3
    table = dict(zip([x.name for x in m.materials], cutouts_from_model(m, 0.375)))
    base = len(m.textures)
    assert table["leaf"] == (0, 3, 0.375)
    assert table["grey"] == (base + sh["grey"], 0, 0.375) and table["rgb"] == (base + sh["rgb"], 0, 0.375)
    assert table["rgba"] == (base + sh["rgba"], 3, 0.375)
    assert table["wall"] == table["plain"] == table["gone"] == OPAQUE
    assert len(m.all_textures) == 5 and cutouts_from_model(m)[m.materials.index(by["leaf"])][2] == 0.5
    assert m.verts.shape == (21, 14) and m.idx.size == 21 and m.tri_material.size == 7 and m.kd4.shape == (len(m.materials), 4)


def test_new_getters_and_the_three_slot_getter(tmp_path):
    """vcth_material_opacity_map, vcth_material_dissolve and the channel getters; the errors of
    the shading list name the missing map_d; vcth_material_shading_map keeps its three slots."""
    lib = host_lib.load()
    obj, _ = write_model(tmp_path)
    lib.vcth_material_opacity_map.argtypes = [P, u32, C.POINTER(C.c_char_p), C.POINTER(i32)]
    lib.vcth_material_dissolve.argtypes = [P, u32, C.POINTER(C.c_float)]
    lib.vcth_texture_channels.argtypes = [P, u32, C.POINTER(C.c_int)]
    lib.vcth_shading_texture_channels.argtypes = [P, u32, C.POINTER(C.c_int)]
    lib.vcth_material_shading_map.argtypes = [P, u32, C.c_int, C.POINTER(C.c_char_p), C.POINTER(i32)]
    lib.vcth_num_shading_texture_errors.argtypes = [P]
    lib.vcth_num_shading_texture_errors.restype = u32
    lib.vcth_shading_texture_error.argtypes = [P, u32]
    lib.vcth_shading_texture_error.restype = C.c_char_p
    h, err = P(), C.create_string_buffer(256)
    assert lib.vcth_load_obj(str(obj).encode(), C.byref(h), err, 256) == 0, err.value
    try:
        names = []
        for i in range(lib.vcth_num_materials(h)):
            nm = C.c_char_p()
            lib.vcth_material(h, i, C.byref(nm), None, None, None)
            names.append(nm.value.decode())
        path, tex, d, comp = C.c_char_p(), i32(-7), C.c_float(-1), C.c_int(-1)
        want = {"leaf": b"", "grey": b"mask_grey.png", "rgb": b"mask_rgb.png", "rgba": b"mask_rgba.png", "gone": b"missing.png"}
        for n, p in want.items():
            assert lib.vcth_material_opacity_map(h, names.index(n), C.byref(path), C.byref(tex)) == 0 and path.value == p, n
            assert (tex.value >= 0) == (n in ("grey", "rgb", "rgba"))
        assert lib.vcth_material_dissolve(h, names.index("leaf"), C.byref(d)) == 0 and d.value == 0.25
        assert lib.vcth_material_dissolve(h, 99, C.byref(d)) == -1 and lib.vcth_material_opacity_map(h, 99, None, None) == -1
        assert lib.vcth_texture_channels(h, 0, C.byref(comp)) == 0 and comp.value == 4
        assert lib.vcth_texture_channels(h, 2, C.byref(comp)) == -1 and lib.vcth_shading_texture_channels(h, 3, C.byref(comp)) == -1
        assert lib.vcth_num_shading_texture_errors(h) == 1 and lib.vcth_shading_texture_error(h, 0).startswith(b"missing.png")
        assert lib.vcth_material_shading_map(h, 0, 3, None, None) == -1          # three slots, as before
        assert lib.vcth_material_shading_map(h, names.index("rgba"), 0, C.byref(path), C.byref(tex)) == 0 and path.value == b"mask_grey.png"
    finally:
        lib.vcth_free(h)


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[4:-4] for p in GOLDEN])
def test_existing_getters_on_the_golden_models(tmp_path, path):
    """Materials, maps and meshes of the golden models are what the goldens record; none of them has
    a map_d, so no material is masked and d is read where the .mtl has it."""
    from vct.cutout import HostModel, OPAQUE, cutouts_from_model
    g = np.load(path)
    (tmp_path / "scene.mtl").write_bytes(g["mtl"].tobytes())
    obj = tmp_path / "model.obj"
    obj.write_bytes(g["obj"].tobytes())
    m = HostModel.load(obj)
    assert [x.name for x in m.materials] == g["mat_names"].tobytes().decode().split("\n")
    assert np.array_equal(m.kd4, g["mat_kd"])
    n = k = 0                                                 # vertices and indices before mesh i
    for i in range(int(g["n_meshes"])):
        ref_v, ref_i = g["mesh%d_verts" % i], g["mesh%d_idx" % i]
        assert np.array_equal(m.verts[n:n + ref_v.shape[0]], ref_v, equal_nan=True), i
        assert np.array_equal(m.idx[k:k + ref_i.size], ref_i + np.uint32(n)), i
        assert (m.tri_material[k // 3:(k + ref_i.size) // 3] == int(g["mesh%d_mat" % i])).all(), i
        n, k = n + ref_v.shape[0], k + ref_i.size
    assert all(x.opacity_map == -1 for x in m.materials)
    mtl = g["mtl"].tobytes().decode(errors="replace")
    if "map_d" not in mtl and not m.textures:
        assert cutouts_from_model(m) == [OPAQUE] * len(m.materials)
