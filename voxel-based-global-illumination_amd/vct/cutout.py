"""Host-side helpers of the alpha cutouts (include/vct_cutout.h).

* :class:`HostModel`: an OBJ/MTL through the C++ host's loader (``libvct_host.so``,
  include/vct_host.h): the flattened arrays, the diffuse and the shading texture lists with
  their channel counts, and per material ``d``, ``map_Kd`` and ``map_d``;
* :func:`cutouts_from_model`: the cutout table of such a model by the rule of vct_host.h --
  a ``map_d`` with four channels is read in channel 3, with one or three in channel 0; without a
  ``map_d`` a four-channel ``map_Kd`` is read in channel 3; every other material is opaque.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

HOST_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvct_host.so")
OPAQUE = (-1, 0, 0.5)


@dataclass
class HostMaterial:
    name: str
    kd: tuple
    dissolve: float = 1.0
    diffuse_map: int = -1         # index into HostModel.textures, or -1
    opacity_map: int = -1         # index into HostModel.shading_textures, or -1


@dataclass
class HostModel:
    """What a cutout table needs of a loaded model.  `textures` / `shading_textures`: (H, W, 4)
    uint8 arrays; `channels` / `shading_channels`: each file's channel count before expansion."""
    verts: np.ndarray = None
    idx: np.ndarray = None
    tri_material: np.ndarray = None
    materials: list = field(default_factory=list)
    textures: list = field(default_factory=list)
    channels: list = field(default_factory=list)
    shading_textures: list = field(default_factory=list)
    shading_channels: list = field(default_factory=list)

    @property
    def kd4(self):
        return np.array([m.kd for m in self.materials], np.float32).reshape(-1, 4)

    @property
    def material_map(self):
        return np.array([m.diffuse_map for m in self.materials], np.int32)

    @property
    def all_textures(self):
        """The one list vct_set_textures takes: the diffuse list, then the shading list."""
        return list(self.textures) + list(self.shading_textures)

    @staticmethod
    def load(path, lib_path=HOST_LIB) -> "HostModel":
        lib = C.CDLL(lib_path)
        P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
        sig = {
            "vcth_load_obj": (C.c_int, [C.c_char_p, C.POINTER(P), C.c_char_p, C.c_int]),
            "vcth_free": (None, [P]),
            "vcth_num_meshes": (u32, [P]), "vcth_num_materials": (u32, [P]),
            "vcth_num_textures": (u32, [P]), "vcth_num_shading_textures": (u32, [P]),
            "vcth_mesh": (C.c_int, [P, u32, C.POINTER(P), C.POINTER(u32), C.POINTER(P), C.POINTER(u32), C.POINTER(u32)]),
            "vcth_material": (C.c_int, [P, u32, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                        C.POINTER(C.c_float)]),
            "vcth_material_diffuse_map": (C.c_int, [P, u32, C.POINTER(C.c_char_p), C.POINTER(i32)]),
            "vcth_material_opacity_map": (C.c_int, [P, u32, C.POINTER(C.c_char_p), C.POINTER(i32)]),
            "vcth_material_dissolve": (C.c_int, [P, u32, C.POINTER(C.c_float)]),
            "vcth_texture": (C.c_int, [P, u32, C.POINTER(P), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_char_p)]),
            "vcth_shading_texture": (C.c_int, [P, u32, C.POINTER(P), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_char_p)]),
            "vcth_texture_channels": (C.c_int, [P, u32, C.POINTER(C.c_int)]),
            "vcth_shading_texture_channels": (C.c_int, [P, u32, C.POINTER(C.c_int)]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        h = P()
        err = C.create_string_buffer(256)
        if lib.vcth_load_obj(os.fsencode(str(path)), C.byref(h), err, 256) != 0:
            raise RuntimeError(err.value.decode())
        try:
            out = HostModel()
            vs, ids, tms, base = [], [], [], 0
            for i in range(lib.vcth_num_meshes(h)):
                vp, ip, nv, ni, mat = P(), P(), u32(), u32(), u32()
                lib.vcth_mesh(h, i, C.byref(vp), C.byref(nv), C.byref(ip), C.byref(ni), C.byref(mat))
                if nv.value:
                    vs.append(np.ctypeslib.as_array(C.cast(vp, C.POINTER(C.c_float)), (nv.value * 14,)).reshape(-1, 14).copy())
                if ni.value:
                    ids.append(np.ctypeslib.as_array(C.cast(ip, C.POINTER(C.c_uint32)), (ni.value,)).copy() + np.uint32(base))
                    tms.append(np.full(ni.value // 3, mat.value, np.uint32))
                base += nv.value
            out.verts = np.concatenate(vs) if vs else np.zeros((0, 14), np.float32)
            out.idx = np.concatenate(ids) if ids else np.zeros(0, np.uint32)
            out.tri_material = np.concatenate(tms) if tms else np.zeros(0, np.uint32)
            for i in range(lib.vcth_num_materials(h)):
                name, kd, d, tex, op = C.c_char_p(), (C.c_float * 4)(), C.c_float(1.0), i32(-1), i32(-1)
                lib.vcth_material(h, i, C.byref(name), None, kd, None)
                lib.vcth_material_dissolve(h, i, C.byref(d))
                lib.vcth_material_diffuse_map(h, i, None, C.byref(tex))
                lib.vcth_material_opacity_map(h, i, None, C.byref(op))
                out.materials.append(HostMaterial((name.value or b"").decode(), tuple(kd), d.value, tex.value, op.value))
            for count, get, chan, tl, cl in (
                    (lib.vcth_num_textures, lib.vcth_texture, lib.vcth_texture_channels, out.textures, out.channels),
                    (lib.vcth_num_shading_textures, lib.vcth_shading_texture, lib.vcth_shading_texture_channels,
                     out.shading_textures, out.shading_channels)):
                for i in range(count(h)):
                    px, w, hh, comp = P(), u32(), u32(), C.c_int()
                    get(h, i, C.byref(px), C.byref(w), C.byref(hh), None)
                    chan(h, i, C.byref(comp))
                    tl.append(np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_uint8)), (hh.value, w.value, 4)).copy())
                    cl.append(comp.value)
            return out
        finally:
            lib.vcth_free(h)


def cutouts_from_model(model, cutoff: float = 0.5):
    """The cutout table of a HostModel (anything with its `materials`, `textures`, `channels`,
    `shading_channels`): one (map, channel, cutoff) per material, the map an index into
    `model.all_textures` (the shading list follows the diffuse list)."""
    base = len(model.textures)
    table = []
    for m in model.materials:
        if m.opacity_map >= 0:
            table.append((base + m.opacity_map, 3 if model.shading_channels[m.opacity_map] == 4 else 0, float(cutoff)))
        elif m.diffuse_map >= 0 and model.channels[m.diffuse_map] == 4:
            table.append((m.diffuse_map, 3, float(cutoff)))
        else:
            table.append(OPAQUE)
    return table
