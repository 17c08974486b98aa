"""Host-side helpers of the shading G-buffer (include/vct_shading.h).

* :class:`ShadingMaterial`: one row of ``vct_set_shading``'s material table;
* :func:`roughness_from_ns`: the Phong exponent ``Ns`` of a .mtl as a roughness, the usual
  Blinn-Phong conversion (a host convention: the library takes any roughness in [0, 1]);
* :func:`smooth`: a scene's arrays with area-weighted vertex normals and per-vertex tangents and
  bitangents from the TexCoords -- what assimp's ``aiProcess_GenSmoothNormals |
  aiProcess_CalcTangentSpace`` hands the reference for a model file.  The synthetic scenes emit
  flat per-corner normals and no tangents; the showroom's sphere gets its smooth stand-in here.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._lib import VCT_SHADING_FLIP_GREEN, VctShadingMaterial

NORMAL_OFFSET, UV_OFFSET, TANGENT_OFFSET, BITANGENT_OFFSET = 12, 24, 32, 44   # bytes in the 56-byte Vertex


@dataclass
class ShadingMaterial:
    ks: tuple = (1.0, 1.0, 1.0)
    roughness: float = 0.1
    normal_map: int = -1          # index into the set_textures list, or -1
    specular_map: int = -1
    flip_green: bool = False

    def to_ctypes(self) -> VctShadingMaterial:
        m = VctShadingMaterial()
        m.ks[:] = [float(x) for x in self.ks]
        m.roughness = float(self.roughness)
        m.normal_map, m.specular_map = int(self.normal_map), int(self.specular_map)
        m.flags = VCT_SHADING_FLIP_GREEN if self.flip_green else 0
        m.reserved = 0
        return m


def set_flat(ctx, verts, idx, roughness: float) -> None:
    """A shading set with every attribute absent and one material of the call's roughness and
    Ks 1, on the static mesh (verts, idx) that `ctx` was voxelized with.  With it
    vct_gbuffer_shaded_device equals vct_gbuffer_raster_device in every bit of pos4, nrm4 and
    alb4 (vct_spec.h "shading attributes", last clause): the way to get the pass's tri_id and
    bary2 planes -- what include/vct_motion.h reads -- for a scene without smooth normals."""
    ctx.set_shading(verts, idx, None, [ShadingMaterial(roughness=roughness)], normal_offset=None, uv_offset=None,
                    tangent_offset=None, bitangent_offset=None)


def roughness_from_ns(ns) -> float:
    """clip(sqrt(2 / (ns + 2)), 0, 1): Ns = 0 is fully rough, a large Ns a mirror."""
    with np.errstate(all="ignore"):
        return float(np.clip(np.sqrt(2.0 / (np.float64(ns) + 2.0)), 0.0, 1.0))


def smooth(scene, crease_deg: float = 45.0, weld: float = 1e-6):
    """(verts [V, 14] float32, idx, tri_mat, kd4) of `scene` (anything with ``arrays()``, or such
    a tuple) with Normal = the area-weighted mean of the face normals around the corner's
    position, and Tangent / Bitangent = the same mean of the faces' UV-derived tangent frames.
    Corners are welded by position (rounded to `weld`); a corner takes the faces around its
    position whose normal is within `crease_deg` of its own face's, so boxes stay boxes.
    Positions, TexCoords, indices and materials are returned as they are."""
    verts, idx, tri_mat, kd = scene.arrays() if hasattr(scene, "arrays") else scene
    verts = np.array(verts, np.float32)
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    P = verts[:, :3].astype(np.float64)[tri]                      # [T, 3, 3]
    UV = verts[:, 6:8].astype(np.float64)[tri]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    fn = np.cross(e1, e2)                                         # length = 2 area: the weight
    d1, d2 = UV[:, 1] - UV[:, 0], UV[:, 2] - UV[:, 0]
    det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
    with np.errstate(all="ignore"):
        r = np.where(det != 0, 1.0 / np.where(det != 0, det, 1.0), 0.0)[:, None]
    ft = (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) * r                  # dP/du
    fb = (e2 * d1[:, 0:1] - e1 * d2[:, 0:1]) * r                  # dP/dv
    area = np.linalg.norm(fn, axis=-1, keepdims=True)
    unit = lambda v: v / np.where(np.linalg.norm(v, axis=-1, keepdims=True) > 0,
                                  np.linalg.norm(v, axis=-1, keepdims=True), 1.0)
    fnu, ftu, fbu = unit(fn), unit(ft), unit(fb)
    key = np.round(P.reshape(-1, 3) / weld).astype(np.int64)
    _, group = np.unique(key, axis=0, return_inverse=True)
    group = group.reshape(-1)
    # every pair (corner i, corner j) of one position: corners sorted by group, each paired with
    # its group's whole run
    n = group.size
    order = np.argsort(group, kind="stable")
    cnt = np.bincount(group)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    per = cnt[group[order]]                                       # partners of each sorted corner
    first = np.repeat(np.arange(n), per)
    within = np.arange(int(per.sum())) - np.repeat(np.cumsum(per) - per, per)
    ci, cj = order[first], order[np.repeat(start[group[order]], per) + within]
    fi, fj = ci // 3, cj // 3
    near = (fnu[fi] * fnu[fj]).sum(-1) >= np.cos(np.radians(crease_deg))
    mean = lambda f: unit(np.stack([np.bincount(ci, weights=f[fj, c] * near, minlength=n) for c in range(3)], -1))
    N, T, B = mean(fn), mean(ftu * area), mean(fbu * area)
    # a vertex shared through the index array takes the last corner's value: unshared corners
    # (every synthetic scene) keep their own
    out = verts.copy()
    flat = tri.reshape(-1)
    out[flat, 3:6] = N.reshape(-1, 3)
    out[flat, 8:11] = T.reshape(-1, 3)
    out[flat, 11:14] = B.reshape(-1, 3)
    return out, np.asarray(idx, np.uint32), np.asarray(tri_mat, np.uint32), np.asarray(kd, np.float32)
