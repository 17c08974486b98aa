"""Inputs of the shading G-buffer (vct_spec.h "shading attributes"; test infrastructure): named
cases (mesh with vertex attributes, material table, textures, camera, frame size), benign and
hostile.  tests/test_shading.py checks the reference on them on the CPU, tests/test_shading_gpu.py
the HIP pass against the reference; tests/shading_ref.py is the reference.

Every mesh is voxelized into the same small grid (N = 32 over [-2, 2]^3): the G-buffer passes read
the mesh records of the last voxelize call, the grid itself is not looked at.  Vertices are the
reference's 56-byte Vertex (14 floats): Position, Normal 3:6, TexCoords 6:8, Tangent 8:11,
Bitangent 11:14.  Kd is distinct per material, so the albedo plane names the material.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import gbuffer_inputs as GI

F = np.float32
N, G0, E = 32, (-2.0, -2.0, -2.0), 4.0
ROUGH = 0.1                                 # the call's roughness: background and flat records
FRAMES = ((70, 45), (64, 48))               # partial and whole 16-pixel tiles


def _rgba(h, w, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    t[..., 2] |= 0x80                        # a normal map's blue: m.z > 0
    return t


TEX_4x4, TEX_3x5 = _rgba(4, 4, 1), _rgba(5, 3, 2)      # (H, W, 4): 4 x 4 and 3 wide x 5 high
TEX_WHITE = np.full((1, 1, 4), 255, np.uint8)          # m = (1, 1, 1)
TEXTURES = [TEX_4x4, TEX_3x5, TEX_WHITE]


def material(ks=(1.0, 1.0, 1.0), roughness=0.1, normal_map=-1, specular_map=-1, flip_green=False):
    from vct.shading import ShadingMaterial
    return ShadingMaterial(ks, roughness, normal_map, specular_map, flip_green)


@dataclass
class Case:
    name: str
    verts: np.ndarray                 # [V, 14] float32
    idx: np.ndarray                   # [3T] uint32
    tri_mat: np.ndarray               # [T] uint32: the material of K1 (Kd) and of the set
    materials: list                   # ShadingMaterial per material
    cam: GI.Cam
    w: int
    h: int
    textures: list = field(default_factory=list)
    present: dict = field(default_factory=lambda: dict(normal=True, uv=True, tangent=True, bitangent=True))
    n_tex_after: int | None = None    # a smaller vct_set_textures after vct_set_shading: stale indices
    dynamic: tuple | None = None      # (verts, idx) of a dynamic layer voxelized after the set
    min_hits: int = 200

    @property
    def kd4(self):
        m = np.arange(len(self.materials))
        return np.stack([(m % 4 + 1) / 4, (m // 4 % 4 + 1) / 4, (m // 16 + 1) / 4, np.ones(len(m))], 1).astype(F)

    def offsets(self):
        """set_shading's four offsets (None: absent)."""
        off = dict(normal=12, uv=24, tangent=32, bitangent=44)
        return {f"{k}_offset": (off[k] if self.present[k] else None) for k in off}


def _verts(P, normal=None, uv=None, tangent=None, bitangent=None):
    """[T, 3, 14] rows from per-corner arrays ([T, 3, c] or broadcastable)."""
    P = np.asarray(P, np.float64)
    v = np.zeros(P.shape[:2] + (14,), F)
    with np.errstate(all="ignore"):
        v[..., :3] = P
        for sl, a in ((slice(3, 6), normal), (slice(6, 8), uv), (slice(8, 11), tangent), (slice(11, 14), bitangent)):
            if a is not None:
                v[..., sl] = np.broadcast_to(np.asarray(a, np.float64), v[..., sl].shape)
    return v


def _case(name, v, tri_mat, materials, cam, w, h, **kw):
    v = v.reshape(-1, 14)
    return Case(name, v, np.arange(v.shape[0], dtype=np.uint32), np.asarray(tri_mat, np.uint32), materials, cam, w, h, **kw)


# ---------------------------------------------------------------------------
# smooth normals: icospheres, vertex normal = normalised position
# ---------------------------------------------------------------------------
OUTSIDE = dict(position=(0.3, 0.2, 2.6), yaw=-96.0, pitch=-4.0)
INSIDE = dict(position=(0.15, -0.1, 0.2), yaw=-60.0, pitch=25.0)


def sphere(level, inside, w, h, zoom=45.0):
    from vct.scenes import _icosphere
    T = _icosphere(level)
    cam = GI.look(**(INSIDE if inside else OUTSIDE), zoom=zoom)
    mats = [material(ks=(0.8, 0.6, 0.4), roughness=0.35)]
    name = f"sphere{level}_{'inside' if inside else 'outside'}_{w}x{h}"
    return _case(name, _verts(T, normal=T), np.zeros(T.shape[0]), mats, cam, w, h,
                 present=dict(normal=True, uv=False, tangent=False, bitangent=False))


def smooth_cases():
    return [sphere(1, False, 70, 45), sphere(2, False, 64, 48), sphere(1, True, 64, 48), sphere(2, True, 70, 45)]


# ---------------------------------------------------------------------------
# maps: a quad and a box with per-face TexCoords, frames from vct.shading.smooth
# ---------------------------------------------------------------------------
MAP_MATERIALS = lambda: [
    material(ks=(0.9, 0.7, 0.5), roughness=0.2, normal_map=0, specular_map=1),               # 4 x 4 normal, 3 x 5 specular
    material(ks=(0.5, 0.5, 1.0), roughness=0.6, normal_map=1, flip_green=True),               # 3 x 5 normal, green flipped
    material(ks=(0.25, 1.0, 0.75), roughness=0.05, specular_map=0),                           # specular map alone
    material(ks=(1.0, 0.0, 0.125), roughness=1.0),                                            # no map
    material(ks=(0.3, 0.3, 0.3), roughness=0.4, normal_map=0, flip_green=True),               # 4 x 4, green flipped
]


def maps_case(w, h, cam=None):
    from vct.scenes import Scene, _box_uv
    from vct.shading import smooth
    s = Scene("maps")
    for _ in range(5):
        s.material((0.5, 0.5, 0.5))
    # a back wall whose TexCoords leave [0, 1] and go negative, in two materials
    s.quad((-1.6, -1.2, -1.0), (0.0, -1.2, -1.0), (0.0, 1.2, -1.0), (-1.6, 1.2, -1.0), (0, 0, 1), 0,
           uv=[(-0.5, -0.25), (1.5, -0.25), (1.5, 1.75), (-0.5, 1.75)])
    s.quad((0.0, -1.2, -1.0), (1.6, -1.2, -1.0), (1.6, 1.2, -1.0), (0.0, 1.2, -1.0), (0, 0, 1), 1,
           uv=[(-2.25, 0.0), (0.75, 0.0), (0.75, 3.0), (-2.25, 3.0)])
    _box_uv(s, (-0.9, -0.8, -0.4), (-0.2, -0.1, 0.3), 2)
    _box_uv(s, (0.2, -0.7, -0.5), (0.8, 0.2, 0.2), 4)
    s.quad((-1.6, -1.2, -1.0), (1.6, -1.2, -1.0), (1.6, -1.2, 1.0), (-1.6, -1.2, 1.0), (0, 1, 0), 3)
    v, i, m, _ = smooth(s)
    cam = cam or GI.look(position=(0.2, 0.4, 2.4), yaw=-94.0, pitch=-12.0)
    return Case(f"maps_{w}x{h}", v, i, m, MAP_MATERIALS(), cam, w, h, textures=TEXTURES[:2])


# ---------------------------------------------------------------------------
# hostile attributes: a wall of quads facing the camera, one finding each
# ---------------------------------------------------------------------------
def _wall(cells):
    """cells: per quad dict(normal, uv, tangent, bitangent, mat) -> [2 len, 3, 14]; quad j spans
    x in [-1.5 + 0.5 j, -1.0 + 0.5 j], y in [-0.5, 0.5] at z = 0, facing +z."""
    out, mats = [], []
    for j, c in enumerate(cells):
        x0, x1 = -1.5 + 0.5 * j, -1.0 + 0.5 * j
        q = np.array([[(x0, -0.5, 0), (x1, -0.5, 0), (x1, 0.5, 0)], [(x0, -0.5, 0), (x1, 0.5, 0), (x0, 0.5, 0)]])
        uv = c.get("uv", np.array([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], np.float64))
        out.append(_verts(q, c.get("normal", (0, 0, 1)), uv, c.get("tangent", (1, 0, 0)), c.get("bitangent", (0, 1, 0))))
        mats += [c.get("mat", 0)] * 2
    return np.concatenate(out), mats


HOSTILE_MATERIALS = lambda: [
    material(ks=(0.9, 0.8, 0.7), roughness=0.3, normal_map=0, specular_map=1),   # 0: mapped
    material(ks=(0.6, 0.6, 0.6), roughness=0.5, normal_map=2),                   # 1: the white texel: m = (1, 1, 1)
    material(ks=(0.2, 0.4, 0.6), roughness=0.7),                                 # 2: unmapped
]


def hostile_normals(w=70, h=45):
    """Zero, NaN, Inf and denormal normals, and normals whose square overflows: N0 = Ng for all
    but the denormal ones' neighbours; a mixed quad (one bad vertex) too."""
    big = 1e30
    mixed = np.array([[(0, 0, 1), (np.nan, 0, 1), (0, 0, 1)], [(0, 0, 1), (0, 0, 1), (0, 0, 1)]])
    cells = [dict(normal=(0, 0, 0), mat=2), dict(normal=(np.nan, 0, 1), mat=2), dict(normal=(0, np.inf, 1), mat=2),
             dict(normal=(0, 0, 1e-40), mat=2), dict(normal=(big, big, big), mat=2), dict(normal=mixed, mat=0)]
    v, mats = _wall(cells)
    return _case("hostile_normals", v, mats, HOSTILE_MATERIALS(), GI.look(position=(0.0, 0.0, 2.2)), w, h, textures=TEXTURES)


def hostile_frames(w=64, h=48):
    """Under a map: zero tangents; T, B, N coplanar so that N1 = 0 (m = (1, 1, 1), T = -N, B = 0);
    NaN and Inf TexCoords; Inf tangents; a shading normal facing away (vertex normals -z)."""
    nan_uv = np.full((2, 3, 2), np.nan)
    inf_uv = np.array([[(np.inf, 0), (1, -np.inf), (1, 1)], [(0, 0), (1, 1), (0, 1)]])
    cells = [dict(tangent=(0, 0, 0), bitangent=(0, 0, 0), mat=0),
             dict(tangent=(0, 0, -1), bitangent=(0, 0, 0), mat=1),
             dict(uv=nan_uv, mat=0), dict(uv=inf_uv, mat=0),
             dict(tangent=(np.inf, 0, 0), mat=0),
             dict(normal=(0, 0, -1), mat=2)]
    v, mats = _wall(cells)
    return _case("hostile_frames", v, mats, HOSTILE_MATERIALS(), GI.look(position=(0.0, 0.0, 2.2)), w, h, textures=TEXTURES)


def stale_map(w=64, h=48):
    """Map indices 1 and 2 made stale by a one-texture vct_set_textures after vct_set_shading:
    a stale map is no map; index 0 stays mapped."""
    v, mats = _wall([dict(mat=0), dict(mat=1), dict(mat=2), dict(mat=0), dict(mat=1), dict(mat=2)])
    return _case("stale_map", v, mats, HOSTILE_MATERIALS(), GI.look(position=(0.0, 0.0, 2.2)), w, h, textures=TEXTURES,
                 n_tex_after=1)


def k1_skipped(w=70, h=45):
    """A triangle K1 skips (a NaN position: an all-zero mesh record, never hit) in the middle of
    the set: the records behind it keep their indices."""
    v, mats = _wall([dict(mat=0), dict(mat=2), dict(mat=1), dict(mat=0)])
    with np.errstate(all="ignore"):
        v[2, 1, 0] = np.nan
    return _case("k1_skipped", v, mats, HOSTILE_MATERIALS(), GI.look(position=(0.0, 0.0, 2.2)), w, h, textures=TEXTURES)


def dynamic_in_front(w=70, h=45):
    """A dynamic-layer triangle in front of shaded quads: the flat record where it wins."""
    v, mats = _wall([dict(mat=0), dict(mat=2), dict(mat=1), dict(mat=0), dict(mat=2), dict(mat=1)])
    dyn = _verts(np.array([[(-0.8, -0.3, 0.5), (0.9, -0.4, 0.6), (0.1, 0.45, 0.4)]]), normal=(0.6, 0, 0.8)).reshape(-1, 14)
    return _case("dynamic_in_front", v, mats, HOSTILE_MATERIALS(), GI.look(position=(0.0, 0.0, 2.2)), w, h,
                 textures=TEXTURES, dynamic=(dyn, np.arange(3, dtype=np.uint32)))


def hostile_cases():
    return [hostile_normals(), hostile_frames(), stale_map(), k1_skipped(), dynamic_in_front()]


def all_cases():
    c = smooth_cases() + [maps_case(70, 45), maps_case(64, 48, GI.look(position=(-0.4, 0.1, 2.0), yaw=-80.0, pitch=-8.0))]
    c += hostile_cases()
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c
