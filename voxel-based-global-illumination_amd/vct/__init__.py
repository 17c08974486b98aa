"""vct — Python host mirror of the MI355X voxel-cone-tracing path.

The product is the C-ABI library ``libvct_hip.so`` (include/vct.h).  This
package is host plumbing around it, shaped like the reference's plug-in
surface:

* :class:`Context` wraps one ``vct_ctx`` (the state a reference ``Renderer``
  would own; renderer.h:3-10);
* :mod:`vct.camera` reproduces the reference FPS camera conventions
  (scene/camera.cpp:24-27, 73-83);
* :mod:`vct.scenes` builds synthetic scenes in the reference ``Vertex`` layout
  (include/stdafx.h:36-42, 56-byte records) with per-material Kd
  (scene/material.h:10), and the G-buffers of SURVEY.md 8d;
* :mod:`vct.multi` splits the cone trace over ranks (screen tiles, RCCL
  broadcast of level 0, gather of the frame).
The ``Renderer`` / ``ConeTraceRenderer`` slot and the name-keyed registry
(core/assets.h:17-20, assets.cpp:44, engine.cpp:151) are in the C++ host
(``host/renderer.h``, ``host/assets.h``).

Host arrays are numpy; device arrays are torch tensors (torch is used only for
device memory, streams and torch.distributed).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import VCT_ALL_RANKS, VctCamera, VctCommId, VctConfig, VctLight, VctSky, VctTexture, VctTraceArgs
from ._lib import VCT_CONES_DIFFUSE, VCT_CONES_SPECULAR, VctMixedHoles, VctMixedParams
from ._lib import VctFog
from ._lib import VctTemporalArgs, VctTemporalParams
from ._lib import VctCone, VctConeQueryArgs, VctProbeGrid
from ._lib import VctVoxelPickArgs, VctVoxelViewArgs
from ._lib import VctEnvSky
from ._lib import VctShadingDesc, VctShadingMaterial
from ._lib import VctCutout
from ._lib import VctBloomParams, VctExposureParams, VctExposureState, VctPresentParams

__all__ = ["VctShadingMaterial","VctEnvSky", "env_sky", "VctTemporalParams","Context", "VctError", "VctConfig", "VctCamera", "tiles_for_rank", "tile_offset", "VERTEX_FLOATS",
           "VCT_ALL_RANKS", "comm_frame_layout", "VctLight", "directional_light", "point_light", "spot_light",
           "VctSky", "sky_light", "VctFog", "fog", "VctCone", "VctProbeGrid", "probe_grid", "VctMixedParams", "VctMixedHoles", "VCT_CONES_DIFFUSE", "VCT_CONES_SPECULAR"]

VERTEX_FLOATS = 14          # reference Vertex: Position, Normal, TexCoords, Tangent, Bitangent
VERTEX_STRIDE = VERTEX_FLOATS * 4
UV_OFFSET = 24              # offsetof(Vertex, TexCoords) (stdafx.h:36-42, mesh.cpp:49)


class VctError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{_lib.STATUS.get(status, status)}: {msg}")
        self.status = status


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def directional_light(dir_to_light, color=(1.0, 1.0, 1.0)) -> VctLight:
    """A vct_light of type VCT_LIGHT_DIRECTIONAL: `dir_to_light` as inject_directional takes it."""
    l = VctLight()
    l.type = _lib.VCT_LIGHT_DIRECTIONAL
    l.direction, l.color = _f3(dir_to_light), _f3(color)
    return l


def point_light(position, color=(1.0, 1.0, 1.0), range: float = 1.0) -> VctLight:
    """A vct_light of type VCT_LIGHT_POINT at world `position`; no light at distance >= range."""
    l = VctLight()
    l.type = _lib.VCT_LIGHT_POINT
    l.position, l.color, l.range = _f3(position), _f3(color), float(range)
    return l


def spot_light(position, direction, color=(1.0, 1.0, 1.0), range: float = 1.0, inner_deg: float = 20.0,
               outer_deg: float = 30.0, cos_inner: float | None = None, cos_outer: float | None = None) -> VctLight:
    """A vct_light of type VCT_LIGHT_SPOT shining along `direction`: full intensity inside
    the half-angle inner_deg, none outside outer_deg.  The angles are degrees and become
    cosines in float32 (np.cos of the float32 radians); cos_inner / cos_outer give the
    cosines directly instead."""
    l = VctLight()
    l.type = _lib.VCT_LIGHT_SPOT
    l.position, l.direction, l.color, l.range = _f3(position), _f3(direction), _f3(color), float(range)
    l.cos_inner = float(np.cos(np.deg2rad(np.float32(inner_deg)))) if cos_inner is None else float(cos_inner)
    l.cos_outer = float(np.cos(np.deg2rad(np.float32(outer_deg)))) if cos_outer is None else float(cos_outer)
    return l


def sky_light(zenith, horizon=None, ground=None, up=(0.0, 1.0, 0.0)) -> VctSky:
    """A vct_sky: the colours straight up, at the horizon (default: the zenith's) and straight
    down (default: black), blended by the cosine to `up`."""
    s = VctSky()
    s.up, s.zenith = _f3(up), _f3(zenith)
    s.horizon = _f3(zenith if horizon is None else horizon)
    s.ground = _f3((0.0, 0.0, 0.0) if ground is None else ground)
    return s


def env_sky(frame=((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), scale: float = 1.0) -> VctEnvSky:
    """A vct_env_sky: `frame` holds the world directions of the map's x, y and z axes as rows
    (world -> map), `scale` the intensity.  The library checks the record's input rule when a
    call uses it."""
    e = VctEnvSky()
    for i, row in enumerate(frame):
        e.frame[i] = _f3(row)
    e.scale = float(scale)
    return e


def fog(density, albedo=(_lib.VCT_FOG_DEFAULT_ALBEDO,) * 3, ambient=0.0, level=_lib.VCT_FOG_DEFAULT_LEVEL,
        step=_lib.VCT_FOG_DEFAULT_STEP) -> VctFog:
    """A vct_fog: `density` is the extinction per world unit, `albedo` the single-scattering
    albedo, `ambient` the weight of the cone-traced indirect term (0: off), one cell of the
    scatter volume is 2^level voxels and the march steps `step` cells.  The fields are checked
    against the grid when a context uses the record (_lib.check_fog, the library's own rule)."""
    f = VctFog()
    f.density, f.albedo, f.ambient, f.level, f.step = float(density), _f3(albedo), float(ambient), int(level), float(step)
    return f


def probe_grid(origin, spacing, dims) -> VctProbeGrid:
    """A vct_probe_grid: probe (i, j, k) at origin + (i, j, k) * spacing, dims = (dx, dy, dz).  The
    library checks the record's input rule when a call uses it."""
    g = VctProbeGrid()
    g.origin, g.spacing = _f3(origin), float(spacing)
    g.dims = (C.c_uint32 * 3)(*[int(v) for v in dims])
    return g


def _light_array(lights):
    lights = list(lights)
    arr = (VctLight * max(len(lights), 1))()
    for i, l in enumerate(lights):
        if not isinstance(l, VctLight):
            raise VctError(_EINVAL, f"lights[{i}]: expected a VctLight (vct.point_light, ...), got {type(l).__name__}")
        arr[i] = l
    return arr, len(lights)


def tiles_for_rank(w: int, h: int, rank: int, world: int) -> int:
    return int(_lib.load().vct_tiles_for_rank(w, h, rank, world))


def tile_offset(w: int, h: int, rank: int, world: int) -> int:
    return int(_lib.load().vct_tile_offset(w, h, rank, world))


_EINVAL = 1
_F32 = ("torch.float32",)
_I32 = ("torch.int32", "torch.uint32")
_I64 = ("torch.int64", "torch.uint64")


class Context:
    """One vct_ctx: grid + pyramid resident in HBM of one GPU."""

    def __init__(self, n: int, aabb_min, extent: float, aniso: bool = True, n_diffuse: int = 9,
                 specular: bool = True, device: int = -1, lib=None, devices: int = 0):
        # lib: another implementation of include/vct.h bound with _lib.bind (tests use
        # the CPU oracle backend); default: the in-tree HIP library, no fallback.
        # devices > 0: one context over that many GPUs (vct_create_multi; screen tiles
        # traced on every device, gathered on device 0 by peer copies)
        self.lib = lib if lib is not None else _lib.load()
        cfg = VctConfig()
        cfg.n = n
        cfg.aabb_min = (C.c_float * 3)(*[float(x) for x in aabb_min])
        cfg.extent = float(extent)
        cfg.aniso = 1 if aniso else 0
        cfg.n_diffuse = n_diffuse
        cfg.specular = 1 if specular else 0
        cfg.device = device
        h = C.c_void_p()
        if devices > 0:
            st = self.lib.vct_create_multi(C.byref(cfg), devices, C.byref(h))
        else:
            st = self.lib.vct_create(C.byref(cfg), C.byref(h))
        if st != 0:
            raise VctError(st, "vct_create failed (is a HIP device visible?)")
        self.num_devices = int(self.lib.vct_num_devices(h))
        self.device = int(device)
        self.h = h
        self.n = n
        self.aniso = aniso
        self.n_diffuse = n_diffuse
        self.specular = specular
        self.aabb_min = tuple(float(x) for x in aabb_min)
        self.extent = float(extent)
        self.stream = 0          # the HIP stream of set_stream (0: the null stream)

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.vct_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st: int, what: str):
        if st != 0:
            err = self.lib.vct_last_error(self.h)
            raise VctError(st, f"{what}: {err.decode() if err else ''}")

    def _dev(self, t, name: str, dtypes=_F32, min_numel: int = 0):
        """Device pointer of a torch tensor after checking that the C-ABI may use it:
        a CUDA tensor on this context's device, of an accepted dtype, contiguous,
        with at least `min_numel` elements (an undersized output would be written
        out of bounds, a host tensor would fault the GPU).  None stays None; a raw
        int is taken as a device pointer the caller vouches for."""
        if t is None or isinstance(t, int):
            return t
        if not getattr(t, "is_cuda", False):
            raise VctError(_EINVAL, f"{name}: expected a device (cuda) tensor, got {getattr(t, 'device', type(t))}")
        if self.device >= 0 and t.device.index != self.device:
            raise VctError(_EINVAL, f"{name}: tensor on {t.device}, context on device {self.device}")
        if str(t.dtype) not in dtypes:
            raise VctError(_EINVAL, f"{name}: dtype {t.dtype}, expected one of {', '.join(dtypes)}")
        if not t.is_contiguous():
            raise VctError(_EINVAL, f"{name}: tensor is not contiguous")
        if t.numel() < min_numel:
            raise VctError(_EINVAL, f"{name}: {t.numel()} elements, needs at least {min_numel}")
        return t.data_ptr()

    def set_stream(self, stream_ptr: int | None):
        self._check(self.lib.vct_set_stream(self.h, C.c_void_p(stream_ptr or 0)), "set_stream")
        self.stream = stream_ptr or 0

    def synchronize(self):
        self._check(self.lib.vct_synchronize(self.h), "synchronize")

    @property
    def trace_form(self) -> int:
        """Kept candidate of the default cone trace for the current workload (vct_trace_form):
        bit 0 the form (0 union: bricks of up to six faces, 4 waves/SIMD; 1 occupancy, 5 waves/SIMD), bit 1
        ray reordering; -1 while still timing."""
        return int(self.lib.vct_trace_form(self.h))

    @property
    def num_levels(self) -> int:
        return int(self.lib.vct_num_levels(self.h))

    def level_dims(self, level: int):
        nl, nf = C.c_uint32(), C.c_uint32()
        self._check(self.lib.vct_level_dims(self.h, level, C.byref(nl), C.byref(nf)), "level_dims")
        return nl.value, nf.value

    # -- K1 / K2 / K3 -----------------------------------------------------
    def set_textures(self, textures):
        """Diffuse maps (vct_set_textures): a list of (H, W, 4) uint8 RGBA arrays, row 0 =
        the image's top row (stbi_load order); [] clears the set."""
        keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in textures]
        arr = (VctTexture * max(len(keep), 1))()
        for i, t in enumerate(keep):
            if t.ndim != 3 or t.shape[2] != 4:
                raise VctError(_EINVAL, f"set_textures: texture {i} must be [H, W, 4] uint8, got {t.shape}")
            arr[i].rgba8 = t.ctypes.data_as(C.c_void_p)
            arr[i].height, arr[i].width = t.shape[0], t.shape[1]
        self._check(self.lib.vct_set_textures(self.h, C.cast(arr, C.c_void_p), len(keep)), "set_textures")

    def voxelize(self, verts: np.ndarray, idx: np.ndarray, tri_material: np.ndarray | None = None,
                 kd4: np.ndarray | None = None, material_map: np.ndarray | None = None,
                 uv_offset: int = UV_OFFSET):
        """K1 (vct_voxelize).  With material_map (per material: set_textures index or -1)
        it is vct_voxelize_textured: albedo = Kd x diffuse map at the hit's TexCoords."""
        verts = np.ascontiguousarray(verts, dtype=np.float32)
        assert verts.ndim == 2 and verts.shape[1] >= 3
        stride = verts.shape[1] * 4
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        mat = None if tri_material is None else np.ascontiguousarray(tri_material, dtype=np.uint32).reshape(-1)
        kd = None if kd4 is None else np.ascontiguousarray(kd4, dtype=np.float32)
        mm = None if material_map is None else np.ascontiguousarray(material_map, dtype=np.int32).reshape(-1)
        if idx.size % 3:
            raise VctError(_EINVAL, f"voxelize: {idx.size} indices, not a multiple of 3")
        if mat is not None and mat.size != idx.size // 3:
            # vct_voxelize reads n_idx / 3 entries of tri_material
            raise VctError(_EINVAL, f"voxelize: tri_material has {mat.size} entries for {idx.size // 3} triangles")
        if kd is not None:
            if kd.ndim != 2 or kd.shape[1] != 4:
                raise VctError(_EINVAL, f"voxelize: kd4 must be [materials, 4], got {kd.shape}")
        n_mat = 0 if kd is None else kd.shape[0]
        if mm is None:
            st = self.lib.vct_voxelize(self.h, _fptr(verts), stride, verts.shape[0], _fptr(idx), idx.size,
                                       _fptr(mat) if mat is not None else None,
                                       _fptr(kd) if kd is not None else None, n_mat)
        else:
            if kd is not None and mm.size != n_mat:
                raise VctError(_EINVAL, f"voxelize: material_map has {mm.size} entries for {n_mat} materials")
            st = self.lib.vct_voxelize_textured(self.h, _fptr(verts), stride, verts.shape[0], _fptr(idx), idx.size,
                                                _fptr(mat) if mat is not None else None,
                                                _fptr(kd) if kd is not None else None, _fptr(mm), mm.size,
                                                uv_offset)
        self._check(st, "voxelize")

    def voxelize_device(self, verts, idx, tri_material=None, kd4=None, material_map=None, uv_offset=UV_OFFSET):
        """K1 on device-resident torch tensors: verts [V, F] float32 (F >= 3, the
        56-byte Vertex is F = 14), idx [3T] int32/uint32, tri_material [T] int32,
        kd4 [M, 4] float32, material_map [M] int32 (vct_voxelize_textured_device)."""
        if verts.dim() != 2 or verts.shape[1] < 3:
            raise VctError(_EINVAL, f"voxelize_device: verts must be [V, F >= 3], got {tuple(verts.shape)}")
        if str(idx.dtype) in _I64:
            # read as uint32 pairs, the triangles would silently collapse onto vertex 0
            raise VctError(_EINVAL, "voxelize_device: idx must be int32 / uint32, not 64-bit")
        n_idx = idx.numel()
        if n_idx % 3:
            raise VctError(_EINVAL, f"voxelize_device: {n_idx} indices, not a multiple of 3")
        if kd4 is not None and (kd4.dim() != 2 or kd4.shape[1] != 4):
            raise VctError(_EINVAL, f"voxelize_device: kd4 must be [materials, 4], got {tuple(kd4.shape)}")
        nm = 0 if kd4 is None else kd4.shape[0]
        args = (self.h, self._dev(verts, "verts"), verts.shape[1] * 4, verts.shape[0], self._dev(idx, "idx", _I32),
                n_idx, self._dev(tri_material, "tri_material", _I32, n_idx // 3), self._dev(kd4, "kd4"))
        if material_map is None:
            st = self.lib.vct_voxelize_device(*args, nm)
        else:
            # the C-ABI bounds both kd4 and the map by one n_mat: a longer map would let K1
            # read kd4 past its end on the device (the host path checks the same)
            if kd4 is not None and material_map.numel() != nm:
                raise VctError(_EINVAL, f"voxelize_device: material_map has {material_map.numel()} entries for "
                                        f"{nm} materials")
            mm = self._dev(material_map, "material_map", ("torch.int32",), max(nm, 1))
            st = self.lib.vct_voxelize_textured_device(*args, mm, material_map.numel(), uv_offset)
        self._check(st, "voxelize_device")

    def inject_directional(self, dir_to_light, color=(1.0, 1.0, 1.0)):
        l = (C.c_float * 3)(*[float(x) for x in dir_to_light])
        c = (C.c_float * 3)(*[float(x) for x in color])
        self._check(self.lib.vct_inject_directional(self.h, l, c), "inject")

    def inject_lights(self, lights):
        """vct_inject_lights: K2 for a list of VctLight (vct.directional_light / point_light /
        spot_light), summed in list order; replaces level 0 as inject_directional does."""
        fn = _lib.bind_light_extension(self.lib, "vct_inject_lights")
        arr, n = _light_array(lights)
        self._check(fn(self.h, arr, n), "inject_lights")

    def build_mips(self):
        self._check(self.lib.vct_build_mips(self.h), "build_mips")

    def inject_bounces(self, n_bounces: int = 1):
        """vct_inject_bounces: n more light bounces into level 0 (after inject + build_mips;
        the mips are rebuilt).  Once per level 0: VctError(ESTATE) on a second call."""
        fn = _lib.bind_extension(self.lib, "vct_inject_bounces")
        self._check(fn(self.h, int(n_bounces)), "inject_bounces")

    def bounce_sources(self) -> int:
        """vct_bounce_sources: occupied voxels with a nonzero normal (the bounce's cone origins)."""
        fn = _lib.bind_extension(self.lib, "vct_bounce_sources")
        n = C.c_uint32()
        self._check(fn(self.h, C.byref(n)), "bounce_sources")
        return int(n.value)

    # -- K4 ---------------------------------------------------------------
    def trace(self, pos4: np.ndarray, nrm4: np.ndarray, alb4: np.ndarray, eye, want_steps=True):
        h, w = pos4.shape[:2]
        pos4 = np.ascontiguousarray(pos4, dtype=np.float32)
        nrm4 = np.ascontiguousarray(nrm4, dtype=np.float32)
        alb4 = np.ascontiguousarray(alb4, dtype=np.float32)
        diff = np.empty((h, w, 4), np.float32)
        spec = np.empty((h, w, 4), np.float32)
        steps = np.empty((h, w), np.uint32) if want_steps else None
        total = C.c_uint64()
        st = self.lib.vct_trace(self.h, _fptr(pos4), _fptr(nrm4), _fptr(alb4), w, h, _f3(eye),
                                _fptr(diff), _fptr(spec), _fptr(steps) if steps is not None else None,
                                C.byref(total))
        self._check(st, "trace")
        return {"diffuse": diff, "spec": spec, "steps_px": steps, "cone_steps": int(total.value)}

    def trace_device(self, pos4, nrm4, alb4, width, height, eye, diffuse4, spec4, steps_px=None,
                     cone_steps=None, texel_fetches=None, tile_rank=0, tile_world=1, tile_compact=False,
                     variant=0):
        """Device-resident trace; arguments are torch CUDA tensors (or raw int pointers)."""
        a = VctTraceArgs()
        px = width * height
        out_px = tiles_for_rank(width, height, tile_rank, tile_world) * 64 * 64 if tile_compact else px
        a.pos4 = self._dev(pos4, "pos4", _F32, 4 * px)
        a.nrm4 = self._dev(nrm4, "nrm4", _F32, 4 * px)
        a.alb4 = self._dev(alb4, "alb4", _F32, 4 * px)
        a.width, a.height = width, height
        a.eye = _f3(eye)
        a.diffuse4 = self._dev(diffuse4, "diffuse4", _F32, 4 * out_px)
        a.spec4 = self._dev(spec4, "spec4", _F32, 4 * out_px)
        a.steps_px = self._dev(steps_px, "steps_px", _I32, px)
        a.cone_steps = self._dev(cone_steps, "cone_steps", _I64, 1)
        a.texel_fetches = self._dev(texel_fetches, "texel_fetches", _I64, 1)
        a.tile_rank, a.tile_world = tile_rank, tile_world
        a.tile_compact = 1 if tile_compact else 0
        a.variant = variant
        self._check(self.lib.vct_trace_device(self.h, C.byref(a)), "trace_device")

    def untile_device(self, gathered4, width, height, world, frame4):
        g = self._dev(gathered4, "gathered4", _F32, max(world, 1) * tiles_for_rank(width, height, 0, world) * 4096 * 4)
        self._check(self.lib.vct_untile_device(self.h, g, width, height, world,
                                               self._dev(frame4, "frame4", _F32, width * height * 4)),
                    "untile_device")

    def untile_planes_device(self, gathered4, width, height, world, frames4, packed=False):
        """gathered4: [world][planes][max_tiles*64*64][4] (one all-gather of equal-size
        rank buffers) or, packed, rank r's [planes][tiles(r)*64*64][4] at tile offset
        planes * tile_offset(r) (the gather to one rank); frames4: [h][w][4] outputs."""
        planes = len(frames4)
        need = (planes * tiles_for_rank(width, height, 0, 1) if packed
                else max(world, 1) * planes * tiles_for_rank(width, height, 0, world)) * 4096 * 4
        g = self._dev(gathered4, "gathered4", _F32, need)
        arr = (C.c_void_p * planes)(*[self._dev(f, "frames4", _F32, width * height * 4) for f in frames4])
        fn = self.lib.vct_untile_planes_packed_device if packed else self.lib.vct_untile_planes_device
        self._check(fn(self.h, g, planes, width, height, world, C.cast(arr, C.c_void_p)), "untile_planes_device")

    # -- one process per GPU over RCCL (vct_comm_*) -----------
    @staticmethod
    def comm_get_id(lib=None) -> bytes:
        lib = lib if lib is not None else _lib.load()
        cid = VctCommId()
        st = lib.vct_comm_get_id(C.byref(cid))
        if st != 0:
            raise VctError(st, "vct_comm_get_id")
        return C.string_at(C.addressof(cid), 128)

    def comm_init(self, comm_id: bytes, nranks: int, rank: int):
        cid = VctCommId()
        C.memmove(C.addressof(cid), comm_id, 128)
        self._check(self.lib.vct_comm_init(self.h, C.byref(cid), nranks, rank), "comm_init")

    def comm_broadcast_level0(self, root: int = 0):
        self._check(self.lib.vct_comm_broadcast_level0(self.h, root), "comm_broadcast_level0")

    def comm_trace_frame(self, pos4, nrm4, alb4, width, height, eye, diffuse4, spec4, root=0,
                         cone_steps=None, variant=0):
        """Trace this rank's tiles and assemble the frame on `root` (VCT_ALL_RANKS: every rank)."""
        a = VctTraceArgs()
        px = width * height
        a.pos4 = self._dev(pos4, "pos4", _F32, 4 * px)
        a.nrm4 = self._dev(nrm4, "nrm4", _F32, 4 * px)
        a.alb4 = self._dev(alb4, "alb4", _F32, 4 * px)
        a.width, a.height = width, height
        a.eye = _f3(eye)
        a.diffuse4 = self._dev(diffuse4, "diffuse4", _F32, 4 * px)
        a.spec4 = self._dev(spec4, "spec4", _F32, 4 * px)
        a.cone_steps = self._dev(cone_steps, "cone_steps", _I64, 1)
        a.variant = variant
        self._check(self.lib.vct_comm_trace_frame(self.h, C.byref(a), root), "comm_trace_frame")

    def comm_destroy(self):
        self._check(self.lib.vct_comm_destroy(self.h), "comm_destroy")

    def comm_rank(self) -> tuple[int, int]:
        """(rank, nranks) of the context's communicator as RCCL holds it (vct_comm_rank;
        (0, 1) without one)."""
        r, n = C.c_uint32(), C.c_uint32()
        self._check(self.lib.vct_comm_rank(self.h, C.byref(r), C.byref(n)), "comm_rank")
        return r.value, n.value

    def comm_set_timeout(self, timeout_ms: int):
        self._check(self.lib.vct_comm_set_timeout(self.h, int(timeout_ms)), "comm_set_timeout")

    def comm_synchronize(self):
        """Wait for the queued work incl. collectives; VctError(ECOMM) after the deadline."""
        self._check(self.lib.vct_comm_synchronize(self.h), "comm_synchronize")


    def _gbuf_ptrs(self, width, height, pos4, nrm4, alb4):
        n = 4 * width * height
        return self._dev(pos4, "pos4", _F32, n), self._dev(nrm4, "nrm4", _F32, n), self._dev(alb4, "alb4", _F32, n)

    def gbuffer_raycast_device(self, cam, width, height, roughness, pos4, nrm4, alb4):
        c = cam.to_ctypes() if hasattr(cam, "to_ctypes") else cam
        self._check(self.lib.vct_gbuffer_raycast_device(self.h, C.byref(c), width, height, float(roughness),
                                                        *self._gbuf_ptrs(width, height, pos4, nrm4, alb4)),
                    "raycast")

    def gbuffer_raster_device(self, cam, width, height, roughness, pos4, nrm4, alb4):
        """Row f2: tile-binned G-buffer pass (same output as gbuffer_raycast_device)."""
        c = cam.to_ctypes() if hasattr(cam, "to_ctypes") else cam
        self._check(self.lib.vct_gbuffer_raster_device(self.h, C.byref(c), width, height, float(roughness),
                                                       *self._gbuf_ptrs(width, height, pos4, nrm4, alb4)),
                    "raster")

    def composite_device(self, pos4, nrm4, alb4, diffuse4, spec4, width, height, dir_to_light,
                         color=(1.0, 1.0, 1.0), out_linear4=None, out_rgba8=None):
        """Row f3 composite + present on device buffers (torch tensors or raw pointers)."""
        l = (C.c_float * 3)(*[float(x) for x in dir_to_light])
        c = (C.c_float * 3)(*[float(x) for x in color])
        n = 4 * width * height
        self._check(self.lib.vct_composite_device(
            self.h, *self._gbuf_ptrs(width, height, pos4, nrm4, alb4), self._dev(diffuse4, "diffuse4", _F32, n),
            self._dev(spec4, "spec4", _F32, n), width, height, l, c, self._dev(out_linear4, "out_linear4", _F32, n),
            self._dev(out_rgba8, "out_rgba8", _I32, width * height)), "composite")

    def composite_lights_device(self, pos4, nrm4, alb4, diffuse4, spec4, width, height, lights,
                                out_linear4=None, out_rgba8=None):
        """composite_device with the direct term summed over a list of VctLight."""
        fn = _lib.bind_light_extension(self.lib, "vct_composite_lights_device")
        arr, nl = _light_array(lights)
        n = 4 * width * height
        self._check(fn(
            self.h, *self._gbuf_ptrs(width, height, pos4, nrm4, alb4), self._dev(diffuse4, "diffuse4", _F32, n),
            self._dev(spec4, "spec4", _F32, n), width, height, arr, nl,
            self._dev(out_linear4, "out_linear4", _F32, n),
            self._dev(out_rgba8, "out_rgba8", _I32, width * height)), "composite_lights")

    def shadow_cones_device(self, pos4, nrm4, width, height, lights, tan_half, vis, cone_steps=None):
        """vct_shadow_cones_device: V in [0, 1] for every (light, pixel) into vis, a float32
        device tensor [len(lights), height, width].  tan_half: one half-angle tangent per
        light; 0 keeps the hard voxel walk for that light.  cone_steps: a 1-element int64
        device tensor that the call adds its cone steps to."""
        fn = _lib.bind_shadow_extension(self.lib, "vct_shadow_cones_device")
        arr, nl = _light_array(lights)
        tan_half = [float(t) for t in tan_half]
        if len(tan_half) != nl:
            raise VctError(_EINVAL, f"shadow_cones: {len(tan_half)} tan_half values for {nl} lights")
        th = (C.c_float * max(nl, 1))(*tan_half)
        n = 4 * width * height
        self._check(fn(self.h, self._dev(pos4, "pos4", _F32, n), self._dev(nrm4, "nrm4", _F32, n), width, height,
                       arr, nl, th, self._dev(vis, "vis", _F32, nl * width * height),
                       self._dev(cone_steps, "cone_steps", _I64, 1)), "shadow_cones")

    def composite_shadowed_device(self, pos4, nrm4, alb4, diffuse4, spec4, width, height, lights, vis,
                                  out_linear4=None, out_rgba8=None):
        """composite_lights_device with V read from vis (shadow_cones_device's output)."""
        fn = _lib.bind_shadow_extension(self.lib, "vct_composite_shadowed_device")
        arr, nl = _light_array(lights)
        n = 4 * width * height
        self._check(fn(
            self.h, *self._gbuf_ptrs(width, height, pos4, nrm4, alb4), self._dev(diffuse4, "diffuse4", _F32, n),
            self._dev(spec4, "spec4", _F32, n), width, height, arr, nl,
            self._dev(vis, "vis", _F32, nl * width * height),
            self._dev(out_linear4, "out_linear4", _F32, n),
            self._dev(out_rgba8, "out_rgba8", _I32, width * height)), "composite_shadowed")

    # -- emissive surfaces (include/vct_emission.h) -------------------------
    def voxelize_emission(self, verts: np.ndarray, idx: np.ndarray, tri_material: np.ndarray | None,
                          ke4: np.ndarray):
        """vct_voxelize_emission: the emission grid of the current voxelization from emitter
        triangles (the voxelized mesh or a subset of it) and ke4 [materials, 4], Ke per material."""
        fn = _lib.bind_emission_extension(self.lib, "vct_voxelize_emission")
        verts = np.ascontiguousarray(verts, dtype=np.float32)
        assert verts.ndim == 2 and verts.shape[1] >= 3
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        mat = None if tri_material is None else np.ascontiguousarray(tri_material, dtype=np.uint32).reshape(-1)
        ke = None if ke4 is None else np.ascontiguousarray(ke4, dtype=np.float32)
        if idx.size % 3:
            raise VctError(_EINVAL, f"voxelize_emission: {idx.size} indices, not a multiple of 3")
        if mat is not None and mat.size != idx.size // 3:
            raise VctError(_EINVAL, f"voxelize_emission: tri_material has {mat.size} entries for "
                                    f"{idx.size // 3} triangles")
        if ke is not None and (ke.ndim != 2 or ke.shape[1] != 4):
            raise VctError(_EINVAL, f"voxelize_emission: ke4 must be [materials, 4], got {ke.shape}")
        self._check(fn(self.h, _fptr(verts), verts.shape[1] * 4, verts.shape[0], _fptr(idx), idx.size,
                       _fptr(mat) if mat is not None else None, _fptr(ke) if ke is not None else None,
                       0 if ke is None else ke.shape[0]), "voxelize_emission")

    def voxelize_emission_device(self, verts, idx, tri_material, ke4):
        """vct_voxelize_emission_device on torch tensors: verts [V, F >= 3] float32, idx [3T]
        int32 / uint32, tri_material [T] int32 or None, ke4 [M, 4] float32."""
        fn = _lib.bind_emission_extension(self.lib, "vct_voxelize_emission_device")
        if verts.dim() != 2 or verts.shape[1] < 3:
            raise VctError(_EINVAL, f"voxelize_emission_device: verts must be [V, F >= 3], got {tuple(verts.shape)}")
        if str(idx.dtype) in _I64:
            raise VctError(_EINVAL, "voxelize_emission_device: idx must be int32 / uint32, not 64-bit")
        n_idx = idx.numel()
        if n_idx % 3:
            raise VctError(_EINVAL, f"voxelize_emission_device: {n_idx} indices, not a multiple of 3")
        if ke4 is not None and not isinstance(ke4, int) and (ke4.dim() != 2 or ke4.shape[1] != 4):
            raise VctError(_EINVAL, f"voxelize_emission_device: ke4 must be [materials, 4], got {tuple(ke4.shape)}")
        nm = 0 if ke4 is None or isinstance(ke4, int) else ke4.shape[0]
        self._check(fn(self.h, self._dev(verts, "verts"), verts.shape[1] * 4, verts.shape[0],
                       self._dev(idx, "idx", _I32), n_idx, self._dev(tri_material, "tri_material", _I32, n_idx // 3),
                       self._dev(ke4, "ke4"), nm), "voxelize_emission_device")

    def emission_voxels(self) -> int:
        """vct_emission_voxels: emissive voxels of the emission grid (0 for an empty one)."""
        fn = _lib.bind_emission_extension(self.lib, "vct_emission_voxels")
        n = C.c_uint32()
        self._check(fn(self.h, C.byref(n)), "emission_voxels")
        return int(n.value)

    def download_emission(self) -> np.ndarray:
        """vct_download_emission: [n, n, n, 4] float32 (z, y, x): (E.rgb, 1) at the emissive
        voxels, +0 elsewhere."""
        fn = _lib.bind_emission_extension(self.lib, "vct_download_emission")
        out = np.empty((self.n, self.n, self.n, 4), np.float32)
        self._check(fn(self.h, _fptr(out)), "download_emission")
        return out

    def inject_emission(self, scale: float = 1.0):
        """vct_inject_emission: level 0 += scale * E (after an inject or upload, before
        build_mips and inject_bounces).  Once per level 0: VctError(ESTATE) on a second call."""
        fn = _lib.bind_emission_extension(self.lib, "vct_inject_emission")
        self._check(fn(self.h, float(scale)), "inject_emission")

    def composite_emissive_device(self, pos4, nrm4, alb4, diffuse4, spec4, width, height, lights, vis=None,
                                  scale: float = 1.0, out_linear4=None, out_rgba8=None):
        """composite_shadowed_device plus scale * E of the pixel's voxel; vis=None: every light
        takes the hard voxel walk (composite_lights_device's direct term)."""
        fn = _lib.bind_emission_extension(self.lib, "vct_composite_emissive_device")
        arr, nl = _light_array(lights)
        n = 4 * width * height
        self._check(fn(
            self.h, *self._gbuf_ptrs(width, height, pos4, nrm4, alb4), self._dev(diffuse4, "diffuse4", _F32, n),
            self._dev(spec4, "spec4", _F32, n), width, height, arr, nl,
            self._dev(vis, "vis", _F32, nl * width * height), float(scale),
            self._dev(out_linear4, "out_linear4", _F32, n),
            self._dev(out_rgba8, "out_rgba8", _I32, width * height)), "composite_emissive")

    # -- sky light (include/vct_sky.h) --------------------------------------
    def sky_cones_device(self, pos4, nrm4, width, height, sky, sky4, diffuse4_inout=None, cone_steps=None):
        """vct_sky_cones_device: (Sk.rgb, vis) per pixel into sky4, a float32 device tensor
        [height, width, 4]; diffuse4_inout (K4's diffuse plane of the frame): rgb += Sk.rgb at
        every valid pixel.  sky: a VctSky (vct.sky_light).  cone_steps: a 1-element int64
        device tensor that the call adds its cone steps to."""
        fn = _lib.bind_sky_extension(self.lib, "vct_sky_cones_device")
        if not isinstance(sky, VctSky):
            raise VctError(_EINVAL, f"sky_cones: expected a VctSky (vct.sky_light), got {type(sky).__name__}")
        n = 4 * width * height
        self._check(fn(self.h, self._dev(pos4, "pos4", _F32, n), self._dev(nrm4, "nrm4", _F32, n), width, height,
                       C.byref(sky), self._dev(sky4, "sky4", _F32, n),
                       self._dev(diffuse4_inout, "diffuse4_inout", _F32, n),
                       self._dev(cone_steps, "cone_steps", _I64, 1)), "sky_cones")

    def inject_sky(self, sky):
        """vct_inject_sky: level 0 += A * Sk at every bounce source, then the mips (after
        build_mips, before inject_bounces).  Once per level 0: VctError(ESTATE) on a second call."""
        fn = _lib.bind_sky_extension(self.lib, "vct_inject_sky")
        if not isinstance(sky, VctSky):
            raise VctError(_EINVAL, f"inject_sky: expected a VctSky (vct.sky_light), got {type(sky).__name__}")
        self._check(fn(self.h, C.byref(sky)), "inject_sky")

    # -- the sky in view (include/vct_sky_view.h) ----------------------------
    def sky_specular_device(self, pos4, nrm4, alb4, width, height, eye, sky, skyspec4, spec4_inout=None,
                            cone_steps=None):
        """vct_sky_specular_device: (S.rgb, T) per pixel into skyspec4, a float32 device tensor
        [height, width, 4]: the sky seen by the pixel's specular cone; spec4_inout (K4's specular
        plane of the frame): rgb += S.rgb at every valid pixel.  sky: a VctSky (vct.sky_light).
        cone_steps: a 1-element int64 device tensor that the call adds its cone steps to."""
        fn = _lib.bind_sky_view_extension(self.lib, "vct_sky_specular_device")
        if not isinstance(sky, VctSky):
            raise VctError(_EINVAL, f"sky_specular: expected a VctSky (vct.sky_light), got {type(sky).__name__}")
        n = 4 * width * height
        self._check(fn(self.h, *self._gbuf_ptrs(width, height, pos4, nrm4, alb4), width, height, _f3(eye),
                       C.byref(sky), self._dev(skyspec4, "skyspec4", _F32, n),
                       self._dev(spec4_inout, "spec4_inout", _F32, n),
                       self._dev(cone_steps, "cone_steps", _I64, 1)), "sky_specular")

    def sky_background_device(self, cam, pos4, width, height, sky, linear4_inout=None, rgba8_inout=None):
        """vct_sky_background_device: at every background pixel of a composited frame, the sky
        colour of the pixel's primary ray through `cam` into the linear frame (alpha 1) and / or
        its tone-mapped bytes into the RGBA8 frame; valid pixels are untouched."""
        fn = _lib.bind_sky_view_extension(self.lib, "vct_sky_background_device")
        if hasattr(cam, "to_ctypes"):
            cam = cam.to_ctypes()
        if not isinstance(cam, VctCamera):
            raise VctError(_EINVAL, f"sky_background: expected a camera, got {type(cam).__name__}")
        if not isinstance(sky, VctSky):
            raise VctError(_EINVAL, f"sky_background: expected a VctSky (vct.sky_light), got {type(sky).__name__}")
        n = 4 * width * height
        self._check(fn(self.h, C.byref(cam), self._dev(pos4, "pos4", _F32, n), width, height, C.byref(sky),
                       self._dev(linear4_inout, "linear4_inout", _F32, n),
                       self._dev(rgba8_inout, "rgba8_inout", _I32, width * height)), "sky_background")

    # -- the environment-map sky (include/vct_env.h) --------------------------
    @staticmethod
    def _env(env, what):
        env = getattr(env, "record", env)            # a vct.env.EnvMap keeps its record
        if not isinstance(env, VctEnvSky):
            raise VctError(_EINVAL, f"{what}: expected a VctEnvSky (vct.env_sky) or a vct.env.EnvMap, got {type(env).__name__}")
        return env

    def set_env(self, oct4):
        """vct_set_env: the context's octahedral map, [S, S, 4] float32 on the host (row 0 =
        p.y = -1), S a power of two; None or an empty array clears it.  Synchronous."""
        fn = _lib.bind_env_extension(self.lib, "vct_set_env")
        if oct4 is None or np.asarray(oct4).size == 0:
            self._check(fn(self.h, None, 0), "set_env")
            return
        m = np.ascontiguousarray(oct4, dtype=np.float32)
        if m.ndim != 3 or m.shape[0] != m.shape[1] or m.shape[2] != 4:
            raise VctError(_EINVAL, f"set_env: the map must be [S, S, 4] float32, got {m.shape}")
        self._check(fn(self.h, _fptr(m), m.shape[0]), "set_env")

    @property
    def env_size(self) -> int:
        return int(_lib.bind_env_extension(self.lib, "vct_env_size")(self.h))

    def env_download_level(self, level: int) -> np.ndarray:
        """vct_env_download_level: level `level` of the map's pyramid, [S_j, S_j, 4] float32."""
        fn = _lib.bind_env_extension(self.lib, "vct_env_download_level")
        sj = max(self.env_size >> level, 1)
        out = np.empty((sj, sj, 4), np.float32)
        self._check(fn(self.h, level, _fptr(out)), "env_download_level")
        return out

    def env_lookup_device(self, env, dir_tau4, count, out4):
        """vct_env_lookup_device: (d.xyz, tau) per lane in dir_tau4 -> (Env.rgb, level m) in out4,
        float32 device tensors of [count, 4]."""
        fn = _lib.bind_env_extension(self.lib, "vct_env_lookup_device")
        self._check(fn(self.h, C.byref(self._env(env, "env_lookup")), self._dev(dir_tau4, "dir_tau4", _F32, 4 * count),
                       count, self._dev(out4, "out4", _F32, 4 * count)), "env_lookup")

    def env_cones_device(self, pos4, nrm4, width, height, env, sky4, diffuse4_inout=None, cone_steps=None):
        """vct_env_cones_device: sky_cones_device with the context's map for the sky colour."""
        fn = _lib.bind_env_extension(self.lib, "vct_env_cones_device")
        n = 4 * width * height
        self._check(fn(self.h, self._dev(pos4, "pos4", _F32, n), self._dev(nrm4, "nrm4", _F32, n), width, height,
                       C.byref(self._env(env, "env_cones")), self._dev(sky4, "sky4", _F32, n),
                       self._dev(diffuse4_inout, "diffuse4_inout", _F32, n),
                       self._dev(cone_steps, "cone_steps", _I64, 1)), "env_cones")

    def inject_env(self, env):
        """vct_inject_env: inject_sky with the map (one of the two, once per level 0)."""
        fn = _lib.bind_env_extension(self.lib, "vct_inject_env")
        self._check(fn(self.h, C.byref(self._env(env, "inject_env"))), "inject_env")

    def env_specular_device(self, pos4, nrm4, alb4, width, height, eye, env, skyspec4, spec4_inout=None,
                            cone_steps=None):
        """vct_env_specular_device: sky_specular_device with the map, blurred by the pixel's aperture."""
        fn = _lib.bind_env_extension(self.lib, "vct_env_specular_device")
        n = 4 * width * height
        self._check(fn(self.h, *self._gbuf_ptrs(width, height, pos4, nrm4, alb4), width, height, _f3(eye),
                       C.byref(self._env(env, "env_specular")), self._dev(skyspec4, "skyspec4", _F32, n),
                       self._dev(spec4_inout, "spec4_inout", _F32, n),
                       self._dev(cone_steps, "cone_steps", _I64, 1)), "env_specular")

    def env_background_device(self, cam, pos4, width, height, env, linear4_inout=None, rgba8_inout=None):
        """vct_env_background_device: sky_background_device with Env(d, 0)."""
        fn = _lib.bind_env_extension(self.lib, "vct_env_background_device")
        if hasattr(cam, "to_ctypes"):
            cam = cam.to_ctypes()
        if not isinstance(cam, VctCamera):
            raise VctError(_EINVAL, f"env_background: expected a camera, got {type(cam).__name__}")
        n = 4 * width * height
        self._check(fn(self.h, C.byref(cam), self._dev(pos4, "pos4", _F32, n), width, height,
                       C.byref(self._env(env, "env_background")),
                       self._dev(linear4_inout, "linear4_inout", _F32, n),
                       self._dev(rgba8_inout, "rgba8_inout", _I32, width * height)), "env_background")

    # -- cone queries and the probe grid (include/vct_query.h) ---------------
    def cone_query_device(self, cones, count, out4, steps=None, cone_steps=None):
        """vct_cone_query_device: marches `count` vct_cone records -- `cones`, a float32 device
        tensor [count, 12] (p, tau, d, t_lim, off, valid) -- and writes (c.rgb, a) per cone into
        out4, a float32 device tensor [count, 4].  steps: an int32 device tensor [count] that
        receives the steps per cone; cone_steps: a 1-element int64 device tensor that the call
        adds its steps to.  Order the cones spatially: the call does not sort."""
        fn = _lib.bind_query_extension(self.lib, "vct_cone_query_device")
        a = _lib.VctConeQueryArgs()
        a.cones = self._dev(cones, "cones", _F32, 12 * count)
        a.count = int(count)
        a.out4 = self._dev(out4, "out4", _F32, 4 * count)
        a.steps = self._dev(steps, "steps", _I32, count)
        a.cone_steps = self._dev(cone_steps, "cone_steps", _I64, 1)
        self._check(fn(self.h, C.byref(a)), "cone_query")

    @staticmethod
    def _probe_grid(grid, what):
        if not isinstance(grid, _lib.VctProbeGrid):
            raise VctError(_EINVAL, f"{what}: expected a VctProbeGrid (vct.probe_grid), got {type(grid).__name__}")
        return int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])

    def probe_build_device(self, grid, probes, state, cone_steps=None):
        """vct_probe_build_device: the six axis cones of every probe of `grid` (a VctProbeGrid)
        into probes, a float32 device tensor [dz, dy, dx, 6, 4], and the probes' validity into
        state, an int32 device tensor [dz, dy, dx]."""
        fn = _lib.bind_query_extension(self.lib, "vct_probe_build_device")
        n = self._probe_grid(grid, "probe_build")
        self._check(fn(self.h, C.byref(grid), self._dev(probes, "probes", _F32, 24 * n),
                       self._dev(state, "state", _I32, n), self._dev(cone_steps, "cone_steps", _I64, 1)), "probe_build")

    def probe_sample_device(self, grid, probes, state, pos4, nrm4, count, out4, misses=None):
        """vct_probe_sample_device: the probes around each of `count` points (pos4, nrm4: float32
        device tensors [count, 4]) blended into out4 [count, 4], a plane with the meaning of
        K4's diffuse4.  misses: a 1-element int32 device tensor, += the points without a valid
        probe around them."""
        fn = _lib.bind_query_extension(self.lib, "vct_probe_sample_device")
        n = self._probe_grid(grid, "probe_sample")
        self._check(fn(self.h, C.byref(grid), self._dev(probes, "probes", _F32, 24 * n),
                       self._dev(state, "state", _I32, n), self._dev(pos4, "pos4", _F32, 4 * count),
                       self._dev(nrm4, "nrm4", _F32, 4 * count), int(count), self._dev(out4, "out4", _F32, 4 * count),
                       self._dev(misses, "misses", _I32, 1)), "probe_sample")

    # -- the voxel view and ray picking (include/vct_voxview.h) ---------------
    def voxel_pick_device(self, org4, dir4, count, hit4, level=0, solid=_lib.VCT_VOXPICK_OCCUPANCY, cells=None):
        """vct_voxel_pick_device: walks `count` rays -- org4 (world origin) and dir4 (direction,
        .w = t_lim in level-0 voxel units), float32 device tensors [count, 4] -- through `level`
        and writes (cell, face, steps, float bits of t) per ray into hit4, an int32 device tensor
        [count, 4].  solid: VCT_VOXPICK_OCCUPANCY (level 0) or VCT_VOXPICK_ALPHA.  cells: a
        1-element int64 device tensor that the call adds the cells it tested to."""
        fn = _lib.bind_voxview_extension(self.lib, "vct_voxel_pick_device")
        a = VctVoxelPickArgs()
        a.org4 = self._dev(org4, "org4", _F32, 4 * count)
        a.dir4 = self._dev(dir4, "dir4", _F32, 4 * count)
        a.count, a.level, a.solid = int(count), int(level), int(solid)
        a.hit4 = self._dev(hit4, "hit4", _I32, 4 * count)
        a.cells = self._dev(cells, "cells", _I64, 1)
        self._check(fn(self.h, C.byref(a)), "voxel_pick")

    def voxel_view_device(self, cam, width, height, level=0, mode=_lib.VCT_VOXVIEW_RADIANCE, shade=False,
                          linear4=None, rgba8=None, hit4=None, cells=None):
        """vct_voxel_view_device: the voxel view of `cam` at `level` in `mode` (VCT_VOXVIEW_*) into
        any of linear4 (float32 [h, w, 4]), rgba8 (int32 [h, w]) and hit4 (int32 [h, w, 4], the
        records of voxel_pick_device); cells as there."""
        fn = _lib.bind_voxview_extension(self.lib, "vct_voxel_view_device")
        if hasattr(cam, "to_ctypes"):
            cam = cam.to_ctypes()
        if not isinstance(cam, VctCamera):
            raise VctError(_EINVAL, f"voxel_view: expected a camera, got {type(cam).__name__}")
        a = VctVoxelViewArgs()
        a.width, a.height, a.level, a.mode, a.shade = int(width), int(height), int(level), int(mode), int(bool(shade))
        n = width * height
        a.linear4 = self._dev(linear4, "linear4", _F32, 4 * n)
        a.rgba8 = self._dev(rgba8, "rgba8", _I32, n)
        a.hit4 = self._dev(hit4, "hit4", _I32, 4 * n)
        a.cells = self._dev(cells, "cells", _I64, 1)
        self._check(fn(self.h, C.byref(cam), C.byref(a)), "voxel_view")

    # -- the shading G-buffer (include/vct_shading.h) ------------------------
    def set_shading(self, verts, idx=None, tri_material=None, materials=(), normal_offset=12, uv_offset=UV_OFFSET,
                    tangent_offset=32, bitangent_offset=44):
        """vct_set_shading: the attribute records and the material table of the current static
        voxelization, from the host arrays that were voxelized (verts [V, F] float32, idx [3T]).
        An offset of None marks the attribute absent; materials: VctShadingMaterial records or
        vct.shading.ShadingMaterial.  set_shading(None) clears the set."""
        fn = _lib.bind_shading_extension(self.lib, "vct_set_shading")
        if verts is None:
            self._check(fn(self.h, None), "set_shading")
            return
        verts = np.ascontiguousarray(verts, dtype=np.float32)
        if verts.ndim != 2:
            raise VctError(_EINVAL, f"set_shading: verts must be [V, F], got {verts.shape}")
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        mat = None if tri_material is None else np.ascontiguousarray(tri_material, dtype=np.uint32).reshape(-1)
        if mat is not None and mat.size != idx.size // 3:
            raise VctError(_EINVAL, f"set_shading: tri_material has {mat.size} entries for {idx.size // 3} triangles")
        recs = [m.to_ctypes() if hasattr(m, "to_ctypes") else m for m in materials]
        if not all(isinstance(m, VctShadingMaterial) for m in recs):
            raise VctError(_EINVAL, "set_shading: materials must be VctShadingMaterial or ShadingMaterial records")
        arr = (VctShadingMaterial * max(len(recs), 1))(*recs)
        d = VctShadingDesc()
        d.verts, d.vertex_stride, d.n_verts = verts.ctypes.data, verts.shape[1] * 4, verts.shape[0]
        d.idx, d.n_idx = idx.ctypes.data, idx.size
        d.tri_material = mat.ctypes.data if mat is not None else None
        absent = lambda o: _lib.VCT_SHADING_NO_ATTR if o is None else int(o)
        d.normal_offset, d.uv_offset = absent(normal_offset), absent(uv_offset)
        d.tangent_offset, d.bitangent_offset = absent(tangent_offset), absent(bitangent_offset)
        d.materials, d.n_materials = C.cast(arr, C.c_void_p), len(recs)
        self._check(fn(self.h, C.byref(d)), "set_shading")

    def gbuffer_shaded_device(self, cam, width, height, roughness, pos4, nrm4, alb4, ks4, geo4=None, tri_id=None,
                              bary2=None):
        """vct_gbuffer_shaded_device: the tile-binned pass with the shading normal in nrm4, the
        material's roughness in alb4.w and Ks x map_Ks in ks4; optionally the geometric normal
        (geo4, float32 [h, w, 4]), the triangle id (int32 [h, w]) and the barycentrics (float32
        [h, w, 2])."""
        fn = _lib.bind_shading_extension(self.lib, "vct_gbuffer_shaded_device")
        c = cam.to_ctypes() if hasattr(cam, "to_ctypes") else cam
        n = width * height
        self._check(fn(self.h, C.byref(c), width, height, float(roughness),
                       *self._gbuf_ptrs(width, height, pos4, nrm4, alb4), self._dev(ks4, "ks4", _F32, 4 * n),
                       self._dev(geo4, "geo4", _F32, 4 * n), self._dev(tri_id, "tri_id", _I32, n),
                       self._dev(bary2, "bary2", _F32, 2 * n)), "gbuffer_shaded")

    # -- alpha-cutout materials (include/vct_cutout.h) -----------------------
    @staticmethod
    def _cutout_table(cutouts):
        """A (VctCutout array or None, entries) pair from None, VctCutout records, or
        (map, channel, cutoff) tuples (vct.cutout.cutouts_from_model gives such a list)."""
        if cutouts is None:
            return None, 0
        recs = []
        for e in cutouts:
            if not isinstance(e, VctCutout):
                m, ch, cut = e
                e = VctCutout(int(m), int(ch), float(cut), 0)
            recs.append(e)
        return (VctCutout * max(len(recs), 1))(*recs), len(recs)

    def voxelize_cutout(self, verts, idx, tri_material=None, kd4=None, material_map=None, material_cutout=None,
                        uv_offset=UV_OFFSET):
        """vct_voxelize_cutout: voxelize(material_map=...) with a per-material cutout table
        (VctCutout records or (map, channel, cutoff) tuples; None = every material opaque)."""
        fn = _lib.bind_cutout_extension(self.lib, "vct_voxelize_cutout")
        verts = np.ascontiguousarray(verts, dtype=np.float32)
        assert verts.ndim == 2 and verts.shape[1] >= 3
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        mat = None if tri_material is None else np.ascontiguousarray(tri_material, dtype=np.uint32).reshape(-1)
        kd = None if kd4 is None else np.ascontiguousarray(kd4, dtype=np.float32)
        mm = None if material_map is None else np.ascontiguousarray(material_map, dtype=np.int32).reshape(-1)
        if idx.size % 3:
            raise VctError(_EINVAL, f"voxelize_cutout: {idx.size} indices, not a multiple of 3")
        if mat is not None and mat.size != idx.size // 3:
            raise VctError(_EINVAL, f"voxelize_cutout: tri_material has {mat.size} entries for {idx.size // 3} triangles")
        if kd is not None and (kd.ndim != 2 or kd.shape[1] != 4):
            raise VctError(_EINVAL, f"voxelize_cutout: kd4 must be [materials, 4], got {kd.shape}")
        table, n_cut = self._cutout_table(material_cutout)
        sizes = {n for n in (None if kd is None else kd.shape[0], None if mm is None else mm.size,
                             None if table is None else n_cut) if n is not None}
        if len(sizes) > 1:   # the C-ABI bounds kd4, the map and the table by one n_materials
            raise VctError(_EINVAL, f"voxelize_cutout: kd4, material_map and material_cutout differ in length: {sorted(sizes)}")
        n_mat = sizes.pop() if sizes else 0
        st = fn(self.h, _fptr(verts), verts.shape[1] * 4, verts.shape[0], _fptr(idx), idx.size,
                _fptr(mat) if mat is not None else None, _fptr(kd) if kd is not None else None,
                _fptr(mm) if mm is not None else None, table, n_mat, uv_offset)
        self._check(st, "voxelize_cutout")

    def voxelize_cutout_device(self, verts, idx, tri_material=None, kd4=None, material_map=None, material_cutout=None,
                               uv_offset=UV_OFFSET):
        """vct_voxelize_cutout_device: voxelize_device's tensors; material_cutout stays a host
        table (VctCutout records or (map, channel, cutoff) tuples; None = every material opaque)."""
        fn = _lib.bind_cutout_extension(self.lib, "vct_voxelize_cutout_device")
        if verts.dim() != 2 or verts.shape[1] < 3:
            raise VctError(_EINVAL, f"voxelize_cutout_device: verts must be [V, F >= 3], got {tuple(verts.shape)}")
        if str(idx.dtype) in _I64:
            raise VctError(_EINVAL, "voxelize_cutout_device: idx must be int32 / uint32, not 64-bit")
        n_idx = idx.numel()
        if n_idx % 3:
            raise VctError(_EINVAL, f"voxelize_cutout_device: {n_idx} indices, not a multiple of 3")
        if kd4 is not None and (kd4.dim() != 2 or kd4.shape[1] != 4):
            raise VctError(_EINVAL, f"voxelize_cutout_device: kd4 must be [materials, 4], got {tuple(kd4.shape)}")
        table, n_cut = self._cutout_table(material_cutout)
        sizes = {n for n in (None if kd4 is None else kd4.shape[0], None if material_map is None else material_map.numel(),
                             None if table is None else n_cut) if n is not None}
        if len(sizes) > 1:   # a longer map or table would let K1 read kd4 past its end on the device
            raise VctError(_EINVAL, f"voxelize_cutout_device: kd4, material_map and material_cutout differ in length: "
                                    f"{sorted(sizes)}")
        n_mat = sizes.pop() if sizes else 0
        st = fn(self.h, self._dev(verts, "verts"), verts.shape[1] * 4, verts.shape[0], self._dev(idx, "idx", _I32), n_idx,
                self._dev(tri_material, "tri_material", _I32, n_idx // 3), self._dev(kd4, "kd4"),
                self._dev(material_map, "material_map", ("torch.int32",), max(n_mat, 1)), table, n_mat, uv_offset)
        self._check(st, "voxelize_cutout_device")

    def gbuffer_cutout_device(self, cam, width, height, roughness, pos4, nrm4, alb4, ks4=None, geo4=None, tri_id=None,
                              bary2=None):
        """vct_gbuffer_cutout_device: the tile-binned pass over accepted candidates.  ks4 None: the
        flat records of gbuffer_raster_device; else the shaded records of gbuffer_shaded_device
        (needs a shading set), with its optional planes."""
        fn = _lib.bind_cutout_extension(self.lib, "vct_gbuffer_cutout_device")
        c = cam.to_ctypes() if hasattr(cam, "to_ctypes") else cam
        n = width * height
        self._check(fn(self.h, C.byref(c), width, height, float(roughness),
                       *self._gbuf_ptrs(width, height, pos4, nrm4, alb4), self._dev(ks4, "ks4", _F32, 4 * n),
                       self._dev(geo4, "geo4", _F32, 4 * n), self._dev(tri_id, "tri_id", _I32, n),
                       self._dev(bary2, "bary2", _F32, 2 * n)), "gbuffer_cutout")

    def cutout_materials(self) -> int:
        """vct_cutout_materials: masked materials of the current mesh, 0 if none."""
        return int(_lib.bind_cutout_extension(self.lib, "vct_cutout_materials")(self.h))

    def specular_tint_device(self, spec4, ks4, width, height, out4=None):
        """vct_specular_tint_device: out.rgb = spec.rgb * ks.rgb, out.a = spec.a (in place when
        out4 is None); call it before any composite."""
        fn = _lib.bind_shading_extension(self.lib, "vct_specular_tint_device")
        n = 4 * width * height
        s = self._dev(spec4, "spec4", _F32, n)
        self._check(fn(self.h, s, self._dev(ks4, "ks4", _F32, n), width, height,
                       s if out4 is None else self._dev(out4, "out4", _F32, n)), "specular_tint")

    # -- volumetric fog (include/vct_fog.h) ----------------------------------
    def _fog(self, fog, what):
        if not isinstance(fog, VctFog):
            raise VctError(_EINVAL, f"{what}: expected a VctFog (vct.fog), got {type(fog).__name__}")
        bad = _lib.check_fog(fog.density, tuple(fog.albedo), fog.ambient, fog.level, fog.step, self.n, self.extent)
        if bad:
            raise VctError(_EINVAL, f"{what}: {bad}")
        return C.byref(fog)

    def build_fog(self, fog, lights=(), tan_half=None):
        """vct_build_fog: the scatter volume of `fog` (vct.fog) from the current pyramid, lit by
        `lights` through one visibility cone each (tan_half: one aperture per light, default
        VCT_FOG_DEFAULT_TAN).  After build_mips (and any inject_sky / inject_bounces)."""
        fn = _lib.bind_fog_extension(self.lib, "vct_build_fog")
        ref = self._fog(fog, "build_fog")
        arr, n = _light_array(lights)
        th = [_lib.VCT_FOG_DEFAULT_TAN] * n if tan_half is None else [float(t) for t in tan_half]
        if len(th) != n:
            raise VctError(_EINVAL, f"build_fog: {len(th)} apertures for {n} lights")
        self._check(fn(self.h, ref, arr, n, (C.c_float * max(n, 1))(*th)), "build_fog")

    def fog_dims(self) -> int:
        """vct_fog_dims: the cell count m of the current scatter volume."""
        m = C.c_uint32()
        self._check(_lib.bind_fog_extension(self.lib, "vct_fog_dims")(self.h, C.byref(m)), "fog_dims")
        return int(m.value)

    def download_fog(self) -> np.ndarray:
        """vct_download_fog: the scatter volume as [m, m, m, 4] float32 (z, y, x)."""
        m = self.fog_dims()
        out = np.empty((m, m, m, 4), np.float32)
        self._check(_lib.bind_fog_extension(self.lib, "vct_download_fog")(self.h, _fptr(out)), "download_fog")
        return out

    def fog_rays_device(self, cam, eye, pos4, width, height, ray4):
        """vct_fog_rays_device: (d.xyz, len) per pixel in voxel units into ray4, a float32 device
        tensor [height, width, 4].  cam: a VctCamera (background pixels get their primary ray) or
        None (background pixels get a null record)."""
        fn = _lib.bind_fog_extension(self.lib, "vct_fog_rays_device")
        if hasattr(cam, "to_ctypes"):
            cam = cam.to_ctypes()
        if cam is not None and not isinstance(cam, VctCamera):
            raise VctError(_EINVAL, f"fog_rays: expected a camera or None, got {type(cam).__name__}")
        n = 4 * width * height
        self._check(fn(self.h, None if cam is None else C.byref(cam), _f3(eye), self._dev(pos4, "pos4", _F32, n),
                       width, height, self._dev(ray4, "ray4", _F32, n)), "fog_rays")

    def fog_march_device(self, fog, eye, ray4, width, height, fog4, steps=None):
        """vct_fog_march_device: (F.rgb, T) per pixel into fog4, a float32 device tensor
        [height, width, 4].  steps: a 1-element int64 device tensor the call adds its samples to."""
        fn = _lib.bind_fog_extension(self.lib, "vct_fog_march_device")
        n = 4 * width * height
        self._check(fn(self.h, self._fog(fog, "fog_march"), _f3(eye), self._dev(ray4, "ray4", _F32, n), width, height,
                       self._dev(fog4, "fog4", _F32, n), self._dev(steps, "steps", _I64, 1)), "fog_march")

    def fog_apply_device(self, fog4, width, height, linear4_inout=None, out_rgba8=None):
        """vct_fog_apply_device: rgb = fmaf(rgb, T, F) on a composite's linear frame, and / or the
        RGBA8 frame of the result."""
        fn = _lib.bind_fog_extension(self.lib, "vct_fog_apply_device")
        n = 4 * width * height
        self._check(fn(self.h, self._dev(fog4, "fog4", _F32, n), width, height,
                       self._dev(linear4_inout, "linear4_inout", _F32, n),
                       self._dev(out_rgba8, "out_rgba8", _I32, width * height)), "fog_apply")

    # -- mixed-resolution trace (include/vct_mixed.h) ------------------------
    def mixed_params(self, factor, normal_cos=None, plane_eps=None, max_holes=0) -> VctMixedParams:
        """A vct_mixed_params: the header defaults of this context for `factor`
        (vct_mixed_default_params), with the fields given replaced."""
        p = VctMixedParams()
        fn = _lib.bind_mixed_extension(self.lib, "vct_mixed_default_params")
        if fn(self.h, factor, C.byref(p)) != 0:      # a factor the header refuses: the calls report it
            p.normal_cos, p.plane_eps = _lib.VCT_MIXED_NORMAL_COS, 0.0
            p.factor = factor
        if normal_cos is not None:
            p.normal_cos = normal_cos
        if plane_eps is not None:
            p.plane_eps = plane_eps
        p.max_holes = max_holes
        return p

    @staticmethod
    def mixed_max_holes(width, height, max_holes=0) -> int:
        """The hole capacity a frame gets: max_holes, or ceil(width * height / 8) for 0."""
        return max_holes if max_holes else (width * height + 7) // 8

    def _mixed_args(self, pos4, nrm4, alb4, width, height, eye, diffuse4, spec4, steps_px, cone_steps,
                    texel_fetches, tile_rank, tile_world, tile_compact, variant):
        a = VctTraceArgs()
        px = width * height
        out_px = tiles_for_rank(width, height, tile_rank, tile_world) * 64 * 64 if tile_compact else px
        a.pos4 = self._dev(pos4, "pos4", _F32, 4 * px)
        a.nrm4 = self._dev(nrm4, "nrm4", _F32, 4 * px)
        a.alb4 = self._dev(alb4, "alb4", _F32, 4 * px)
        a.width, a.height = width, height
        a.eye = _f3(eye)
        a.diffuse4 = self._dev(diffuse4, "diffuse4", _F32, 4 * out_px)
        a.spec4 = self._dev(spec4, "spec4", _F32, 4 * out_px)
        a.steps_px = self._dev(steps_px, "steps_px", _I32, px)
        a.cone_steps = self._dev(cone_steps, "cone_steps", _I64, 1)
        a.texel_fetches = self._dev(texel_fetches, "texel_fetches", _I64, 1)
        a.tile_rank, a.tile_world = tile_rank, tile_world
        a.tile_compact = 1 if tile_compact else 0
        a.variant = variant
        return a

    def trace_cones_device(self, cones, pos4, nrm4, alb4, width, height, eye, diffuse4=None, spec4=None,
                           steps_px=None, cone_steps=None, texel_fetches=None, tile_rank=0, tile_world=1,
                           tile_compact=False, variant=0):
        """vct_trace_cones_device: trace_device restricted to `cones` (VCT_CONES_DIFFUSE,
        VCT_CONES_SPECULAR or both); the plane of an unselected set may be None and is not
        written."""
        fn = _lib.bind_mixed_extension(self.lib, "vct_trace_cones_device")
        a = self._mixed_args(pos4, nrm4, alb4, width, height, eye, diffuse4, spec4, steps_px, cone_steps,
                             texel_fetches, tile_rank, tile_world, tile_compact, variant)
        self._check(fn(self.h, C.byref(a), cones), "trace_cones_device")

    def mixed_pick_device(self, pos4, nrm4, alb4, width, height, eye, factor, lo_pos4, lo_nrm4, lo_alb4, lo_src):
        """vct_mixed_pick_device: the low G-buffer (ceil(width / factor) by ceil(height / factor))
        and lo_src (int32 / uint32), the full-resolution index of each low pixel's record."""
        fn = _lib.bind_mixed_extension(self.lib, "vct_mixed_pick_device")
        n = 4 * width * height
        f = factor if factor > 0 else 1
        nl = ((width + f - 1) // f) * ((height + f - 1) // f)
        self._check(fn(self.h, self._dev(pos4, "pos4", _F32, n), self._dev(nrm4, "nrm4", _F32, n),
                       self._dev(alb4, "alb4", _F32, n), width, height, C.byref(_f3(eye)), factor,
                       self._dev(lo_pos4, "lo_pos4", _F32, 4 * nl), self._dev(lo_nrm4, "lo_nrm4", _F32, 4 * nl),
                       self._dev(lo_alb4, "lo_alb4", _F32, 4 * nl), self._dev(lo_src, "lo_src", _I32, nl)),
                    "mixed_pick_device")

    def mixed_holes(self, max_holes, pos4, nrm4, alb4, px, count, stats=None) -> VctMixedHoles:
        """A vct_mixed_holes over device tensors: the packed hole G-buffer (ceil(max_holes / 64)
        rows of 64 pixels), px (max_holes int32 / uint32), count (1) and stats (4, or None)."""
        n = 4 * 64 * ((max_holes + 63) // 64)
        ho = VctMixedHoles()
        ho.pos4 = self._dev(pos4, "holes.pos4", _F32, n)
        ho.nrm4 = self._dev(nrm4, "holes.nrm4", _F32, n)
        ho.alb4 = self._dev(alb4, "holes.alb4", _F32, n)
        ho.px = self._dev(px, "holes.px", _I32, max_holes)
        ho.count = self._dev(count, "holes.count", _I32, 1)
        ho.stats = self._dev(stats, "holes.stats", _I32, 4)
        ho.max_holes = max_holes
        return ho

    def mixed_upsample_device(self, pos4, nrm4, alb4, width, height, factor, lo_pos4, lo_nrm4, lo_src, lo_plane4,
                              params, plane4, holes):
        """vct_mixed_upsample_device: plane4 from the low plane, and the hole list into `holes`
        (a VctMixedHoles, Context.mixed_holes)."""
        fn = _lib.bind_mixed_extension(self.lib, "vct_mixed_upsample_device")
        if not isinstance(params, VctMixedParams) or not isinstance(holes, VctMixedHoles):
            raise VctError(_EINVAL, "mixed_upsample: expected a VctMixedParams and a VctMixedHoles")
        n = 4 * width * height
        f = factor if factor > 0 else 1
        nl = ((width + f - 1) // f) * ((height + f - 1) // f)
        self._check(fn(self.h, self._dev(pos4, "pos4", _F32, n), self._dev(nrm4, "nrm4", _F32, n),
                       self._dev(alb4, "alb4", _F32, n), width, height, factor,
                       self._dev(lo_pos4, "lo_pos4", _F32, 4 * nl), self._dev(lo_nrm4, "lo_nrm4", _F32, 4 * nl),
                       self._dev(lo_src, "lo_src", _I32, nl), self._dev(lo_plane4, "lo_plane4", _F32, 4 * nl),
                       C.byref(params), self._dev(plane4, "plane4", _F32, n), C.byref(holes)),
                    "mixed_upsample_device")

    def mixed_scatter_device(self, hole_plane4, holes, plane4):
        """vct_mixed_scatter_device: plane4[holes.px[k]] = hole_plane4[k] for the listed holes.
        plane4 must be the frame the list was made for."""
        fn = _lib.bind_mixed_extension(self.lib, "vct_mixed_scatter_device")
        if not isinstance(holes, VctMixedHoles):
            raise VctError(_EINVAL, "mixed_scatter: expected a VctMixedHoles")
        n = 4 * 64 * ((holes.max_holes + 63) // 64)
        self._check(fn(self.h, self._dev(hole_plane4, "hole_plane4", _F32, n), C.byref(holes),
                       self._dev(plane4, "plane4", _F32, 4)), "mixed_scatter_device")

    def trace_mixed_device(self, params, pos4, nrm4, alb4, width, height, eye, diffuse4, spec4, steps_px=None,
                           cone_steps=None, texel_fetches=None, tile_rank=0, tile_world=1, tile_compact=False,
                           variant=0):
        """vct_trace_mixed_device: the mixed-resolution frame (params: Context.mixed_params)."""
        fn = _lib.bind_mixed_extension(self.lib, "vct_trace_mixed_device")
        if not isinstance(params, VctMixedParams):
            raise VctError(_EINVAL, "trace_mixed: expected a VctMixedParams (Context.mixed_params)")
        a = self._mixed_args(pos4, nrm4, alb4, width, height, eye, diffuse4, spec4, steps_px, cone_steps,
                             texel_fetches, tile_rank, tile_world, tile_compact, variant)
        self._check(fn(self.h, C.byref(a), C.byref(params)), "trace_mixed_device")

    # -- temporal accumulation (include/vct_temporal.h) -----------------------
    def temporal_params(self, normal_cos=None, plane_eps=None, max_len=None) -> VctTemporalParams:
        """A vct_temporal_params: the header defaults of this context
        (vct_temporal_default_params), with the fields given replaced."""
        p = VctTemporalParams()
        self._check(_lib.bind_temporal_extension(self.lib, "vct_temporal_default_params")(self.h, C.byref(p)),
                    "temporal_default_params")
        if normal_cos is not None:
            p.normal_cos = normal_cos
        if plane_eps is not None:
            p.plane_eps = plane_eps
        if max_len is not None:
            p.max_len = max_len
        return p

    def temporal_accumulate_device(self, params, pos4, nrm4, width, height, cur, out, out_len, prev_cam=None,
                                   prev_pos4=None, prev_nrm4=None, hist=None, hist_len=None, motion4=None,
                                   stats=None, n_planes=None):
        """vct_temporal_accumulate_device.  cur / hist / out: sequences of up to four float32
        device tensors [height, width, 4] (this frame's planes, last frame's accumulated planes,
        this frame's accumulated planes; out[p] may be cur[p]); hist_len / out_len: int32 or
        uint32 device tensors [height, width]; prev_cam: last frame's camera, or None for a
        frame without history (hist, hist_len and the previous G-buffer are then not read);
        motion4: None, or where each pixel's surface point was last frame (w = 0: nowhere);
        stats: None, or 4 int32 {valid, reused, reset_offscreen, reset_rejected}.
        n_planes: len(cur) unless given."""
        fn = _lib.bind_temporal_extension(self.lib, "vct_temporal_accumulate_device")
        if not isinstance(params, VctTemporalParams):
            raise VctError(_EINVAL, "temporal_accumulate: expected a VctTemporalParams (Context.temporal_params)")
        if hasattr(prev_cam, "to_ctypes"):
            prev_cam = prev_cam.to_ctypes()
        if prev_cam is not None and not isinstance(prev_cam, VctCamera):
            raise VctError(_EINVAL, f"temporal_accumulate: expected a camera or None, got {type(prev_cam).__name__}")
        cur, out, hist = list(cur), list(out), list(hist or [])
        if max(len(cur), len(out), len(hist)) > 4:
            raise VctError(_EINVAL, "temporal_accumulate: more than four planes")
        n, px = 4 * width * height, width * height
        a = VctTemporalArgs()
        a.width, a.height = width, height
        a.pos4, a.nrm4 = self._dev(pos4, "pos4", _F32, n), self._dev(nrm4, "nrm4", _F32, n)
        a.motion4 = self._dev(motion4, "motion4", _F32, n)
        a.prev_cam = C.pointer(prev_cam) if prev_cam is not None else None
        a.prev_pos4, a.prev_nrm4 = self._dev(prev_pos4, "prev_pos4", _F32, n), self._dev(prev_nrm4, "prev_nrm4", _F32, n)
        a.n_planes = len(cur) if n_planes is None else n_planes
        for name, field, planes in (("cur", a.cur4, cur), ("hist", a.hist4, hist), ("out", a.out4, out)):
            for p, t in enumerate(planes):
                field[p] = self._dev(t, f"{name}[{p}]", _F32, n)
        a.hist_len = self._dev(hist_len, "hist_len", _I32, px)
        a.out_len = self._dev(out_len, "out_len", _I32, px)
        a.stats = self._dev(stats, "stats", _I32, 4)
        self._check(fn(self.h, C.byref(a), C.byref(params)), "temporal_accumulate_device")

    # -- dynamic layer (include/vct_dynamic.h) --------------------------------
    def voxelize_dynamic(self, verts: np.ndarray, idx: np.ndarray, tri_material: np.ndarray | None = None,
                         kd4: np.ndarray | None = None):
        """vct_voxelize_dynamic: replace the context's dynamic layer with these triangles (Kd
        materials only); afterwards the grid equals a voxelize of the static mesh followed by
        them.  An empty idx removes the layer.  Inject and build_mips follow as after voxelize."""
        fn = _lib.bind_dynamic_extension(self.lib, "vct_voxelize_dynamic")
        verts = np.ascontiguousarray(verts, dtype=np.float32)
        if verts.ndim != 2 or verts.shape[1] < 3:
            raise VctError(_EINVAL, f"voxelize_dynamic: verts must be [V, F >= 3], got {verts.shape}")
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        mat = None if tri_material is None else np.ascontiguousarray(tri_material, dtype=np.uint32).reshape(-1)
        kd = None if kd4 is None else np.ascontiguousarray(kd4, dtype=np.float32)
        if idx.size % 3:
            raise VctError(_EINVAL, f"voxelize_dynamic: {idx.size} indices, not a multiple of 3")
        if mat is not None and mat.size != idx.size // 3:
            raise VctError(_EINVAL, f"voxelize_dynamic: tri_material has {mat.size} entries for "
                                    f"{idx.size // 3} triangles")
        if kd is not None and (kd.ndim != 2 or kd.shape[1] != 4):
            raise VctError(_EINVAL, f"voxelize_dynamic: kd4 must be [materials, 4], got {kd.shape}")
        self._check(fn(self.h, _fptr(verts), verts.shape[1] * 4, verts.shape[0], _fptr(idx), idx.size,
                       _fptr(mat) if mat is not None else None, _fptr(kd) if kd is not None else None,
                       0 if kd is None else kd.shape[0]), "voxelize_dynamic")

    def voxelize_dynamic_device(self, verts, idx, tri_material=None, kd4=None):
        """vct_voxelize_dynamic_device on torch tensors: verts [V, F >= 3] float32, idx [3T]
        int32 / uint32, tri_material [T] int32 or None, kd4 [M, 4] float32 or None."""
        fn = _lib.bind_dynamic_extension(self.lib, "vct_voxelize_dynamic_device")
        if verts.dim() != 2 or verts.shape[1] < 3:
            raise VctError(_EINVAL, f"voxelize_dynamic_device: verts must be [V, F >= 3], got {tuple(verts.shape)}")
        if str(idx.dtype) in _I64:
            raise VctError(_EINVAL, "voxelize_dynamic_device: idx must be int32 / uint32, not 64-bit")
        n_idx = idx.numel()
        if n_idx % 3:
            raise VctError(_EINVAL, f"voxelize_dynamic_device: {n_idx} indices, not a multiple of 3")
        if kd4 is not None and (kd4.dim() != 2 or kd4.shape[1] != 4):
            raise VctError(_EINVAL, f"voxelize_dynamic_device: kd4 must be [materials, 4], got {tuple(kd4.shape)}")
        nm = 0 if kd4 is None else kd4.shape[0]
        self._check(fn(self.h, self._dev(verts, "verts"), verts.shape[1] * 4, verts.shape[0],
                       self._dev(idx, "idx", _I32), n_idx, self._dev(tri_material, "tri_material", _I32, n_idx // 3),
                       self._dev(kd4, "kd4"), nm), "voxelize_dynamic_device")

    def dynamic_voxels(self) -> int:
        """vct_dynamic_voxels: voxels the dynamic layer in place hits (0 without one)."""
        fn = _lib.bind_dynamic_extension(self.lib, "vct_dynamic_voxels")
        n = C.c_uint32()
        self._check(fn(self.h, C.byref(n)), "dynamic_voxels")
        return int(n.value)

    # -- dynamic objects (include/vct_objects.h) ------------------------------
    def objects_define(self, meshes, kd4: np.ndarray | None = None):
        """vct_objects_define: register the set.  meshes: a sequence of (verts [V, F >= 3]
        float32 in object space, idx [3T], tri_material [T] or None); kd4: the set's one material
        table [M, 4] or None (albedo 1).  Every object starts hidden; an empty sequence removes
        the set."""
        fn = _lib.bind_objects_extension(self.lib, "vct_objects_define")
        kd = None if kd4 is None else np.ascontiguousarray(kd4, dtype=np.float32)
        if kd is not None and (kd.ndim != 2 or kd.shape[1] != 4):
            raise VctError(_EINVAL, f"objects_define: kd4 must be [materials, 4], got {kd.shape}")
        keep, arr = [], (_lib.VctObjectMesh * max(len(meshes), 1))()
        for k, mesh in enumerate(meshes):
            verts, idx = mesh[0], mesh[1]
            mat = mesh[2] if len(mesh) > 2 else None
            verts = np.ascontiguousarray(verts, dtype=np.float32)
            if verts.ndim != 2 or verts.shape[1] < 3:
                raise VctError(_EINVAL, f"objects_define: object {k}: verts must be [V, F >= 3], got {verts.shape}")
            idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
            mat = None if mat is None else np.ascontiguousarray(mat, dtype=np.uint32).reshape(-1)
            if mat is not None and mat.size != idx.size // 3:
                raise VctError(_EINVAL, f"objects_define: object {k}: tri_material has {mat.size} entries for "
                                        f"{idx.size // 3} triangles")
            keep.append((verts, idx, mat))
            arr[k].verts, arr[k].vertex_stride, arr[k].n_verts = verts.ctypes.data, verts.shape[1] * 4, verts.shape[0]
            arr[k].idx, arr[k].n_idx = idx.ctypes.data, idx.size
            arr[k].tri_material = mat.ctypes.data if mat is not None else None
        self._check(fn(self.h, arr, len(meshes), _fptr(kd) if kd is not None else None,
                       0 if kd is None else kd.shape[0]), "objects_define")

    def objects_update(self, ids, poses: np.ndarray):
        """vct_objects_update: place the objects `ids` by `poses`, host arrays: poses is n records
        of 80 bytes (vct.objects.POSE, or any contiguous array of 80 n bytes)."""
        fn = _lib.bind_objects_extension(self.lib, "vct_objects_update")
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        poses = np.ascontiguousarray(poses)
        if poses.nbytes != 80 * ids.size:
            raise VctError(_EINVAL, f"objects_update: {poses.nbytes} bytes of poses for {ids.size} ids (80 each)")
        self._check(fn(self.h, _fptr(ids), _fptr(poses), ids.size), "objects_update")

    def objects_update_device(self, ids, poses):
        """vct_objects_update_device: ids a host array, poses a torch tensor on the context's
        device: [n, 20] float32 (the last four columns hold the bits of visible and reserved) or
        [n, 80] uint8."""
        fn = _lib.bind_objects_extension(self.lib, "vct_objects_update_device")
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        if poses is not None and not isinstance(poses, int):
            per = {"torch.float32": 20, "torch.uint8": 80}.get(str(poses.dtype))
            if per is None or poses.dim() != 2 or poses.shape[1] != per:
                raise VctError(_EINVAL, "objects_update_device: poses must be [n, 20] float32 or [n, 80] uint8, got "
                                        f"{tuple(poses.shape)} {poses.dtype}")
            if poses.shape[0] < ids.size:
                raise VctError(_EINVAL, f"objects_update_device: {poses.shape[0]} poses for {ids.size} ids")
        self._check(fn(self.h, _fptr(ids), self._dev(poses, "poses", ("torch.float32", "torch.uint8")), ids.size),
                    "objects_update_device")

    def objects_stats(self) -> dict:
        """vct_objects_get_stats as a dict (all zero without a set); never waits."""
        fn = _lib.bind_objects_extension(self.lib, "vct_objects_get_stats")
        st = _lib.VctObjectsStats()
        self._check(fn(self.h, C.byref(st)), "objects_stats")
        return {k: int(getattr(st, k)) for k, _ in _lib.VctObjectsStats._fields_ if k != "reserved"}

    # -- object motion (include/vct_motion.h) ---------------------------------
    @staticmethod
    def _pose_records(poses, what: str) -> int:
        """How many 80-byte pose records a [n, 20] float32 / [n, 80] uint8 device tensor holds."""
        per = {"torch.float32": 20, "torch.uint8": 80}.get(str(poses.dtype))
        if per is None or poses.dim() != 2 or poses.shape[1] != per:
            raise VctError(_EINVAL, f"{what}: poses must be [n, 20] float32 or [n, 80] uint8, got "
                                    f"{tuple(poses.shape)} {poses.dtype}")
        return int(poses.shape[0])

    def objects_poses_device(self, out):
        """vct_objects_poses_device: queue a copy of the set's current poses (the last pose given
        to each object, all zero for one never posed) into `out`, a device tensor [n, 20] float32
        or [n, 80] uint8 with n >= n_objects.  Never waits."""
        fn = _lib.bind_motion_extension(self.lib, "vct_objects_poses_device")
        n = self._pose_records(out, "objects_poses_device")
        self._check(fn(self.h, self._dev(out, "out", ("torch.float32", "torch.uint8")), n), "objects_poses_device")

    def objects_motion_device(self, width, height, pos4, tri_id, bary2, prev_poses, motion4, nrm4=None, prev_nrm4=None,
                              stats=None, n_prev=None):
        """vct_objects_motion_device: motion4 (and prev_nrm4 from nrm4, both or neither) for this
        frame's shaded-pass planes from `prev_poses`, the set's poses at last frame's end (a device
        tensor as objects_poses_device fills it; n_prev: its record count unless given).
        stats: None, or 4 int32 {valid, static_or_unmoved, moved, appeared}."""
        fn = _lib.bind_motion_extension(self.lib, "vct_objects_motion_device")
        n = width * height
        a = _lib.VctMotionArgs()
        a.width, a.height = width, height
        a.pos4, a.nrm4 = self._dev(pos4, "pos4", _F32, 4 * n), self._dev(nrm4, "nrm4", _F32, 4 * n)
        a.tri_id, a.bary2 = self._dev(tri_id, "tri_id", _I32, n), self._dev(bary2, "bary2", _F32, 2 * n)
        a.n_prev = self._pose_records(prev_poses, "objects_motion_device") if n_prev is None else n_prev
        a.prev_poses = self._dev(prev_poses, "prev_poses", ("torch.float32", "torch.uint8"))
        a.motion4, a.prev_nrm4 = self._dev(motion4, "motion4", _F32, 4 * n), self._dev(prev_nrm4, "prev_nrm4", _F32, 4 * n)
        a.stats = self._dev(stats, "stats", _I32, 4)
        self._check(fn(self.h, C.byref(a)), "objects_motion_device")

    # -- grid access ------------------------------------------------------
    def download_level(self, level: int, face: int = 0) -> np.ndarray:
        nl, _ = self.level_dims(level)
        out = np.empty((nl, nl, nl, 4), np.float32)
        self._check(self.lib.vct_download_level(self.h, level, face, _fptr(out)), "download_level")
        return out

    def download_pyramid(self) -> list:
        """[level][face] -> (n_l, n_l, n_l, 4) arrays (level 0 has one face)."""
        out = []
        for l in range(self.num_levels):
            _, nf = self.level_dims(l)
            out.append([self.download_level(l, f) for f in range(nf)])
        return out

    def upload_level0(self, r0: np.ndarray):
        r0 = np.ascontiguousarray(r0, dtype=np.float32)
        assert r0.size == self.n ** 3 * 4
        self._check(self.lib.vct_upload_level0(self.h, _fptr(r0)), "upload_level0")

    def level0_device(self):
        p, b = C.c_void_p(), C.c_size_t()
        self._check(self.lib.vct_level0_device(self.h, C.byref(p), C.byref(b)), "level0_device")
        return p.value, b.value

    def copy_level0_to_device(self, dst):
        ptr = self._dev(dst, "dst", _F32, 4 * self.n ** 3)
        self._check(self.lib.vct_copy_level0_to_device(self.h, ptr), "copy_level0_to_device")

    def set_level0_from_device(self, src):
        ptr = self._dev(src, "src", _F32, 4 * self.n ** 3)
        self._check(self.lib.vct_set_level0_from_device(self.h, ptr), "set_level0_from_device")

    def download_voxels(self):
        n = self.n
        ao = np.empty((n, n, n, 4), np.float32)
        nm = np.empty((n, n, n, 4), np.float32)
        self._check(self.lib.vct_download_voxels(self.h, _fptr(ao), _fptr(nm)), "download_voxels")
        return ao, nm

    # -- grid dump / load (vct_save_grid / vct_load_grid; vct.dump wraps them) --------
    def save_grid(self, stem, what: int):
        """vct_save_grid: what = VCT_DUMP_* bits (vct.dump.VOXELS | LEVEL0 | PYRAMID)."""
        self._check(self.lib.vct_save_grid(self.h, os.fsencode(str(stem)), what), "save_grid")

    def load_grid(self, stem):
        """vct_load_grid: replaces this context's grid state with the dump's."""
        self._check(self.lib.vct_load_grid(self.h, os.fsencode(str(stem))), "load_grid")

    def download_accum(self):
        n = self.n
        sums = np.empty((n ** 3, 6), np.int64)
        counts = np.empty((n ** 3,), np.uint32)
        self._check(self.lib.vct_download_accum(self.h, _fptr(sums), _fptr(counts)), "download_accum")
        return sums, counts


def comm_frame_layout(w: int, h: int, nranks: int, rank: int, root: int, lib=None) -> dict:
    """vct_comm_frame_layout: where rank's tiles sit in the frame exchange buffer."""
    from ._lib import VctCommLayout
    lib = lib if lib is not None else _lib.load()
    out = VctCommLayout()
    st = lib.vct_comm_frame_layout(w, h, nranks, rank, root, C.byref(out))
    if st != 0:
        raise VctError(st, "vct_comm_frame_layout")
    return {f: int(getattr(out, f)) for f, _ in VctCommLayout._fields_}
