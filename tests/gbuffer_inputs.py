"""Hostile inputs of the two G-buffer passes (vct_spec.h "G-buffer input rule"; test
infrastructure): named cases (mesh, camera, frame size), the legal ones and the illegal cameras
of the rule, one per clause.  tests/test_gbuffer_inputs.py checks them on the CPU,
tests/test_gbuffer_inputs_gpu.py on the HIP passes; tests/gbuffer_ref.py is the reference.

Every triangle has its own material with a distinct Kd, so the albedo plane names the winner.
Every mesh is voxelized into the same tiny grid (N = 8 over [-2, 2]^3): the G-buffer passes read
the mesh records of the last voxelize call, the grid itself is not looked at.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F = np.float32
N, G0, E = 8, (-2.0, -2.0, -2.0), 4.0
ROUGH = 0.1
ORTHO_EPS, ZOOM_MIN, ZOOM_MAX, MAX_DIM, FOCAL_LIMIT = 2.0 ** -20, F(2.0 ** -10), F(179.0), 16384, 2.0 ** 17


def ulps(x, k):
    """x moved by k float32 steps (k < 0: toward -inf)."""
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


# ---------------------------------------------------------------------------
# cameras
# ---------------------------------------------------------------------------
class Cam:
    """A vct_camera in float32 fields."""

    def __init__(self, position, front, up, right, zoom=45.0, near=0.1, far=100.0):
        self.position, self.front, self.up, self.right = (np.array(v, F) for v in (position, front, up, right))
        self.zoom, self.near, self.far = F(zoom), F(near), F(far)

    def to_ctypes(self):
        from vct import VctCamera
        c = VctCamera()
        for name in ("position", "front", "up", "right"):
            getattr(c, name)[:] = [float(x) for x in getattr(self, name)]
        c.zoom_deg, c.near_plane, c.far_plane = float(self.zoom), float(self.near), float(self.far)
        return c

    def but(self, **kw):
        c = Cam(self.position, self.front, self.up, self.right, self.zoom, self.near, self.far)
        for k, v in kw.items():
            setattr(c, k, np.array(v, F) if np.ndim(v) else F(v))
        return c


def look(position=(0.0, 0.0, 3.0), yaw=-90.0, pitch=0.0, **kw):
    """The project's own Camera (float64-normalised, rounded to float32) as a Cam."""
    from vct.camera import Camera
    c = Camera(position=position, yaw=yaw, pitch=pitch)
    return Cam(position, c.front, c.up, c.right, **kw)


def ray64(cam, w, h, X, Y):
    """float64 direction (not normalised, D.front = 1) of the ray through screen point (X, Y)
    (pixel x has its centre at X = x + 0.5)."""
    th = np.tan(np.radians(float(cam.zoom)) / 2)
    a, b = (2 * X / w - 1) * th * (w / h), (1 - 2 * Y / h) * th
    return cam.front.astype(np.float64) + a * cam.right.astype(np.float64) + b * cam.up.astype(np.float64)


# ---------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------
class Mesh:
    def __init__(self):
        self.v, self.uvs, self.tex_of = [], [], []

    def tri(self, a, b, c, uv=None, tex=-1):
        self.v += [a, b, c]
        self.uvs += list(uv) if uv is not None else [(0.0, 0.0)] * 3
        self.tex_of.append(tex)
        return self

    def quad(self, p, eu, ev, **kw):
        p, eu, ev = (np.asarray(x, np.float64) for x in (p, eu, ev))
        return self.tri(p, p + eu, p + eu + ev, **kw).tri(p, p + eu + ev, p + ev, **kw)

    def box(self, lo, hi):
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        d = hi - lo
        ex, ey, ez = np.diag(d)
        for p, a, b in ((lo, ex, ey), (lo, ey, ez), (lo, ez, ex), (hi, -ey, -ex), (hi, -ez, -ey), (hi, -ex, -ez)):
            self.quad(p, a, b)
        return self

    def add(self, other):
        self.v += other.v
        self.uvs += other.uvs
        self.tex_of += other.tex_of
        return self

    @property
    def n_tri(self):
        return len(self.tex_of)

    def arrays(self):
        """(verts [V, 14] float32 with the TexCoords in columns 6:8, idx, tri_material, kd4,
        material_map or None): one material per triangle, Kd distinct and exact in float32."""
        n = self.n_tri
        with np.errstate(all="ignore"):
            verts = np.zeros((3 * n, 14), F)
            verts[:, :3] = np.array(self.v, np.float64).astype(F)
            verts[:, 6:8] = np.array(self.uvs, F)
        t = np.arange(n)
        kd = np.stack([(t % 16 + 1) / 16, (t // 16 % 16 + 1) / 16, (t // 256 + 1) / 4, np.ones(n)], 1).astype(F)
        tex = np.array(self.tex_of, np.int32)
        return verts, np.arange(3 * n, dtype=np.uint32), t.astype(np.uint32), kd, (tex if (tex >= 0).any() else None)


def stage(seed=3, extra=20):
    """A room around the default camera (its walls cross cz = 0), two boxes and some loose triangles."""
    m = Mesh().box((-1.75, -1.25, -1.5), (2.0, 1.5, 3.5))
    m.box((-0.9, -1.25, -0.6), (-0.2, 0.1, 0.2)).box((0.3, -1.25, 0.4), (0.8, -0.5, 1.1))
    rng = np.random.default_rng(seed)
    for _ in range(extra):
        c = rng.uniform((-1.5, -1.0, -1.2), (1.5, 1.0, 1.5))
        m.tri(*(c + rng.uniform(-0.45, 0.45, (3, 3))))
    return m


def wall(z, half=4.0):
    """A quad facing +z; off centre, so that its diagonal does not pass through the frame's centre."""
    return Mesh().quad((-half, -half + 0.9, z), (2 * half, 0, 0), (0, 2 * half, 0))


TEXTURE = (np.arange(4 * 4 * 4, dtype=np.uint32).reshape(4, 4, 4) * 37 % 251).astype(np.uint8)


@dataclass
class Case:
    name: str
    mesh: Mesh
    cam: Cam
    w: int
    h: int
    benign: bool = False          # every hit reprojects to its pixel centre (reference-like camera and mesh)
    f64: str = ""                 # non-empty: why the case is left out of the float64 comparison
    thr: float = 1e-4             # robustness margin of the float64 comparison
    finding: int = 0              # 1 / 2 / 3: the parent's k_bin_rect loses a winner on this case
    min_hits: int = 1             # pixels with a hit (the case shows what it is about)
    textures: list = field(default_factory=list)


def _needles(cam, w, h):
    """Thin triangles whose projected boxes end on the boundary between tile 0 and tile 1: their
    long edge lies on the rays of pixel centres 15.5 and 16.5 (both axes)."""
    m = Mesh()
    P = cam.position.astype(np.float64)
    at = lambda X, Y, z: P + ray64(cam, w, h, X, Y) * z
    for k, (c0, c1) in enumerate(((15.5, 15.5 - 0.02), (16.5, 16.5 + 0.02), (15.5, 15.5 + 0.02), (16.5, 16.5 - 0.02))):
        z = 1.5 + 0.1 * k
        m.tri(at(c0, 2.5, z), at(c0, 30.5, z), at(c1, 17.0, z))          # vertical needle, x on the boundary
        m.tri(at(3.5, c0, z + 0.05), at(40.5, c0, z + 0.05), at(20.0, c1, z + 0.05))   # horizontal one
    return m


def _subpixel(cam, w, h):
    """Triangles smaller than a pixel: around pixel corners (between centres: never hit by an
    ideal ray) and around pixel centres (one pixel each)."""
    m = Mesh()
    P = cam.position.astype(np.float64)
    at = lambda X, Y: P + ray64(cam, w, h, X, Y) * 2.0
    for i in range(12):
        X, Y = 5.0 + 4 * i, 7.0 + 3 * i                                     # a pixel corner
        m.tri(at(X - 0.3, Y - 0.3), at(X + 0.3, Y - 0.3), at(X, Y + 0.3))
        X, Y = 6.5 + 4 * i, 4.5 + 3 * i                                     # a pixel centre
        m.tri(at(X - 0.2, Y - 0.2), at(X + 0.2, Y - 0.2), at(X, Y + 0.2))
    return m


def _at_focal_limit():
    """A tall narrow frame just inside VCT_GBUF_FOCAL_LIMIT (s M^2 = 1.30e5 of 1.31e5), a basis
    skewed just inside the bound and an eye away from the origin: triangles whose vertices lie on
    pixel-centre rays, so that every rounding of the projection shows against the margin."""
    base = look(position=(37.25, -12.125, 55.5), yaw=-61.0, pitch=17.0, zoom=0.92)
    f, r, u = (v.astype(np.float64) for v in (base.front, base.right, base.up))
    cam = base.but(right=r + 0.8e-6 * f, up=u - 0.8e-6 * f + 0.8e-6 * r)
    w, h = 64, 2048
    P = cam.position.astype(np.float64)
    at = lambda X, Y, z: P + ray64(cam, w, h, X, Y) * z
    m = Mesh()
    rng = np.random.default_rng(17)
    for i in range(48):
        x0, y0 = rng.integers(0, w - 8), rng.integers(0, h - 40)
        z = rng.uniform(5.0, 90.0)
        m.tri(at(x0 + 0.5, y0 + 0.5, z), at(x0 + 0.5 + rng.integers(1, 8), y0 + 0.5, z * rng.uniform(0.9, 1.1)),
              at(x0 + 0.5, y0 + 0.5 + rng.integers(1, 40), z * rng.uniform(0.9, 1.1)))
    return m, cam, w, h


def _stack600():
    """600 triangles over the first tile, nearer with the index: the nearest sits in the last of
    the three kRayChunk = 256 chunks; triangle 100 repeats triangle 599 (a tie across chunks, which
    goes to the lower index), triangle 300 repeats 598."""
    cam, w, h = look(), 48, 32
    P = cam.position.astype(np.float64)
    m = Mesh()
    tris = []
    for i in range(600):
        z = 2.0 - i / 600.0               # the depth: the last triangle is the nearest
        at = lambda X, Y: P + ray64(cam, w, h, X, Y) * z
        x0 = (i % 7) * 0.5
        tris.append((at(x0, 0.2), at(15.8, 0.4 + (i % 5)), at(2.0 + (i % 3), 15.7)))
    tris[100], tris[300] = tris[599], tris[598]
    for t in tris:
        m.tri(*t)
    return m, cam, w, h


def _far_cases():
    out = []
    for plane in ("far", "near"):
        for k in (-3, -2, -1, 0, 1, 2, 3):
            cam = look(**{plane: ulps(2.0, k)}) if plane == "far" else look(near=ulps(2.0, k))
            out.append(Case(f"{plane}_{k:+d}ulp", wall(1.0).add(wall(0.5)), cam, 24, 16,
                            f64="the depth sits within ulps of the plane", finding=2 if plane == "far" and k < 0 else 0,
                            min_hits=0))
    return out


def legal_cases():
    d = look()
    c = []
    st = stage()
    # ---- cameras ----
    c.append(Case("near_wall_5e-6", wall(3 - 5e-6, 1.0).add(wall(2.0)), d, 48, 32, finding=1, min_hits=0,
                  f64="every pixel's nearest hit is nearer than near"))
    below = Mesh().tri((-50, 3 - 1e-6, -50), (50, 3 - 1e-6, -50), (0, 3 - 1e-6, 60)).add(wall(1.0))
    c.append(Case("plane_1e-6_under_eye", below, look(position=(0.0, 3.0, 3.0)), 48, 80, finding=1,
                  f64="t of the grazing plane is rounding noise"))
    through = Mesh().tri((-50, 3, -50), (50, 3, -50), (0, 3, 60)).add(wall(1.0))
    c.append(Case("plane_through_eye", through, look(position=(0.0, 3.0, 3.0), pitch=7.0), 48, 32,
                  f64="t = 0 up to rounding"))
    c.append(Case("eye_on_vertex", Mesh().tri((0, 0, 3), (-1, -1, 1), (1.5, -0.5, 0.5)).add(wall(-1.0)),
                  look(yaw=-80.0), 48, 32, f64="the eye is a vertex: t of that triangle is rounding noise"))
    c.append(Case("eye_in_plane", Mesh().tri((-1, 0, 2), (1, 0, 2), (0, 0, 0.5)).tri((-1, 0.25, 2.5), (1, 0.5, 1), (0, 3, 0))
                  .add(wall(-1.0)), look(position=(0.0, 0.0, 3.0), yaw=-93.0, pitch=0.0), 67, 45,
                  f64="edge-on triangle: det is rounding noise on the row through it"))
    c += _far_cases()
    # every vertex one ulp beyond far = 100, while some pixels' computed depth is not
    c.append(Case("far_100_wall_1ulp_beyond", wall(3.0 - float(ulps(100.0, 1)), 60.0), d, 48, 32, finding=2,
                  f64="the depth sits within ulps of the plane"))
    c.append(Case("near_eq_far", wall(1.0), look(near=2.0, far=2.0), 24, 16, min_hits=0,
                  f64="the depth sits on both planes"))
    c.append(Case("pitch_+89", st, look(pitch=89.0), 67, 45))
    c.append(Case("pitch_-89", st, look(pitch=-89.0), 67, 45))
    c.append(Case("zoom_min", wall(1.0), look(zoom=ulps(ZOOM_MIN, 1)), 3, 2, thr=1e-2))
    c.append(Case("zoom_max", st, look(zoom=ulps(ZOOM_MAX, -1)), 48, 32))
    c.append(Case("eye_1e4_zoom_min", st, look(position=(0.8, 0.9, 1e4), zoom=ulps(ZOOM_MIN, 1), far=2e4), 3, 2,
                  thr=0.01))
    c.append(Case("eye_1e4", st, look(position=(0.0, 0.0, 1e4), zoom=0.01, far=2e4), 24, 16, thr=0.01))
    big = Mesh()
    rng = np.random.default_rng(5)
    for _ in range(24):   # coordinates on the float32 grid at 1e6 (ulp 1/16)
        ctr = np.round(rng.uniform(-6, 6, 3) * 4) / 4
        big.tri(*(1e6 + ctr + np.round(rng.uniform(-3, 3, (3, 3)) * 4) / 4))
    c.append(Case("eye_1e6", big, look(position=(1e6, 1e6, 1e6 + 16.0)), 48, 32, thr=1e-3))
    skew = d.but(right=d.right.astype(np.float64) + 0.8e-6 * d.front.astype(np.float64))
    c.append(Case("skew_inside_bound", st, skew, 67, 45))
    # ---- meshes ----
    t3 = ((-1, -1, 0), (1, -1, 0.5), (0, 1, 0.25))
    c.append(Case("duplicate_coplanar", Mesh().tri(*t3).tri(*t3).tri(t3[0], t3[2], t3[1]).add(wall(-1.0)), d, 67, 45,
                  f64="ties in t"))
    fan = Mesh()
    ring = [(-1, -1), (1, -1), (1, 1), (0, 1.25), (-1, 1)]
    for i in range(5):   # a fan around (0, 0): the centre pixel of an odd frame is on the shared vertex,
        a, b = ring[i], ring[(i + 1) % 5]   # the centre column on the shared edge x = 0
        fan.tri((0, 0, 1), (a[0], a[1], 1), (b[0], b[1], 1))
    c.append(Case("centre_on_edge_and_vertex", fan, d, 67, 45, f64="pixel centres on a shared edge and vertex"))
    e = Mesh()
    for k, a in enumerate((0.0, 1e-7, -3e-7, 1e-5, 0.02)):   # planes through the eye, tilted by a
        e.tri((-1 + 0.1 * k, -0.5 + a * 2, 1), (-0.6 + 0.1 * k, 0.7 + a * 2, 1), (-0.8 + 0.1 * k, 0.1 * (1 + a), 2.5))
    c.append(Case("edge_on", e.add(wall(-1.0)), look(yaw=-97.0, pitch=3.0), 67, 45,
                  f64="edge-on triangles: det is rounding noise"))
    col = Mesh()   # collinear vertices in general position: n = 0 up to rounding, det is noise
    for k in range(6):
        a, dirn = np.array((-1.2 + 0.4 * k, -0.9, 1.0 + 0.1 * k)), np.array((0.31 + 0.05 * k, 0.77, -0.23))
        col.tri(a, a + 0.7 * dirn, a + 1.9 * dirn)
    c.append(Case("collinear", col.add(wall(-1.0)), look(yaw=-84.0, pitch=-6.0), 67, 45))
    c.append(Case("needles_tile_boundary", _needles(d, 67, 45).add(wall(-1.0)), d, 67, 45,
                  f64="needles along pixel-centre rays: every hit is an edge hit"))
    c.append(Case("subpixel", _subpixel(d, 67, 45).add(wall(-1.0)), d, 67, 45))
    huge = Mesh()
    for s, y in ((1e15, -1.0), (1e18, -1.5)):
        huge.tri((-s, y, -s), (s, y, -s), (0.0, y, s))
    c.append(Case("huge_1e15_1e18", huge.add(Mesh().box((-0.5, -1.0, -0.5), (0.5, 0.0, 0.5))), d, 67, 45, thr=1e-3))
    def zeros():   # zero-area triangles, and three that K1 skips (an all-zero record)
        z = Mesh().tri((0, 0, 1), (0, 0, 1), (1, 0, 1)).tri((-1, 0, 1), (0, 0, 1), (1, 0, 1))
        z.tri((0.5, 0.5, 1), (0.5, 0.5, 1), (0.5, 0.5, 1))
        z.tri((np.nan, 0, 1), (1, 0, 1), (0, 1, 1)).tri((0, 0, 1), (np.inf, 0, 1), (0, 1, 1))
        return z.tri((0, 0, 1), (1, 0, 1), (0, -np.inf, 1))
    c.append(Case("zero_area_and_k1_zero", zeros().tri((-1, -1, 0.5), (1, -1, 0.5), (0, 1, 0.5)), d, 67, 45))
    c.append(Case("zero_records_behind_eye", zeros().add(wall(1.0)), look(position=(0.0, 0.0, -3.0), yaw=90.0), 24, 16))
    tex = Mesh().quad((-1, -1, 1), (2, 0, 0), (0, 2, 0), uv=None)
    tex.uvs = [(0, 0), (1.5, 0), (1.5, 1.5), (0, 0), (1.5, 1.5), (0, 1.5)]
    tex.tex_of = [0, 0]
    c.append(Case("textured", tex.add(wall(-1.0)), d, 24, 16, textures=[TEXTURE]))
    m600, cam600, w600, h600 = _stack600()
    c.append(Case("stack600", m600, cam600, w600, h600, f64="duplicated nearest triangles: ties across chunks"))
    ml, cl, wl, hl = _at_focal_limit()
    c.append(Case("margin_at_focal_limit", ml, cl, wl, hl, finding=3, min_hits=100,
                  f64="long triangles seen edge-on through a long lens: u and v are rounding noise"))
    # ---- frames ----
    for w, h in ((1, 1), (17, 1), (1, 33)):
        c.append(Case(f"frame_{w}x{h}", st, d, w, h, thr=1e-4))
    c.append(Case("frame_67x45", st, d, 67, 45, benign=True))
    c.append(Case("frame_67x45_inside", st, look(position=(0.2, -0.3, 0.5), yaw=-120.0, pitch=20.0), 67, 45, benign=True))
    c.append(Case("frame_520x500", st, look(position=(0.4, 0.2, 2.5), yaw=-100.0, pitch=-8.0), 520, 500, benign=True))
    c.append(Case("frame_16384x2", st, look(zoom=0.02), MAX_DIM, 2, thr=1e-3))
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


# ---------------------------------------------------------------------------
# illegal cameras: one per clause of the rule
# ---------------------------------------------------------------------------
def illegal_cases():
    """[(name, cam, w, h)]: each is VCT_EINVAL with nothing written."""
    d = look()
    f64 = lambda v: np.asarray(v, np.float64)
    out = [
        ("position_nan", d.but(position=(0.0, np.nan, 3.0)), 24, 16),
        ("position_inf", d.but(position=(np.inf, 0.0, 3.0)), 24, 16),
        ("front_nan", d.but(front=(np.nan, 0.0, -1.0)), 24, 16),
        ("up_inf", d.but(up=(0.0, np.inf, 0.0)), 24, 16),
        ("right_nan", d.but(right=(1.0, 0.0, np.nan)), 24, 16),
        ("front_length_2", d.but(front=2 * f64(d.front)), 24, 16),
        ("up_length_1+2e-6", d.but(up=(1 + 1e-6) * f64(d.up)), 24, 16),
        ("right_zero", d.but(right=(0.0, 0.0, 0.0)), 24, 16),
        ("skew_front_right_1.2e-6", d.but(right=f64(d.right) + 1.2e-6 * f64(d.front)), 24, 16),
        ("skew_front_up_1.2e-6", d.but(up=f64(d.up) - 1.2e-6 * f64(d.front)), 24, 16),
        ("skew_up_right_1.2e-6", d.but(up=f64(d.up) + 1.2e-6 * f64(d.right)), 24, 16),
        ("zoom_at_min", d.but(zoom=ZOOM_MIN), 3, 2),
        ("zoom_at_max", d.but(zoom=ZOOM_MAX), 24, 16),
        ("zoom_0", d.but(zoom=0.0), 24, 16),
        ("zoom_negative", d.but(zoom=-45.0), 24, 16),
        ("zoom_180", d.but(zoom=180.0), 24, 16),
        ("zoom_nan", d.but(zoom=np.nan), 24, 16),
        ("zoom_inf", d.but(zoom=np.inf), 24, 16),
        ("near_negative", d.but(near=-0.1), 24, 16),
        ("near_above_far", d.but(near=2.0, far=ulps(2.0, -1)), 24, 16),
        ("near_nan", d.but(near=np.nan), 24, 16),
        ("far_inf", d.but(far=np.inf), 24, 16),
        ("far_nan", d.but(far=np.nan), 24, 16),
        ("w_0", d, 0, 16),
        ("h_0", d, 24, 0),
        ("w_above_max", d.but(zoom=0.02), MAX_DIM + 1, 2),
        ("h_above_max", d.but(zoom=0.02), 2, MAX_DIM + 1),
        ("focal_limit", d.but(zoom=0.01), 64, 48),
        ("focal_limit_wide", d.but(zoom=178.5), 1024, 512),
    ]
    return out
