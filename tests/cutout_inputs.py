"""The catalogue of the cutout tests (vct_spec.h "cutouts"; test infrastructure).

Meshes are gbuffer_inputs.Mesh with a cutout entry per triangle (one material per triangle, so
the table has one entry per triangle too).  Grid n = 16 (one case at 32) over [-2, 2]^3; frames
67 x 45 and 16 x 16, not multiples of the 16-pixel tile, and gbuffer_inputs' stack600 at 48 x 32.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import gbuffer_inputs as GI

F = np.float32
N, G0, E = 16, (-2.0, -2.0, -2.0), 4.0
ROUGH = 0.1
OPAQUE = (-1, 0, 0.5)


# ---------------------------------------------------------------------------
# masks (H, W, 4) uint8; generated
# ---------------------------------------------------------------------------
def _rgba(a):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.uint8)[..., None], np.shape(a) + (4,)))


ONES = _rgba(np.full((2, 2), 255))                                   # M == 1.0f exactly
ZERO = _rgba(np.zeros((2, 2)))
TWO = _rgba(np.array([[0, 255]]))                                    # two texels: M = ax between their centres
ONE = _rgba(np.array([[128]]))                                       # 1 x 1: M = 128 / 255.0f everywhere
STRIPES = _rgba(np.tile(np.array([255, 255, 0, 0] * 2), (8, 1)))     # 8 x 8, columns in pairs
_y, _x = np.mgrid[0:4, 0:4]
CHANNELS = np.stack([(_x % 2) * 255, (_y % 2) * 255, ((_x + _y) % 2) * 255,
                     (((_x - 1.5) ** 2 + (_y - 1.5) ** 2) < 1.5) * 255], -1).astype(np.uint8)   # stripes, stripes, checks, a disc
_rng = np.random.default_rng(11)
NOISE = _rgba(np.where(_rng.random((16, 16)) < 0.55, 255, _rng.integers(0, 200, (16, 16))))   # thin features, soft edges
DIFFUSE = GI.TEXTURE                                                 # 4 x 4 RGBA, every channel busy
M_ONE = F(128) / F(255)                                              # the 1 x 1 mask's value


class Mesh(GI.Mesh):
    """gbuffer_inputs.Mesh with a cutout (map, channel, cutoff) or None per triangle."""

    def __init__(self):
        super().__init__()
        self.cut_of = []

    def tri(self, a, b, c, uv=None, tex=-1, cut=None):
        super().tri(a, b, c, uv=uv, tex=tex)
        self.cut_of.append(cut)
        return self

    def quad(self, p, eu, ev, uv0=(0.0, 0.0), uv1=(1.0, 1.0), cut=None, cut2="same", tex=-1):
        """Two triangles over p + [0, 1] eu + [0, 1] ev with TexCoords uv0 .. uv1; cut2: the second
        triangle's entry when it differs."""
        p, eu, ev = (np.asarray(x, np.float64) for x in (p, eu, ev))
        (u0, v0), (u1, v1) = uv0, uv1
        self.tri(p, p + eu, p + eu + ev, uv=[(u0, v0), (u1, v0), (u1, v1)], tex=tex, cut=cut)
        return self.tri(p, p + eu + ev, p + ev, uv=[(u0, v0), (u1, v1), (u0, v1)], tex=tex,
                        cut=cut if cut2 == "same" else cut2)

    def add(self, other):
        super().add(other)
        self.cut_of += list(getattr(other, "cut_of", [None] * other.n_tri))
        return self

    def arrays(self, table=True):
        """gbuffer_inputs.Mesh.arrays and the table: a (map, channel, cutoff) per material, or None
        (table False, or no triangle has an entry)."""
        v, i, m, kd, mm = super().arrays()
        cuts = [OPAQUE if c is None else c for c in self.cut_of]
        return v, i, m, kd, mm, (cuts if table else None)

    def without_masked(self):
        """arrays() without the triangles that have an entry: the same vertices, materials and Kd,
        fewer indices."""
        v, i, m, kd, mm, _ = self.arrays()
        keep = [k for k, c in enumerate(self.cut_of) if c is None]
        return v, i.reshape(-1, 3)[keep].reshape(-1), m[keep], kd, mm


def from_plain(mesh, cut_of, uv_of=None):
    """A gbuffer_inputs.Mesh with entries (and TexCoords) per triangle."""
    out = Mesh()
    for k in range(mesh.n_tri):
        uv = mesh.uvs[3 * k: 3 * k + 3] if uv_of is None else uv_of(k)
        out.tri(*mesh.v[3 * k: 3 * k + 3], uv=uv, tex=mesh.tex_of[k], cut=cut_of(k))
    return out


@dataclass
class Case:
    name: str
    mesh: Mesh
    textures: list
    cam: object = None            # a frame case when given
    w: int = 67
    h: int = 45
    n: int = N
    k1: bool = True               # compared against cutout_ref.voxelize
    table: bool = True            # False: material_cutout == NULL
    identity: str = ""            # "solid": the mask cannot matter; "dropped": the masked triangles vanish
    covered: object = None        # hand-computed: True = every point of the masked triangles, False = none
    dynamic: Mesh = None          # a dynamic layer (opaque)
    n_tex_after: int = None       # the texture count after a smaller vct_set_textures
    min_rejected: int = 0         # SAT-passing pairs the mask rejects, at least
    min_holes: int = 0            # pixels whose winner differs from the solid frame's, at least
    note: str = ""


CAM = GI.look()                                           # at (0, 0, 3), looking down -z
WALL = dict(p=(-1.9, -1.9, -1.5), eu=(3.8, 0, 0), ev=(0, 3.8, 0))
MID = dict(p=(-1.2, -1.0, -0.45), eu=(2.4, 0, 0), ev=(0, 2.0, 0))
FRONT = dict(p=(-0.9, -0.8, 0.55), eu=(1.9, 0, 0), ev=(0, 1.5, 0.3))     # tilted: crosses voxel layers


def scene(front=None, mid=None, wall_tex=-1, front_tex=-1, front_uv=((0.0, 0.0), (1.0, 1.0)),
          mid_uv=((0.0, 0.0), (2.0, 2.0))):
    """An opaque wall, a quad in front of it and a tilted one in front of that."""
    m = Mesh().quad(**WALL, tex=wall_tex, uv1=(3.0, 3.0))
    m.quad(**MID, uv0=mid_uv[0], uv1=mid_uv[1], cut=mid)
    return m.quad(**FRONT, uv0=front_uv[0], uv1=front_uv[1], cut=front, tex=front_tex)


def _const_uv(u, v=0.5):
    return ((u, v), (u, v))       # every vertex the same TexCoords: M is one value over the triangle


def identity_cases():
    return [
        Case("opaque_table", scene(wall_tex=0), [DIFFUSE], CAM, identity="solid"),
        Case("all255_cutoff1", scene(front=(1, 0, 1.0), mid=(1, 3, 1.0), wall_tex=0), [DIFFUSE, ONES], CAM,
             identity="solid", covered=True),
        Case("all0", scene(front=(1, 2, 0.5), mid=(1, 0, 2.0 ** -20), wall_tex=0), [DIFFUSE, ZERO], CAM,
             identity="dropped", covered=False, min_rejected=50, min_holes=500),
        Case("null_table", scene(front=(1, 0, 0.5), mid=(1, 0, 0.5), wall_tex=0), [DIFFUSE, ZERO], CAM, table=False,
             identity="solid"),
    ]


def threshold_cases():
    half_up = float(np.nextafter(F(0.5), F(1)))
    u_below = float(np.nextafter(F(0.5), F(0)))          # s = 2u - 0.5 = 0.5 - 2^-24, exact
    out = [
        # M = ax = 2u - 0.5 between the two texel centres (u in [0.25, 0.75)), H = 1: M(ay) = M
        Case("two_texel_exact", scene(front=(0, 1, 0.5), front_uv=_const_uv(0.5)), [TWO], CAM, covered=True),
        Case("two_texel_below_u", scene(front=(0, 1, 0.5), front_uv=_const_uv(u_below)), [TWO], CAM, covered=False,
             min_rejected=20, min_holes=200),
        Case("two_texel_below_cutoff", scene(front=(0, 1, half_up), front_uv=_const_uv(0.5)), [TWO], CAM,
             covered=False, min_rejected=20, min_holes=200),
        Case("one_by_one_at", scene(front=(0, 2, float(M_ONE)), front_uv=((-3.25, 7.5), (4.0, -2.0))), [ONE], CAM,
             covered=True),
        Case("one_by_one_above", scene(front=(0, 2, float(np.nextafter(M_ONE, F(1)))),
                                      front_uv=((-3.25, 7.5), (4.0, -2.0))), [ONE], CAM, covered=False,
             min_rejected=20, min_holes=200),
        Case("wrap", scene(front=(0, 0, 0.5), front_uv=((-1.7, -2.3), (1.9, 2.6)), mid=(0, 1, 0.25),
                           mid_uv=((-0.4, 0.3), (-3.1, 1.2))), [STRIPES], CAM, min_rejected=20, min_holes=100),
        Case("nonfinite_uv", _nonfinite_uv(), [CHANNELS], CAM),
        Case("channels", _channels(), [CHANNELS], CAM, min_rejected=20, min_holes=100),
        Case("alpha_of_diffuse", scene(front=(0, 3, 0.5), front_tex=0, front_uv=((0.1, 0.2), (2.3, 1.7))), [DIFFUSE], CAM,
             min_rejected=5, min_holes=50),
    ]
    return out


def _nonfinite_uv():
    m = scene()
    k = m.n_tri
    m.quad(p=(-1.5, 0.9, 0.9), eu=(1.2, 0, 0), ev=(0, 0.8, 0), cut=(0, 2, 0.5))
    m.quad(p=(0.2, 0.9, 0.9), eu=(1.2, 0, 0), ev=(0, 0.8, 0), cut=(0, 0, 0.5))
    for j, bad in enumerate((np.nan, np.inf, -np.inf, np.nan, 0.3, np.inf)):
        u, v = m.uvs[3 * k + j]
        m.uvs[3 * k + j] = (bad, v) if j % 2 == 0 else (u, bad)
    m.uvs[3 * k + 7] = (np.nan, np.nan)
    return m


def _channels():
    m = Mesh().quad(**WALL)
    for c in range(4):
        m.quad(p=(-1.7 + 0.85 * c, -0.9 + 0.1 * c, 0.2 + 0.15 * c), eu=(0.8, 0, 0.1), ev=(0, 1.6, 0), uv1=(1.0, 2.0),
               cut=(0, c, 0.5))
    return m


def k1_cases():
    # one rejected and one accepted pair in the voxels along a quad's diagonal; a masked and an
    # opaque triangle in the same voxels; half a quad rejected as a whole (a two-texel mask
    # stretched over eight voxels: whole voxels lose every pair)
    m = Mesh().quad(p=(-1.6, -1.6, -0.9), eu=(1.5, 0, 0), ev=(0, 1.5, 0.2), cut=(0, 0, 0.5), cut2=(1, 0, 0.5))
    m.quad(p=(0.1, -1.6, 0.3), eu=(1.5, 0, 0), ev=(0, 1.5, 0), uv1=(3.0, 3.0), cut=(2, 0, 0.5))
    m.quad(p=(0.1, -1.6, 0.35), eu=(1.5, 0, 0), ev=(0, 1.5, 0))
    m.quad(p=(-1.8, 0.2, 0.6), eu=(2.0, 0, 0), ev=(0, 1.0, 0), uv0=(0.25, 0.0), uv1=(0.75, 1.0), cut=(3, 0, 0.5))
    out = [Case("k1_pairs", m, [ZERO, ONES, STRIPES, TWO], min_rejected=40)]
    # a K1-skipped triangle (a non-finite q) of a masked material, next to the scene
    m = scene(front=(0, 0, 0.5))
    m.tri((0.0, 0.0, 1.0), (3e38, 0.0, 1.0), (0.0, 1.0, 1.0), uv=[(0, 0), (1, 0), (0, 1)], cut=(0, 1, 0.5))
    m.tri((0.0, 0.0, 1.2), (np.inf, 0.0, 1.2), (0.0, 1.0, 1.2), uv=[(0, 0), (1, 0), (0, 1)], cut=(0, 1, 0.5))
    out.append(Case("k1_skipped", m, [STRIPES], CAM, min_rejected=5))
    # degenerate triangles (den <= 0: b = 0, the first vertex's TexCoords) of masked materials:
    # u0 = 0.75 is texel 1's centre (M = 1), u0 = 0.25 texel 0's (M = 0)
    m = Mesh().quad(**WALL)
    for j, u0 in enumerate((0.75, 0.25)):
        a = np.array((-1.0 + j, -1.1, 0.33 + 0.5 * j))
        m.tri(a, a + (0.9, 0.7, 0.2), a + (1.8, 1.4, 0.4), uv=[(u0, 0.5), (0.5, 0.5), (0.1, 0.5)], cut=(0, 0, 0.5))
        m.tri(a, a, a, uv=[(u0, 0.5)] * 3, cut=(0, 0, 0.5))
    out.append(Case("k1_degenerate", m, [TWO], min_rejected=3))
    out.append(Case("grid32", scene(front=(1, 0, 0.5), mid=(2, 0, 0.5), wall_tex=0), [DIFFUSE, NOISE, STRIPES], n=32,
                    min_rejected=100))
    return out


def _stack600_masked():
    """gbuffer_inputs' stack600 (a tile whose bin spans three staging chunks; the nearest triangle
    in the last chunk, ties across chunks) with triangles 100 .. 599 masked: the masked layers are
    nearer than the opaque ones."""
    plain, cam, w, h = GI._stack600()
    # TexCoords = the vertices' screen positions / 8 (a layer's vertices share one depth, so the
    # TexCoords are affine on the screen): the layers' holes line up, and where the stripes (even
    # layers) and the disc (odd layers) both reject, the nearest opaque layer shows
    src = lambda k: 599 if k == 100 else 598 if k == 300 else k          # the repeats: the same triangle, TexCoords too
    screen = lambda i: [((i % 7) * 0.5, 0.2), (15.8, 0.4 + (i % 5)), (2.0 + (i % 3), 15.7)]
    m = from_plain(plain, lambda k: ((0, k % 4, 0.5) if src(k) % 2 == 0 else (1, 3, 0.5)) if k >= 100 else None,
                   lambda k: [(x / 8.0, y / 8.0) for x, y in screen(src(k))])
    return Case("stack600_masked", m, [STRIPES, CHANNELS], cam, w, h, k1=False, min_holes=15)


def _inside():
    plain = GI.stage()
    rng = np.random.default_rng(9)
    uvs = rng.uniform(-1.0, 2.0, (plain.n_tri, 3, 2))
    pick = rng.random(plain.n_tri) < 0.6
    m = from_plain(plain, lambda k: (int(k % 2), k % 4, 0.4) if pick[k] else None, lambda k: [tuple(x) for x in uvs[k]])
    cam = GI.look(position=(0.3, 0.1, 0.9), yaw=-120.0, pitch=-12.0)
    return Case("inside_stage", m, [NOISE, CHANNELS], cam, k1=False, min_holes=100)


def gbuffer_cases():
    out = [
        # holes in a masked quad show a second masked quad, whose holes show an opaque wall
        Case("nested", scene(front=(1, 0, 0.5), mid=(2, 0, 0.5), wall_tex=0), [DIFFUSE, NOISE, STRIPES], CAM,
             min_rejected=50, min_holes=150),
    ]
    # duplicate coplanar triangles: the lower index rejected, the higher accepted at the same t
    m = Mesh().quad(**WALL)
    tri = ((-1.0, -0.9, 0.4), (1.1, -0.7, 0.4), (0.1, 1.0, 0.6))
    m.tri(*tri, uv=[(0, 0), (1, 0), (0, 1)], cut=(0, 0, 0.5)).tri(*tri, uv=[(0, 0), (1, 0), (0, 1)], cut=(1, 0, 0.5))
    out.append(Case("duplicate_coplanar", m, [ZERO, ONES], CAM, 16, 16, min_holes=10))
    # near = 2: an accepted hit nearer than near hides the wall (background); a rejected one does not
    m = Mesh().quad(**WALL)
    m.quad(p=(-1.0, -0.8, 1.5), eu=(1.0, 0, 0), ev=(0, 1.6, 0), cut=(1, 0, 0.5))
    m.quad(p=(0.0, -0.8, 1.5), eu=(1.0, 0, 0), ev=(0, 1.6, 0), cut=(0, 0, 0.5))
    out.append(Case("near_plane", m, [ZERO, ONES], GI.look(near=2.0), min_holes=100))
    out += [_stack600_masked(), _inside()]
    # a mask index made stale by a smaller vct_set_textures: no mask in the G-buffer pass
    out.append(Case("stale_mask", scene(front=(1, 0, 0.5), mid=(0, 0, 0.5)), [NOISE, STRIPES], CAM, n_tex_after=1,
                    min_rejected=20))
    # a dynamic-layer triangle in front of and one behind a masked quad
    dyn = Mesh().tri((-0.6, -0.5, 1.0), (0.3, -0.4, 1.0), (-0.2, 0.5, 1.1)).tri((-0.3, -0.7, 0.1), (1.0, -0.6, 0.1),
                                                                                  (0.4, 0.7, 0.2))
    out.append(Case("dynamic_layer", scene(front=(0, 0, 0.5)), [NOISE], CAM, dynamic=dyn, min_rejected=10, min_holes=50))
    return out


def all_cases():
    return identity_cases() + threshold_cases() + k1_cases() + gbuffer_cases()


DYN_KD = np.array([0.125, 0.875, 0.375, 1.0], F)          # the Kd of a case's dynamic layer

# one per VCT_EINVAL line of the table rule: (map, channel, cutoff, reserved) of material 0
# (illegal_entry: with the texture count of the moment)
ILLEGAL_TABLES = {
    "map_below_-1": (-2, 0, 0.5, 0), "map_beyond": ("n_tex", 0, 0.5, 0), "channel_4": (0, 4, 0.5, 0),
    "cutoff_zero": (0, 0, 0.0, 0), "cutoff_negative": (0, 0, -0.5, 0), "cutoff_above_1": (0, 0, 1.0000001, 0),
    "cutoff_nan": (0, 0, float("nan"), 0), "cutoff_inf": (0, 0, float("inf"), 0), "reserved": (0, 0, 0.5, 1),
    "no_materials": None,       # a table with n_materials == 0
}


def illegal_entry(name, n_tex):
    e = ILLEGAL_TABLES[name]
    return None if e is None else tuple(n_tex if x == "n_tex" else x for x in e)
