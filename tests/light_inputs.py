"""Hostile lights for K2 (TEST INFRASTRUCTURE): a deterministic catalogue of light directions,
colours, voxel fields and light lists that are legal at the ABI -- or illegal in a way the
"K2 input rule" of include/vct_spec.h names -- but lie outside everything the stock scenes and
their five light directions exercise.

The oracle (vo_inject) defines the result of every legal directional entry, tests/lights_ref.py
that of every light list; the tests compare bit for bit.  What is illegal is predicted here by
the rule itself in numpy float32 (`direction_status`, `colour_status`), never hard-coded.

Directions (`directions()`; each raw, and where still legal scaled by 1e-18 and 1e18):
  axis       the six axis directions, the zero components written +0.0 and -0.0
  planar     one zero component, all sign combinations of the other two
  ties       (+-1, +-1, +-1); (1, 1, 0) and its kin; power-of-two ratios such as (1, 2, 4) and
             (1, 0.5, 0.25), where equal t on two or three axes recurs at every cell
  tiny       per axis and sign one component of 1e-20, 1e-37 (td finite, tm + td overflows),
             2^-126, 1e-40 and 1e-45 (td = +inf: the axis does not move); the other two
             components (0.8, 0.907), both positive and both negative
  edge       float32 squared length the smallest normal, a denormal, 0, the largest finite, +inf
  nonfinite  NaN, +inf, -inf in each component (always VCT_EINVAL)

Colours (`COLOURS`): 0, -0.0, a negative, VCT_COLOR_LIMIT and the next float above it, NaN, +-inf.

Voxel fields (`field(name)`; meshes through K1, on scenes.grid_for_unit_box(n) unless the name
ends in `_exact`, which is g0 = 0, E = n, so that q = p):
  integer_q  a quad through the grid centre with unit normal (1, sqrt 2, 1) / 2 and half-size
             0.45 of the grid's extent: its resolved normal has components 0.49999973, so x + 0.5 + N_x rounds to an
             integer from x = 8 upwards; siblings with the sqrt 2 / 2 component on each axis and
             with the normal negated; n = 16 and n = 32
  faces      a closed box flush with the grid's six faces (q outside: V = 1 before the first
             cell) and the same box one voxel inside; some of its Kd negative, so that an unlit
             voxel's +0 and a product with n.l = 0 differ in their sign bit
  counts     occupied lists of 4095, 4096 and 4097 entries (k2_shade's chunk), lit lists of 255,
             256 and 257 (a 256-thread block), one voxel, every voxel (n = 8), none (a mesh
             outside the grid)
  exits      n = 32: receivers whose walks leave the grid after 1..40 cells, with occluders in
             the first cell, in the last cell before the exit, and in the cell a walk that
             left through +x or +y would index if it wrapped (it must not count)
  sizes      one generic scene (floor, floating box, tilted quad) at n = 4, 8, 16, 64 and 128

Light lists (`light_lists()`, on the field `lists16_exact`): only what tests/test_lights.py and
tests/test_lights_gpu.py do not pin already.  Left out because pinned there: range culling and
the light outside the grid shining in, the light at a voxel centre (exact-zero components of l,
`test_light_set_classes` / `test_inject_lights_matches_reference`), list order, empty lists and
the 64-light limit (`test_inject_lights_errors`, `test_batches_and_limits`).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

F = np.float32
INF = F(np.inf)
VCT_OK, VCT_EINVAL = 0, 1
COLOR_LIMIT = F(2.0 ** 105)          # VCT_COLOR_LIMIT (include/vct_spec.h)
SCALES = (None, 1e-18, 1e18)
DIR_FAMILIES = ("axis", "planar", "ties", "tiny", "edge", "nonfinite")

Direction = namedtuple("Direction", "name family d")          # d: float32[3], as passed to the ABI
Colour = namedtuple("Colour", "name c")
Field = namedtuple("Field", "name family n g0 E verts idx mat kd")
LightList = namedtuple("LightList", "name lights")

KD = np.array([[0.75, 0.5, 0.25, 1.0], [-0.5, 0.25, -1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [0.125, 2.0, 0.5, 1.0]], F)


# ---------------------------------------------------------------------------
# the rule, in float32
# ---------------------------------------------------------------------------
def direction_len(d):
    """len = sqrtf((dx*dx + dy*dy) + dz*dz), every step rounded to float32."""
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def direction_status(d):
    ln = direction_len(d)
    return VCT_OK if (ln > 0 and np.isfinite(ln)) else VCT_EINVAL


def normalised(d):
    d = np.asarray(d, F)
    with np.errstate(all="ignore"):
        return d / direction_len(d)


def colour_status(c):
    c = np.asarray(c, F)
    ok = np.isfinite(c) & ~np.signbit(c) & (c <= COLOR_LIMIT)
    return VCT_OK if bool(ok.all()) else VCT_EINVAL


# ---------------------------------------------------------------------------
# directions
# ---------------------------------------------------------------------------
TINY = (("1e-20", 1e-20), ("1e-37", 1e-37), ("2^-126", 2.0 ** -126), ("1e-40", 1e-40), ("1e-45", 1e-45))


def _raw_directions():
    out = []

    def add(name, family, d):
        out.append(Direction(name, family, np.array(d, F)))

    for a in range(3):
        for s in (1.0, -1.0):
            for zname, z in (("+0", 0.0), ("-0", -0.0)):
                d = [z, z, z]
                d[a] = s
                add(f"axis_{'xyz'[a]}{'+' if s > 0 else '-'}_{zname}", "axis", d)
    for a in range(3):
        for s1 in (1.0, -1.0):
            for s2 in (1.0, -1.0):
                d = [0.0, 0.0, 0.0]
                d[(a + 1) % 3], d[(a + 2) % 3] = s1 * 0.3, s2 * 0.9
                add(f"planar_{'xyz'[a]}0_{'+' if s1 > 0 else '-'}{'+' if s2 > 0 else '-'}", "planar", d)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                add("ties_diag_" + "".join("+" if s > 0 else "-" for s in (sx, sy, sz)), "ties", (sx, sy, sz))
    for a in range(3):
        for s1 in (1.0, -1.0):
            for s2 in (1.0, -1.0):
                d = [0.0, 0.0, 0.0]
                d[(a + 1) % 3], d[(a + 2) % 3] = s1, s2
                add(f"ties_110_{'xyz'[a]}0_{'+' if s1 > 0 else '-'}{'+' if s2 > 0 else '-'}", "ties", d)
    for name, d in (("124", (1, 2, 4)), ("421", (4, 2, 1)), ("1_half_quarter", (1, 0.5, 0.25)),
                    ("-1_2_-4", (-1, 2, -4)), ("214", (2, 1, 4)), ("-0.25_-0.5_1", (-0.25, -0.5, 1))):
        add("ties_pow2_" + name, "ties", d)
    for a in range(3):
        for s in (1.0, -1.0):
            for vname, v in TINY:
                for o in (1.0, -1.0):
                    d = [0.0, 0.0, 0.0]
                    d[a], d[(a + 1) % 3], d[(a + 2) % 3] = s * v, o * 0.8, o * 0.907
                    add(f"tiny_{'xyz'[a]}{'+' if s > 0 else '-'}{vname}_{'pos' if o > 0 else 'neg'}", "tiny", d)
    # squared length: smallest normal, denormal, 0, the largest finite, +inf (one and three components)
    add("edge_sq_min_normal", "edge", (2.0 ** -63, 0.0, 0.0))
    add("edge_sq_denormal", "edge", (0.0, -(2.0 ** -70), 0.0))
    add("edge_sq_denormal3", "edge", (2.0 ** -73, 2.0 ** -73, -(2.0 ** -73)))
    add("edge_sq_zero", "edge", (1e-30, -1e-30, 1e-30))
    add("edge_sq_zero_denormals", "edge", (1e-40, 1e-40, 1e-45))
    add("edge_zero", "edge", (0.0, -0.0, 0.0))
    add("edge_sq_max_finite", "edge", (0.0, 0.0, float(np.nextafter(F(2.0 ** 64), F(0)))))
    add("edge_sq_inf", "edge", (2.0 ** 64, 0.0, 0.0))
    add("edge_sq_sum_inf", "edge", (-1.2e19, 1.2e19, 1.2e19))
    add("edge_max_float", "edge", (3.4028234e38, 1.0, 1.0))
    for a in range(3):
        for vname, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            d = [0.3, 0.5, 0.8]
            d[a] = v
            add(f"nonfinite_{'xyz'[a]}_{vname}", "nonfinite", d)
    return out


_dirs = None


def directions():
    """Every direction raw and scaled by 1e-18 and 1e18 (the product rounded to float32); a
    scaled copy of an illegal direction, or one that the scaling makes illegal, stays in the
    list: its status is the rule's."""
    global _dirs
    if _dirs is None:
        out = []
        for e in _raw_directions():
            for s in SCALES:
                if s is None:
                    out.append(e)
                else:
                    with np.errstate(all="ignore"):
                        out.append(Direction(f"{e.name}*{s:g}", e.family, (e.d * F(s)).astype(F)))
        names = [e.name for e in out]
        assert len(set(names)) == len(names)
        _dirs = out
    return _dirs


def legal_directions(families=DIR_FAMILIES, raw_only=False):
    return [e for e in directions() if e.family in families and direction_status(e.d) == VCT_OK
            and not (raw_only and "*" in e.name)]


def illegal_directions():
    return [e for e in directions() if direction_status(e.d) != VCT_OK]


def sample_directions(per_family=3):
    """A few legal directions of every family (for the large fields): spread over each
    family's list, the td = +inf entries of `tiny` always among them."""
    out = []
    for fam in DIR_FAMILIES:
        leg = legal_directions((fam,))
        if not leg:
            continue
        step = max(1, len(leg) // per_family)
        out += leg[::step][:per_family]
    out += [e for e in legal_directions(("tiny",), raw_only=True) if "1e-40" in e.name and e.name.endswith("-1e-40_pos")]
    seen, uniq = set(), []
    for e in out:
        if e.name not in seen:
            seen.add(e.name)
            uniq.append(e)
    return uniq


COLOURS = [
    Colour("zero", (0.0, 0.0, 0.0)),
    Colour("one", (1.0, 0.5, 0.25)),
    Colour("neg_zero", (1.0, -0.0, 1.0)),
    Colour("negative", (1.0, 1.0, -1e-30)),
    Colour("limit", (float(COLOR_LIMIT), 1.0, float(COLOR_LIMIT))),
    Colour("above_limit", (float(np.nextafter(COLOR_LIMIT, INF)), 1.0, 1.0)),
    Colour("max_float", (1.0, 3.4028234e38, 1.0)),
    Colour("nan", (np.nan, 1.0, 1.0)),
    Colour("+inf", (1.0, np.inf, 1.0)),
    Colour("-inf", (1.0, 1.0, -np.inf)),
]


# ---------------------------------------------------------------------------
# voxel fields
# ---------------------------------------------------------------------------
class _Builder:
    """Triangles in VOXEL units, placed on the unit-box grid (or the exact one)."""

    def __init__(self, n, exact=False):
        self.n = n
        if exact:
            self.g0, self.E = (0.0, 0.0, 0.0), float(n)
        else:
            from vct import scenes
            self.g0, self.E = scenes.grid_for_unit_box(n)
        self.exact = exact
        self.v, self.i, self.m = [], [], []

    def world(self, q):
        q = np.asarray(q, np.float64)
        if self.exact:
            return q.astype(F)
        return (np.asarray(self.g0, np.float64) + q * (self.E / self.n)).astype(F)

    def tri_world(self, p0, p1, p2, mat=0):
        b = len(self.v)
        self.v += [np.asarray(p, F) for p in (p0, p1, p2)]
        self.i += [b, b + 1, b + 2]
        self.m.append(mat % len(KD))

    def tri(self, q0, q1, q2, mat=0):
        self.tri_world(self.world(q0), self.world(q1), self.world(q2), mat)

    def quad(self, o, e1, e2, mat=0):
        """o, o + e1, o + e1 + e2, o + e2: normal along e1 x e2"""
        o, e1, e2 = (np.asarray(a, np.float64) for a in (o, e1, e2))
        self.tri(o, o + e1, o + e1 + e2, mat)
        self.tri(o, o + e1 + e2, o + e2, mat)

    def box(self, lo, hi, mat=0):
        """closed box, normals outward; one material per face pair"""
        lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        d = hi - lo
        ex, ey, ez = (d[0], 0, 0), (0, d[1], 0), (0, 0, d[2])
        self.quad(lo, ey, ez, mat)                          # -x (e1 x e2 = y x z = +x: flip below)
        self.v[-6:] = self.v[-6:][::-1]
        self.quad((hi[0], lo[1], lo[2]), ey, ez, mat)       # +x
        self.quad(lo, ez, ex, mat + 1)                      # -y
        self.v[-6:] = self.v[-6:][::-1]
        self.quad((lo[0], hi[1], lo[2]), ez, ex, mat + 1)   # +y
        self.quad(lo, ex, ey, mat + 2)                      # -z
        self.v[-6:] = self.v[-6:][::-1]
        self.quad((lo[0], lo[1], hi[2]), ex, ey, mat + 2)   # +z

    def speck(self, x, y, z, axis, sign, mat=0, s=0.2):
        """a small triangle through the centre of voxel (x, y, z), normal sign * axis: it
        occupies that voxel alone and resolves to an exactly axis-aligned unit normal"""
        c = np.array([x + 0.5, y + 0.5, z + 0.5])
        u, w = np.zeros(3), np.zeros(3)
        u[(axis + 1) % 3], w[(axis + 2) % 3] = s, s
        if sign < 0:
            u, w = w, u
        self.tri(c - u - w, c + u, c + w, mat)

    def field(self, name, family):
        nv = len(self.v)
        verts = np.array(self.v, F).reshape(nv, 3) if nv else np.zeros((0, 3), F)
        return Field(name, family, self.n, self.g0, self.E, verts, np.array(self.i, np.uint32),
                     np.array(self.m, np.uint32), KD.copy())


def _integer_q(n, big, negate, exact=False):
    """The quad through the grid centre with unit normal (1, sqrt 2, 1) / 2 (the sqrt 2 / 2
    component on axis `big`), half-size 0.45 of the grid's extent (its corners lie outside
    the grid), optionally facing the other way."""
    b = _Builder(n, exact)
    nrm = np.full(3, 0.5)
    nrm[big] = np.sqrt(2.0) / 2.0
    t1 = np.zeros(3)
    t1[(big + 1) % 3], t1[(big + 2) % 3] = 1.0 / np.sqrt(2.0), -1.0 / np.sqrt(2.0)
    t2 = np.cross(nrm, t1)
    if negate:
        t1, t2 = t2, t1
    half = 0.45 * n                                          # 0.45 of the grid's extent, in voxels
    c = np.full(3, n / 2.0)
    p = [c - half * t1 - half * t2, c + half * t1 - half * t2, c + half * t1 + half * t2, c - half * t1 + half * t2]
    b.tri(p[0], p[1], p[2], 0)
    b.tri(p[0], p[2], p[3], 3)
    return b


def _generic(n, exact=False):
    """floor, a floating box that shadows it, a tilted quad: something of everything"""
    b = _Builder(n, exact)
    s = n / 16.0
    b.quad((1.2 * s, 1.6 * s, 1.2 * s), (0, 0, 13.5 * s), (13.5 * s, 0, 0), 0)          # floor, normal +y
    b.box((5.3 * s, 6.2 * s, 4.4 * s), (9.6 * s, 9.7 * s, 8.3 * s), 1)
    b.quad((2.1 * s, 3.0 * s, 11.0 * s), (9.0 * s, 6.0 * s, 1.5 * s), (-1.0 * s, 5.0 * s, 3.0 * s), 3)
    b.quad((13.4 * s, 2.0 * s, 2.0 * s), (0, 9.0 * s, 0), (0, 0, 9.0 * s), 2)             # wall, normal +x ... -x side
    return b


def exit_rows(axis=0):
    """The exits field's rows for a light along +x (axis 0) or +y (axis 1): (k, a, b, kind).
    Axis 0: the receiver sits in voxel (31 - k, a, b) with normal +x, so its walk starts in
    cell x = 32 - k and tests k cells before it leaves through +x (k = 1..31).  kind: None, or
    where the row's occluder sits: 'first' (the start cell), 'last' (cell x = 31), 'wrap' (cell
    (0, a + 1, b): what x = 32 of row a is in a packed index, a being even).  Axis 1 is the same
    layout with (x, y, z) -> (y, z, x): the rows of the two never meet (their z differ)."""
    rows = []
    for k in range(1, 32):
        a, b = (2 if axis == 0 else 4) * (k % 8), 2 + 4 * (k // 8)
        rows.append((k, a, b, None))
        rows.append((k, a, b + 16, ("first", "last", "wrap")[k % 3]))
    return rows


def exit_cell(axis, x_, y_, z_):
    c = [0, 0, 0]
    c[axis], c[(axis + 1) % 3], c[(axis + 2) % 3] = x_, y_, z_
    return tuple(c)


def _exits():
    b = _Builder(32)
    for axis in (0, 1):
        for k, y, z, kind in exit_rows(axis):
            b.speck(*exit_cell(axis, 31 - k, y, z), axis, 1.0, k)
            if kind == "first" and k > 1:
                b.speck(*exit_cell(axis, 32 - k, y, z), (axis + 1) % 3, 1.0, 1)
            elif kind == "last" and k > 1:
                b.speck(*exit_cell(axis, 31, y, z), (axis + 1) % 3, -1.0, 2)
            elif kind == "wrap":
                b.speck(*exit_cell(axis, 0, y + 1, z), axis, -1.0, 3)
    return b


_fields = {}
FIELD_NAMES = (
    ["integer_q%d_%s%s" % (n, "xyz"[big], "-" if neg else "+") for n in (16, 32) for big in range(3) for neg in (0, 1)]
    + ["integer_q16_y+_exact", "faces8_flush", "faces8_inside", "counts64_occ4095", "counts64_occ4096",
       "counts64_occ4097", "counts16_lit255", "counts16_lit256", "counts16_lit257", "counts8_one", "counts8_full",
       "counts8_none", "exits32", "sizes4", "sizes8", "sizes16", "sizes64", "sizes128", "lists16_exact"])
SMALL_FIELDS = [f for f in FIELD_NAMES if not any(f.startswith(p) for p in ("counts64", "sizes64", "sizes128"))]


def field(name):
    if name in _fields:
        return _fields[name]
    fam = "integer_q" if name.startswith("integer_q") else name.split("_")[0].rstrip("0123456789")
    if name.startswith("integer_q"):
        n = 16 if name.startswith("integer_q16") else 32
        tag = name.split("_")[2]
        b = _integer_q(n, "xyz".index(tag[0]), tag[1] == "-", exact=name.endswith("_exact"))
    elif name.startswith("faces8"):
        b = _Builder(8)
        if name.endswith("flush"):
            b.box((0, 0, 0), (8, 8, 8), 0)
        else:
            b.box((1.5, 1.5, 1.5), (6.5, 6.5, 6.5), 0)         # the voxel shell one voxel inside
    elif name.startswith("counts64"):
        b = _Builder(64)
        if name.endswith("4095"):
            b.quad((0, 0, 10.5), (64, 0, 0), (0, 62.5, 0), 0)               # 64 x 63 voxels
            b.quad((0, 63.25, 10.5), (62.5, 0, 0), (0, 0.5, 0), 3)          # 63 more
        else:
            b.quad((0, 0, 10.5), (64, 0, 0), (0, 64, 0), 0)                 # 64 x 64
            if name.endswith("4097"):
                b.speck(20, 30, 40, 2, -1.0, 1)
    elif name.startswith("counts16"):
        b = _Builder(16)
        if name.endswith("255"):
            b.quad((0, 0, 5.5), (16, 0, 0), (0, 14.5, 0), 0)                # 16 x 15, normal +z
            b.quad((0, 15.25, 5.5), (14.5, 0, 0), (0, 0.5, 0), 3)           # 15 more
        else:
            b.quad((0, 0, 5.5), (16, 0, 0), (0, 16, 0), 0)
            if name.endswith("257"):
                b.speck(7, 9, 11, 2, 1.0, 1)
    elif name == "counts8_one":
        b = _Builder(8)
        b.speck(3, 4, 5, 1, 1.0, 1)
    elif name == "counts8_full":
        b = _Builder(8)
        for z in range(8):
            b.quad((0, 0, z + 0.5), (8, 0, 0), (0, 8, 0), z)
    elif name == "counts8_none":
        b = _Builder(8)
        b.quad((-9, -9, -5.5), (30, 0, 0), (0, 30, 0), 0)
        b.speck(8, 3, 3, 0, 1.0, 1)
        b.speck(3, -1, 3, 1, -1.0, 2)
    elif name == "exits32":
        b = _exits()
    elif name.startswith("sizes"):
        b = _generic(int(name[5:]))
    elif name == "lists16_exact":
        b = _generic(16, exact=True)
        for x, y, z, ax, sg in ((2, 12, 3, 0, 1.0), (12, 12, 3, 2, 1.0), (3, 12, 13, 1, -1.0), (8, 13, 8, 1, 1.0)):
            b.speck(x, y, z, ax, sg, 2)                   # axis-aligned receivers: q at cell centres
    else:
        raise KeyError(name)
    _fields[name] = b.field(name, fam)
    return _fields[name]


def voxels(O, f):
    """The oracle's K1 of a field -> (albedo_occ, normal), read-only."""
    sums, counts = O.voxelize(f.n, f.g0, f.E, f.verts, f.idx, f.mat, f.kd)
    ao, nm = O.resolve(f.n, sums, counts)
    ao.setflags(write=False)
    nm.setflags(write=False)
    return ao, nm


# ---------------------------------------------------------------------------
# the walk once more, with its cell count (the catalogue's conditions use it; the CPU tests
# hold it against the oracle and tests/lights_ref.py)
# ---------------------------------------------------------------------------
def walk_count(occ, q, l, nan_rule="spec"):
    """A.3 from q [R, 3] along l [R, 3] (or [3]) over occ [n, n, n] (z, y, x), all receivers in
    lockstep -> (V [R] float32, cells [R]: the cells tested, `left` [R]: the walk left the grid).
    nan_rule "spec": the K2 input rule (an axis whose td is not finite does not move).
    "parent": the walk as the oracle had it before that rule, where a NaN t makes every
    comparison false and the walk steps z, then y (kept to count what the rule changed)."""
    n = occ.shape[0]
    q = np.asarray(q, F)
    R = q.shape[0]
    l = np.broadcast_to(np.asarray(l, F), (R, 3))
    V, cells, left = np.zeros(R, F), np.zeros(R, np.int64), np.zeros(R, bool)
    with np.errstate(all="ignore"):
        v = np.floor(q).astype(np.int64)
        outside = np.any((v < 0) | (v >= n), axis=1)
        V[outside] = 1.0
        left[outside] = True
        s = np.where(l > 0, 1, np.where(l < 0, -1, 0)).astype(np.int64)
        td = np.where(s != 0, F(1.0) / np.abs(l), INF).astype(F)
        if nan_rule == "spec":
            s = np.where(td == INF, 0, s)
        vf = v.astype(F)
        tm = np.where(s > 0, ((vf + F(1.0)) - q) * td, np.where(s < 0, (q - vf) * td, INF)).astype(F)
    act = np.flatnonzero(~outside)
    v, s, td, tm = v[act], s[act], td[act], tm[act]
    while act.size:
        cells[act] += 1
        hit = occ[v[:, 2], v[:, 1], v[:, 0]]
        ax = np.where((tm[:, 0] <= tm[:, 1]) & (tm[:, 0] <= tm[:, 2]), 0, np.where(tm[:, 1] <= tm[:, 2], 1, 2))
        rows = np.arange(act.size)
        v[rows, ax] += s[rows, ax]
        with np.errstate(all="ignore"):
            tm[rows, ax] = tm[rows, ax] + td[rows, ax]
        out = ~hit & np.any((v < 0) | (v >= n), axis=1)
        V[act[out]] = 1.0
        left[act[out]] = True
        keep = ~hit & ~out
        act, v, s, td, tm = act[keep], v[keep], s[keep], td[keep], tm[keep]
    return V, cells, left


def receivers(ao, nm):
    """(z, y, x) of the occupied voxels, their q = ((float)x + 0.5f) + N, N and A."""
    z, y, x = np.nonzero(ao[..., 3] != 0)
    N = np.ascontiguousarray(nm[z, y, x, :3], F)
    q = (np.stack([x, y, z], axis=1).astype(F) + F(0.5)) + N
    return (z, y, x), q, N, np.ascontiguousarray(ao[z, y, x, :3], F)


def inject_batch(ao, nm, dirs, color=(1.0, 1.0, 1.0), nan_rule="spec"):
    """vct_inject_directional for many raw directions at once -> [D, n, n, n, 4] float32: one
    lockstep walk over every (lit voxel, direction) pair."""
    n = ao.shape[0]
    occ = ao[..., 3] != 0
    (z, y, x), q, N, A = receivers(ao, nm)
    c = np.asarray(color, F)
    out = np.zeros((len(dirs), n, n, n, 4), F)
    out[:, z, y, x, 3] = 1.0
    with np.errstate(all="ignore"):
        L = np.stack([normalised(d) for d in dirs])                                    # [D, 3]
        ndl = (N[None, :, 0] * L[:, None, 0] + N[None, :, 1] * L[:, None, 1]) + N[None, :, 2] * L[:, None, 2]
        di, ri = np.nonzero(ndl > 0)
        V, _, _ = walk_count(occ, q[ri], L[di], nan_rule)
        val = ((A[ri] * c[None, :]) * ndl[di, ri, None]) * V[:, None]
    out[di, z[ri], y[ri], x[ri], :3] = val
    return out


def integer_q_light(name):
    """The light that meets the integer q of an integer_q field: -1e-40 (td = +inf, and
    0 * inf at an integer q) on the first axis whose normal component is 0.5, the other two
    components (0.8, 0.907) with the normal's sign.  -> (axis, float32[3])"""
    tag = name.split("_")[2]
    big, neg = "xyz".index(tag[0]), tag[1] == "-"
    a = [i for i in range(3) if i != big][-1]            # z for the x and y quads, y for the z quad
    o = -1.0 if neg else 1.0
    d = [0.0, 0.0, 0.0]
    d[a], d[(a + 1) % 3], d[(a + 2) % 3] = -1e-40, o * 0.8, o * 0.907
    return a, np.array(d, F)


# ---------------------------------------------------------------------------
# light lists (field lists16_exact: g0 = 0, E = 16, so world = voxel units and q = p)
# ---------------------------------------------------------------------------
def light_lists():
    import vct
    n = 16.0
    one = (1.0, 0.75, 0.5)
    ulp_up = lambda v: float(np.nextafter(F(v), INF))
    P, S, D = vct.point_light, vct.spot_light, vct.directional_light
    out = []

    def add(name, *lights):
        out.append(LightList(name, list(lights)))

    # r2 overflows: l = d / inf = 0 (skipped by n.l), or inf / inf = NaN where pL itself overflows
    add("far_r2_finite", P((1e18, 2e18, 1e18), one, 3e38))
    add("far_r2_overflow", P((1e19, 2e19, 1e19), one, 3e38), S((1e19, 2e19, 1e19), (-1, -2, -1), one, 3e38,
                                                                 cos_inner=0.9, cos_outer=0.1))
    add("far_pl_overflow", P((3e38, 3e38, 3e38), one, 3e38), P((-3e38, 8.0, 8.0), one, 1.0))
    # range: inv_rr = +inf (u = inf, w = 0: every receiver culled) and inv_rr = 0 (no window)
    add("range_tiny", P((8.2, 12.3, 7.9), one, 1e-25))
    add("range_huge", P((8.2, 12.3, 7.9), one, 1e30))
    add("range_denormal_rr", P((8.2, 12.3, 7.9), one, 1e-20))        # rv * rv a denormal: inv_rr = +inf
    # spot: cos_inner - cos_outer one ulp (inv_span 2^24), and one denormal ulp above 0 (inv_span =
    # +inf): the receivers at q.y = 12.5 see the light at pL.y = 12.5 exactly at cd = cos_outer = 0,
    # (cd - cos_outer) * inv_span = 0 * inf
    add("spot_ulp_half", S((8.3, 14.8, 8.4), (0.1, -1.0, 0.05), one, 40.0, cos_inner=ulp_up(0.5), cos_outer=0.5))
    add("spot_ulp_zero", S((7.5, 12.5, 7.5), (0.0, -1.0, 0.0), one, 40.0, cos_inner=1e-45, cos_outer=0.0))
    # positions
    add("inside_occupied", P((7.4, 8.1, 6.2), one, 30.0), P((8.5, 1.9, 8.5), one, 30.0))   # in the box, in the floor
    add("on_faces", P((0.0, 9.0, 8.0), one, 40.0), P((8.0, 16.0, 8.0), one, 40.0), P((16.0, 16.0, 0.0), one, 40.0))
    add("outside", P((-3.0, 20.0, 8.0), one, 60.0), S((8.0, 40.0, 8.0), (0.0, -1.0, 0.0), one, 90.0, 10.0, 25.0))
    # the receiver's own cell: the speck at (8, 13, 8) has q = (8.5, 14.5, 8.5); t_lim below the first t
    add("own_cell", P((8.75, 14.75, 8.625), one, 20.0), P((8.5, 14.5, 8.5), one, 20.0), P((8.5, 14.9375, 8.5), one, 20.0))
    # one or two coordinates shared with receivers' q (specks: q at cell centres x.5; floor: q.y = 3.0 or so)
    add("shared_coords", P((3.5, 12.5, 9.5), one, 30.0), P((12.5, 12.5, 4.5), one, 30.0), P((8.5, 9.5, 8.5), one, 30.0),
        P((12.5, 6.5, 4.5), one, 30.0))
    everything = [l for e in out for l in e.lights]
    add("all_together", *everything, D((0.8, 0.907, -1e-40), (0.5, 0.5, 0.5)))
    assert len(everything) + 1 <= 64
    return out


def filler_lights():
    """33 lights in front of the light under test, so that it is light 33 of 34 and falls into
    the second 32-light batch: 32 point lights that every receiver culls (range 1e-25) and,
    among them, one dim directional light, so that level 0 is not zero before the last light."""
    import vct
    out = [vct.point_light((8.0 + 0.01 * i, 9.0, 7.0), (1.0, 1.0, 1.0), 1e-25) for i in range(33)]
    out[7] = vct.directional_light((0.3, 0.9, 0.2), (0.25, 0.5, 0.125))
    return out


FILLER_DIR, FILLER_COLOUR = (0.3, 0.9, 0.2), (0.25, 0.5, 0.125)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def gbuffer_of(f, ao, nm, w=32):
    """A G-buffer whose pixels are the field's occupied voxels (vct_spec.h "light bounces":
    P_c = g0_c + ((float)x_c + 0.5f) * hh, N and A the voxel's), padded with background pixels
    to full rows of w.  On an `_exact` field (g0 = 0, hh = 1) the composite's q = (P - g0) *
    inv_h + N is K2's q bit for bit, integer components included.  -> pos4, nrm4, alb4 [h, w, 4]"""
    (z, y, x), q, N, A = receivers(ao, nm)
    hh = F(f.E) / F(f.n)
    P = np.asarray(f.g0, F)[None, :] + (np.stack([x, y, z], axis=1).astype(F) + F(0.5)) * hh
    h = (len(x) + w - 1) // w + 1
    pos, nrm, alb = (np.zeros((h * w, 4), F) for _ in range(3))
    k = len(x)
    pos[:k, :3], pos[:k, 3] = P, 1.0
    nrm[:k, :3] = N
    alb[:k, :3], alb[:k, 3] = A, 1.0
    return pos.reshape(h, w, 4), nrm.reshape(h, w, 4), alb.reshape(h, w, 4)
