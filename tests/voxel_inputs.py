"""Hostile triangles for K1 (TEST INFRASTRUCTURE): a deterministic catalogue of meshes that are
legal at the ABI (include/vct.h, "Input rule") but lie outside every family the procedural
scenes draw from, the exact-arithmetic overlap sets that pin the float32 SAT, and the
seeded adversarial triangles of the band test.

The oracle (vo_voxelize) defines the result of every entry; the tests compare bit for bit.

Entries are written in VOXEL units (the q of vct_spec.h) and placed twice per grid size:
  placement "exact": g0 = 0, E = n, so inv_h = 1 and q = p exactly;
  placement "unit":  scenes.grid_for_unit_box(n), an inexact inv_h (q lands within an ulp
                     or two of the stated value; what the name promises is then asserted as a
                     class: outside stays outside, a point stays a point, non-finite stays so).
`build()` asserts these placement conditions on q computed in the kernels' operation order.

Families (`catalogue`):
  lattice     vertices exactly on integer planes and +-1, +-2 ulp off them; triangles lying in
              x = 0, x = k, x = n; quads whose diagonal runs through voxel corners
  degenerate  points (inside / face / edge / corner), collinear (axis, oblique), two equal
              vertices, an area below binary32 resolution (zero face normal)
  sliver      slivers of aspect 1 : 2^20, triangles below 2^-10 voxel, one triangle covering the
              grid, one spanning +-1e4 E that cuts it
  outside     wholly outside by 0.5 h, 3 h, 1e3 E, 1e10 E per axis and sign; a finite 3e38
              vertex (q overflows where inv_h > 1); straddling each face; touching q = 0 / q = n
  nonfinite   NaN, +Inf, -Inf in each component of each vertex slot; all nine NaN; Inf - Inf
              edges; each next to a clean triangle in the same voxel
  materials   negative, zero, denormal, 32767.99 Kd; mixed signs over many hits of one voxel
  counts      a giant triangle between one-candidate triangles; consecutive triangles with
              1..9 candidates (kCandPerThread = 8); `count_mesh` builds the n_tri cases
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

F = np.float32
FAMILIES = ("lattice", "degenerate", "sliver", "outside", "nonfinite", "materials", "counts")
PLACEMENTS = ("exact", "unit")
# kind: "live" (may cover voxels), "none" (adds nothing by construction), "clean" (a plain
# neighbour of a hostile entry).  hits: the number of voxels covered at placement "exact"
# (None: not stated).  raw: world-space vertices used as they are (q is then ignored)
Entry = namedtuple("Entry", "name family q kd kind hits raw")
Mesh = namedtuple("Mesh", "verts idx mat kd names entries n g0 E placement")

# ---- the exact-arithmetic band ---------------------------------------------------------
# K1's SAT compares p = u . a with rad = 0.5 (|ux| + |uy| + |uz|) in binary32.  With unit
# roundoff 2^-24, a three-term dot product of vectors u, a carries an absolute error of at most
# about 3 * 2^-24 |u| |a|, and a = q - c itself one more rounding: as a distance in voxels
# (divide by |u|) that is about 4 * 2^-24 |a|.  Inside the grids of this project |a| <= 64 sqrt3
# ~ 111, so the error stays below 4 * 2^-24 * 111 ~ 2.6e-5 < 2^-14 = 6.1e-5: the float32 test
# can differ from exact arithmetic only for contacts thinner than DELTA.  A triangle whose
# vertices lie farther out (the +-1e4 E entry) gets the same bound at its own |a| (`delta_for`).
DELTA_BITS = 14
SCALE_BITS = 60                      # the q of every finite entry are integers times 2^-60
S = 1 << SCALE_BITS


def delta_for(q, n):
    """DELTA (as an integer scaled by S) for a triangle with binary32 vertices q (3, 3):
    2^-14 wherever |a| <= 64 sqrt3, 4 * 2^-24 * max|a| beyond (rounded up to a power of two)."""
    amax = float(np.max(np.abs(np.asarray(q, np.float64) - n / 2.0))) * 3 ** 0.5 + n * 3 ** 0.5 / 2
    bits = DELTA_BITS
    while 4.0 * 2.0 ** -24 * amax >= 2.0 ** -bits:
        bits -= 1
    return S >> bits if bits >= 0 else S << -bits


def grid_of(n, placement):
    if placement == "exact":
        return (0.0, 0.0, 0.0), float(n)
    from vct import scenes
    return scenes.grid_for_unit_box(n)


def q_of(p, g0, E, n):
    """q = (p - g0) * inv_h in the kernels' binary32 operation order; p: (..., 3)."""
    inv_h = F(n) / F(E)
    with np.errstate(all="ignore"):
        return (np.asarray(p, F) - np.asarray(g0, F)) * inv_h


def _world(q, g0, E, n):
    """The binary32 world position whose q (kernel order) is nearest the stated one."""
    q = np.asarray(q, np.float64)
    if g0 == (0.0, 0.0, 0.0) and E == float(n):
        return q.astype(F)
    h = float(F(E)) / n
    out = np.empty(q.shape, F)
    inv_h = F(n) / F(E)
    for i, (t, g) in enumerate(zip(q.ravel(), np.tile(np.asarray(g0, np.float64), q.size // 3))):
        if not np.isfinite(t):
            out.flat[i] = t
            continue
        c = F(g + t * h)
        best, cand = None, c
        for step in range(-6, 7):
            x = c
            for _ in range(abs(step)):
                x = np.nextafter(x, F(np.inf if step > 0 else -np.inf))
            with np.errstate(all="ignore"):
                err = abs(float((x - F(g)) * inv_h) - t)
            if best is None or err < best:
                best, cand = err, x
        out.flat[i] = cand
    return out


def _ulps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return float(x)


def _kd_for(i):
    """A distinct, ordinary Kd per entry (multiples of 1/64 in [0.125, 0.875])."""
    return ((8 + (i * 5) % 49) / 64.0, (8 + (i * 11) % 49) / 64.0, (8 + (i * 17) % 49) / 64.0)


def catalogue(n):
    """-> list of Entry for grid size n (voxel units)."""
    out = []
    nan, inf = float("nan"), float("inf")

    def add(name, family, q, kind="live", hits=None, kd=None, raw=None):
        out.append(Entry(name, family, None if q is None else [list(map(float, v)) for v in q],
                         kd, kind, hits, raw))

    def tiny(cx, cy, cz, s=0.125):
        """a small triangle strictly inside the voxel that holds (cx, cy, cz)"""
        return [(cx, cy, cz), (cx + s, cy, cz), (cx, cy + s, cz + s)]

    # ---- lattice ------------------------------------------------------------------
    add("lat_on", "lattice", [(2, 2, 2), (4, 2, 2), (2, 4, 2)])
    for k in (1, -1, 2, -2):
        z = _ulps(3.0, k)
        add(f"lat_ulp{k:+d}", "lattice", [(1.25, 1.25, z), (2.75, 1.25, z), (1.25, 2.75, z)])
    for name, x in (("plane_x0", 0.0), ("plane_xk", 5.0), ("plane_xn", float(n))):
        add(name, "lattice", [(x, 1.5, 1.5), (x, 3.5, 1.5), (x, 1.5, 3.5)])
    zq = n - 1.5
    add("diag_a0", "lattice", [(1, 1, zq), (5, 1, zq), (5, 5, zq)])
    add("diag_a1", "lattice", [(1, 1, zq), (5, 5, zq), (1, 5, zq)])
    add("wall_a0", "lattice", [(1, 1, 1), (1, 5, 1), (1, 5, 5)])
    add("wall_a1", "lattice", [(1, 1, 1), (1, 5, 5), (1, 1, 5)])

    # ---- degenerate -----------------------------------------------------------------
    add("pt_inside", "degenerate", [(2.5, 2.5, 2.5)] * 3, hits=1)
    add("pt_face", "degenerate", [(3, 2.5, 4.5)] * 3, hits=2)
    add("pt_edge", "degenerate", [(3, 3, 5.5)] * 3, hits=4)
    add("pt_corner", "degenerate", [(6, 6, 6)] * 3, hits=8)
    add("col_axis", "degenerate", [(1.5, 5.5, 5.5), (2.5, 5.5, 5.5), (4.5, 5.5, 5.5)], hits=4)
    add("col_oblique", "degenerate", [(0.5, 0.5, 6.5), (1.5, 1.5, 6.5), (3.5, 3.5, 6.5)])
    add("two_equal", "degenerate", [(5.5, 1.5, 1.5), (5.5, 1.5, 1.5), (6.5, 2.5, 1.5)])
    c, d = 2.0 ** -30, 2.0 ** -30 * (1 + 2.0 ** -22)
    add("tiny_area", "degenerate", [(c, c, c), (d, c, c), (c, d, c)])

    # ---- sliver / tiny / giant ------------------------------------------------------
    add("sliver_axis", "sliver", [(1.5, 1.5, 4.5), (5.5, 1.5, 4.5), (3.5, 1.5 + 2.0 ** -18, 4.5)])
    add("sliver_oblique", "sliver", [(0.75, 0.75, 0.75), (6.75, 5.75, 4.75), (6.75, 5.75 + 2.0 ** -17, 4.75)])
    add("tiny_inside", "sliver", tiny(4.5, 4.5, 4.5, 2.0 ** -12), hits=1)
    add("tiny_corner", "sliver", [(4, 4, 4), (4 + 2.0 ** -12, 4, 4), (4, 4 + 2.0 ** -12, 4)])
    add("giant_cover", "sliver", [(-n, -n, 2.5), (3 * n, -n, 2.5), (-n, 3 * n, 2.5)], hits=n * n)
    g = 1e4 * n
    add("giant_cut", "sliver", [(-g, -g, 1.5), (g, -g, n - 1.5), (0, g, n / 2)])

    # ---- outside ----------------------------------------------------------------------
    m = n // 2
    for a, an in enumerate("xyz"):
        for s, sn in ((1, "+"), (-1, "-")):
            for dist, dn in ((0.5, "half"), (3.0, "3h"), (1e3 * n, "1e3E"), (1e10 * n, "1e10E")):
                v = float(F(n + dist)) if s > 0 else -dist
                tri = []
                for o1, o2 in ((0.25, 0.25), (0.75, 0.25), (0.25, 0.75)):
                    p = [m + o1, m + o2, m + o1]
                    p[a] = v
                    p[(a + 1) % 3], p[(a + 2) % 3] = m + o1, m + o2
                    tri.append(tuple(p))
                add(f"out_{an}{sn}_{dn}", "outside", tri, kind="none")
            lo, hi = (n - 0.75, n + 0.75) if s > 0 else (-0.75, 0.75)
            tri = []
            for t, o1, o2 in ((lo, 0.25, 0.25), (hi, 0.5, 0.25), (lo, 0.25, 0.75)):
                p = [0.0, 0.0, 0.0]
                p[a], p[(a + 1) % 3], p[(a + 2) % 3] = t, 1 + o1, 1 + o2
                tri.append(tuple(p))
            add(f"straddle_{an}{sn}", "outside", tri, hits=1)
    big = 3e38
    add("out_overflow", "outside", None, kind="none",
        raw=[(big, 0.1, 0.1), (big, 0.2, 0.1), (big, 0.1, 0.2)])
    add("touch_q0", "outside", [(0, 2.5, 2.5), (-1, 2.25, 2.5), (-1, 2.75, 2.5)], hits=1)
    add("touch_qn", "outside", [(n, 2.5, 2.5), (n + 1, 2.25, 2.5), (n + 1, 2.75, 2.5)], hits=1)

    # ---- non-finite (each next to a clean triangle in the same voxel) ----------------
    cases = []
    for s in range(3):
        for a, an in enumerate("xyz"):
            for val, vn in ((nan, "nan"), (inf, "pinf"), (-inf, "ninf")):
                cases.append((f"nf_{vn}_v{s}{an}", [(s, a, val)]))
    cases.append(("nf_all_nan", [(k, a, nan) for k in range(3) for a in range(3)]))
    cases.append(("nf_inf_minus_inf", [(0, 0, inf), (1, 0, inf)]))
    cases.append(("nf_inf_to_ninf", [(0, 1, inf), (2, 1, -inf)]))
    for i, (name, edits) in enumerate(cases):
        vx, vy, vz = 1 + i % (n - 2), 1 + (i // (n - 2)), n - 2
        # general position: with axis-parallel edges the SAT's own 0 x inf products would reject
        # most of these triangles even without the rule; this shape would cover a row of voxels
        tri = [[vx + 0.25, vy + 0.25, vz + 0.25], [vx + 0.75, vy + 0.5, vz + 0.5], [vx + 0.5, vy + 0.75, vz + 0.75]]
        for k, a, val in edits:
            tri[k][a] = val
        add(name, "nonfinite", tri, kind="none")
        add(name + ".clean", "nonfinite", tiny(vx + 0.375, vy + 0.375, vz + 0.375), kind="clean", hits=1)

    # ---- materials ----------------------------------------------------------------------
    for i, (name, kd) in enumerate((("kd_neg", (-0.5, -0.25, -1.0)), ("kd_zero", (0.0, 0.0, 0.0)),
                                    ("kd_denorm", (1e-40, -1e-40, 1e-45)),
                                    ("kd_max", (32767.99, -32767.99, 32767.99)))):
        add(name, "materials", tiny(1.25 + i, 2.25, 3.25), hits=1, kd=kd)
    for i in range(12):      # one voxel, twelve hits: r and b sum below zero, g above
        kd = (-0.75, 0.5, -0.125) if i % 3 else (0.25, -0.625, 0.0625)
        add(f"kd_mix{i}", "materials", tiny(5.125 + 0.03125 * i, 2.25, 3.25), hits=1, kd=kd)

    # ---- counts -----------------------------------------------------------------------------
    add("one_a", "counts", tiny(1.25, 1.25, 6.25), hits=1)
    add("giant_between", "counts", [(-n, -n, 5.5), (3 * n, -n, 5.5), (-n, 3 * n, 5.5)], hits=n * n)
    add("one_b", "counts", tiny(2.25, 1.25, 6.25), hits=1)
    for k in range(1, 10):   # k candidates along x, all of them hit
        x1 = min(0.5 + (k - 1), n - 0.5)
        kk = int(x1 - 0.5) + 1
        add(f"cand_{k}", "counts", [(0.5, 2.5 + 0.125, 0.25 + 0.5 * (k % 2)), (x1, 2.5 + 0.125, 0.25 + 0.5 * (k % 2)),
                                    (0.5, 2.5 + 0.25, 0.25 + 0.5 * (k % 2))], hits=kk)
    return out


def build(families, n, placement="exact", exclude=(), only_kind=None):
    """The mesh of the catalogue entries of `families` (in catalogue order), one material per
    triangle.  exclude: entry names left out; only_kind: keep only entries of these kinds.
    -> Mesh; verts (V, 3) float32, idx (3T,) uint32, mat (T,) uint32, kd (T, 4) float32, names[t]
    the entry of triangle t.  The placement conditions are asserted here."""
    g0, E = grid_of(n, placement)
    cat = catalogue(n)
    sel = [(i, e) for i, e in enumerate(cat) if e.family in families and e.name not in exclude
           and (only_kind is None or e.kind in only_kind)]
    verts, kd, names, ents = [], [], [], []
    for i, e in sel:
        p = np.asarray(e.raw, F) if e.raw is not None else _world(e.q, g0, E, n)
        verts.append(p.reshape(3, 3))
        kd.append(tuple(e.kd if e.kd is not None else _kd_for(i)) + (1.0,))
        names.append(e.name)
        ents.append(e)
    t = len(sel)
    verts = np.concatenate(verts).astype(F) if t else np.zeros((0, 3), F)
    mesh = Mesh(verts, np.arange(3 * t, dtype=np.uint32), np.arange(t, dtype=np.uint32),
                np.asarray(kd, F).reshape(-1, 4), names, ents, n, g0, E, placement)
    _check_placement(mesh)
    return mesh


def _check_placement(mesh):
    n, exact = mesh.n, mesh.placement == "exact"
    q = q_of(mesh.verts, mesh.g0, mesh.E, n).reshape(-1, 3, 3)
    p = mesh.verts.reshape(-1, 3, 3)
    for e, qt, pt in zip(mesh.entries, q, p):
        name = e.name
        fin = bool(np.isfinite(qt).all())
        if e.raw is None and exact and e.family != "nonfinite":
            assert np.array_equal(qt, np.asarray(e.q, F)), name          # q = p: what the entry states
        if e.raw is None and fin:
            assert np.abs(qt.astype(np.float64) - np.asarray(e.q)).max() <= 2e-6 * max(1.0, np.abs(e.q).max()), name
            assert all(float(v) * S == int(float(v) * S) for v in qt.ravel()), name   # exact-arithmetic domain
        if e.family == "nonfinite" and e.kind == "none":
            assert not fin and np.array_equal(np.isfinite(qt), np.isfinite(np.asarray(e.q))), name
        elif name == "out_overflow":
            assert np.isfinite(pt).all(), name
            assert (not fin) if F(n) / F(mesh.E) > 1.2 else (qt[:, 0] > n + 1).all(), name
        else:
            assert fin, name
        if e.family == "outside" and e.kind == "none" and name != "out_overflow":
            a = "xyz".index(name[4])
            assert (qt[:, a] > n).all() if name[5] == "+" else (qt[:, a] < 0).all(), name
        if name.startswith("pt_"):
            assert (qt == qt[0]).all(), name
        if name.startswith("touch_q") and exact:
            assert qt[0, 0] == (0 if name.endswith("0") else n), name
        if name == "tiny_area":           # the face normal's length is zero in binary32 (len == 0 branch)
            e1, e2 = pt[1] - pt[0], pt[2] - pt[0]
            with np.errstate(all="ignore"):
                fn = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                               e1[0] * e2[1] - e1[1] * e2[0]], F)
                assert np.sqrt((fn[0] * fn[0] + fn[1] * fn[1]) + fn[2] * fn[2]) == 0, name
        if e.kind == "clean" or name in ("tiny_inside", "pt_inside") or name.startswith("kd_"):
            assert (np.floor(qt) == np.floor(qt[0])).all() and (qt != np.floor(qt)).all(), name   # inside one voxel
    for e, qt in zip(mesh.entries, q):    # a hostile non-finite entry shares its voxel with its clean neighbour
        if e.kind == "clean" and e.name[:-len(".clean")] in mesh.names:
            host = q[mesh.names.index(e.name[:-len(".clean")])]
            okv = np.isfinite(host)
            assert (np.floor(host[okv]) == np.floor(np.broadcast_to(qt[0], host.shape)[okv])).all(), e.name


def count_mesh(n_tri, n, placement="exact"):
    """n_tri triangles, most of them outside the grid (zero candidates), with tiny one-voxel
    triangles scattered among them and one in last place.  -> (Mesh, expected counts [n^3])."""
    g0, E = grid_of(n, placement)
    stride = 877 if n_tri > 4096 else 97
    t = np.arange(n_tri)
    live = (t % stride == 5 % max(min(stride, n_tri), 1)) | (t == n_tri - 1)
    vox = np.stack([(t * 7) % n, (t * 3) % n, (t * 5) % n], 1).astype(np.float64)
    base = np.where(live[:, None], vox + 0.25, np.array([n + 3.25, n / 2 + 0.25, n / 2 + 0.25]))
    q = np.stack([base, base + [0.125, 0, 0], base + [0, 0.125, 0.125]], 1)          # (T, 3, 3)
    verts = _world_fast(q.reshape(-1, 3), g0, E, n)
    qk = q_of(verts, g0, E, n).reshape(-1, 3, 3)
    assert (np.floor(qk[live]) == vox[live][:, None]).all() and (qk[live] != np.floor(qk[live])).all()
    assert (qk[~live][..., 0] > n + 2).all()
    expect = np.bincount((vox[live] @ [1, n, n * n]).astype(np.int64), minlength=n ** 3).astype(np.uint32)
    kd = np.array([_kd_for(i) + (1.0,) for i in range(4)], F)
    mesh = Mesh(verts, np.arange(3 * n_tri, dtype=np.uint32), (t % 4).astype(np.uint32), kd,
                None, None, n, g0, E, placement)
    return mesh, expect


def _world_fast(q, g0, E, n):
    if g0 == (0.0, 0.0, 0.0) and E == float(n):
        return q.astype(F)
    return (np.asarray(g0, np.float64) + q * (float(F(E)) / n)).astype(F)


def empty_mesh(n, placement="exact"):
    g0, E = grid_of(n, placement)
    return Mesh(np.zeros((0, 3), F), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.ones((1, 4), F),
                [], [], n, g0, E, placement)


# ---------------------------------------------------------------------------
# exact arithmetic: Python ints scaled by 2^60
# ---------------------------------------------------------------------------
def _ints(qt):
    return [[int(float(v) * S) for v in row] for row in np.asarray(qt, F)]


def cand_box(qt, n, pad=1):
    """The voxels of the triangle's candidate box, padded by `pad`, clipped to the grid."""
    qt = np.clip(np.asarray(qt, np.float64), -2.0, n + 2.0)
    lo = np.maximum(np.ceil(qt.min(0)).astype(np.int64) - 1 - pad, 0)
    hi = np.minimum(np.floor(qt.max(0)).astype(np.int64) + pad, n - 1)
    return lo, hi


def exact_overlap(Q, cx, cy, cz, half):
    """Closed 13-axis SAT of the triangle Q (3 x 3 ints, scaled by S) against the box of centre
    (cx, cy, cz) and half-size `half` (ints scaled by S), in exact integer arithmetic."""
    a = [(v[0] - cx, v[1] - cy, v[2] - cz) for v in Q]
    for i in range(3):
        if min(a[0][i], a[1][i], a[2][i]) > half or max(a[0][i], a[1][i], a[2][i]) < -half:
            return False
    e = [tuple(a[(k + 1) % 3][i] - a[k][i] for i in range(3)) for k in range(3)]
    nx = e[0][1] * e[1][2] - e[0][2] * e[1][1]
    ny = e[0][2] * e[1][0] - e[0][0] * e[1][2]
    nz = e[0][0] * e[1][1] - e[0][1] * e[1][0]
    if abs(nx * a[0][0] + ny * a[0][1] + nz * a[0][2]) > half * (abs(nx) + abs(ny) + abs(nz)):
        return False
    for ex, ey, ez in e:
        for ux, uy, uz in ((0, -ez, ey), (ez, 0, -ex), (-ey, ex, 0)):
            p = [ux * v[0] + uy * v[1] + uz * v[2] for v in a]
            r = half * (abs(ux) + abs(uy) + abs(uz))
            if min(p) > r or max(p) < -r:
                return False
    return True


def exact_segment(P0, P1, cx, cy, cz, half):
    """Closed segment P0 P1 (ints; P0 == P1: a point) against the closed box, by exact slabs:
    the parameter interval [t0, t1] of each axis as fractions compared by cross-multiplying."""
    lo_n, lo_d, hi_n, hi_d = 0, 1, 1, 1            # t in [0, 1]
    for p0, p1, c in zip(P0, P1, (cx, cy, cz)):
        d = p1 - p0
        if d == 0:
            if abs(p0 - c) > half:
                return False
            continue
        n0, n1 = (c - half) - p0, (c + half) - p0  # t d in [n0, n1]
        if d < 0:
            n0, n1, d = -n1, -n0, -d
        if n0 * lo_d > lo_n * d:
            lo_n, lo_d = n0, d
        if n1 * hi_d < hi_n * d:
            hi_n, hi_d = n1, d
    return lo_n * hi_d <= hi_n * lo_d


def _shape(Q):
    """'point', 'segment' (-> its two end points) or 'triangle' of integer vertices."""
    e1 = [Q[1][i] - Q[0][i] for i in range(3)]
    e2 = [Q[2][i] - Q[0][i] for i in range(3)]
    cr = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
    if any(cr):
        return "triangle", None
    # collinear: the extreme pair along the longest difference
    pts = sorted(Q, key=lambda v: tuple(v))
    return ("point" if pts[0] == pts[2] else "segment"), (pts[0], pts[2])


def exact_sets(qt, n, delta=None):
    """-> (inner, outer): flat voxel indices (sets) whose closed box of half-size 0.5 - DELTA /
    0.5 + DELTA overlaps the binary32 triangle qt in exact arithmetic (candidate box +- 1)."""
    Q = _ints(qt)
    d = delta_for(qt, n) if delta is None else delta
    kind, ends = _shape(Q)
    lo, hi = cand_box(qt, n)
    inner, outer = set(), set()
    for z in range(lo[2], hi[2] + 1):
        for y in range(lo[1], hi[1] + 1):
            for x in range(lo[0], hi[0] + 1):
                c = (x * S + S // 2, y * S + S // 2, z * S + S // 2)
                for half, dst in ((S // 2 + d, outer), (S // 2 - d, inner)):
                    hit = exact_overlap(Q, *c, half) if kind == "triangle" else exact_segment(*ends, *c, half)
                    if not hit:
                        break               # not in the outer set: not in the inner one either
                    dst.add(x + n * (y + n * z))
    return inner, outer


def band_counts(mesh, skip=()):
    """Per-voxel sums of the inner and outer sets over the mesh's finite triangles ->
    (inner [n^3], outer [n^3]) uint32: every implementation's counts must lie between them."""
    n = mesh.n
    lo, hi = np.zeros(n ** 3, np.uint32), np.zeros(n ** 3, np.uint32)
    q = q_of(mesh.verts, mesh.g0, mesh.E, n).reshape(-1, 3, 3)
    for t, qt in enumerate(q):
        if not np.isfinite(qt).all() or (mesh.names and mesh.names[t] in skip):
            continue
        i, o = exact_sets(qt, n)
        lo[list(i)] += 1
        hi[list(o)] += 1
    return lo, hi


def seeded_triangles(n, count=400, seed=2024):
    """Adversarial triangles in voxel units on a 2^-12 grid: general position, near-lattice
    (vertices within a few 2^-12 of integer points), slivers and tiny ones, a quarter each."""
    rng = np.random.default_rng(seed + n)
    g = 2.0 ** -12
    out = []
    for i in range(count):
        k = i % 4
        if k == 0:
            tri = rng.uniform(-1, n + 1, (3, 3))
        elif k == 1:
            tri = rng.integers(0, n + 1, (3, 3)) + rng.integers(-2, 3, (3, 3)) * g
        elif k == 2:
            a, b = rng.uniform(0, n, 3), rng.uniform(0, n, 3)
            tri = np.stack([a, b, (a + b) / 2 + rng.integers(-3, 4, 3) * g])
        else:
            a = rng.uniform(0, n, 3) if i % 8 == 3 else rng.integers(0, n + 1, 3).astype(np.float64)
            tri = a + rng.integers(-3, 4, (3, 3)) * g
        out.append(np.round(tri / g) * g)
    return np.asarray(out, np.float64)


def seeded_mesh(n, placement="exact", count=400):
    g0, E = grid_of(n, placement)
    q = seeded_triangles(n, count)
    verts = _world_fast(q.reshape(-1, 3), g0, E, n)
    t = len(q)
    return Mesh(verts, np.arange(3 * t, dtype=np.uint32), (np.arange(t) % 4).astype(np.uint32),
                np.array([_kd_for(i) + (1.0,) for i in range(4)], F), [f"seed{i}" for i in range(t)], None,
                n, g0, E, placement)


# ---------------------------------------------------------------------------
def describe_diff(got, ref, mesh):
    """got / ref: (sums [n^3, 6], counts [n^3]).  Names the first differing voxels and the
    entries whose candidate boxes contain them."""
    n = mesh.n
    d = (np.asarray(got[1]).astype(np.int64) != np.asarray(ref[1]).astype(np.int64)) | \
        (np.asarray(got[0]) != np.asarray(ref[0])).any(-1)
    vs = np.flatnonzero(d)
    q = q_of(mesh.verts, mesh.g0, mesh.E, n).reshape(-1, 3, 3)
    msg = []
    for v in vs[:8]:
        x, y, z = int(v % n), int(v // n % n), int(v // (n * n))
        near = []
        for t, qt in enumerate(q):
            if not np.isfinite(qt).all():
                continue
            lo, hi = cand_box(qt, n, pad=0)
            if (lo <= (x, y, z)).all() and ((x, y, z) <= hi).all():
                near.append(mesh.names[t] if mesh.names else f"tri{t}")
        msg.append(f"({x},{y},{z}) count {int(got[1][v])} vs {int(ref[1][v])} near {near[:6]}")
    return f"{vs.size} voxels differ: " + "; ".join(msg)
