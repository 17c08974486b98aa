"""Hostile receivers for the shadow walk (TEST INFRASTRUCTURE): a deterministic catalogue of
G-buffer pixels that are legal at the ABI (include/vct.h: any pos4.w != 0 is a valid pixel) and
whose cone origin q = (P - g0) * inv_h + N is NaN, too large for an int, or exactly on the
edges of the "shadow-walk receiver rule" of include/vct_spec.h, written behind the pixels of a
clean frame, with the lights and the two voxel fields they are tested on.

The rule defines V for every entry, and `expected_v` writes it down by hand: 1 for a q that
fails 0 <= q_a < n (a NaN fails), and for a q inside the grid what the walk from the cell
floor(q) gives (tests/light_inputs.py walk_count, which knows nothing of the rule: every such q
fits an int).  `composite_expect` is the plain numpy restatement of the composite around it.

The grid is g0 = (0, 0, 0), E = n = 16, so inv_h = 1 and q_a = P_a + N_a in one rounding: a q of
-0.0 or of a denormal can only be reached where g0_a is +0 ((-0.0) - (+0.0) is the one
subtraction that gives -0.0).  The exact-origin construction of tests/trace_inputs.py
(`_exact_origin`: P one voxel outside, N_a = target - v by Sterbenz) is used as it is.

Entries (`catalogue()`; every entry is a (P, N) record, albedo / diffuse / specular are
ordinary finite numbers; NORMALS are the six axis vectors and +-(0.48, 0.6, 0.64)):
  nan_axis   NaN in q.x, .y, .z, .xy, .xz, .yz, .xyz, once through P (every normal of NORMALS)
             and once as (+inf) + (-inf) across P and N (the other components of N from NORMALS;
             `planes_only`: N.l is +inf or NaN, so the composite's colour would be inf and its
             tone curve NaN -- these go to the visibility planes only, where V = 1 is defined)
  big        per axis +-1e30 and +-inf in P, q = +-2^31 exactly, prev(2^31), -2^31 - 256, and the
             1e3 E positions of trace_inputs (n + 1e3 E, -1e3 E)
  edge       per axis q exactly +0, -0.0, prev(0) as a denormal (-1e-45) and as a normal
             (-2^-126), n, prev(n) and next(n): once through N (P at its exact origin, N the axis
             normal or, for the three tiny values, an axis normal with the tiny component added)
             and once through P (N_a = 0, every normal of NORMALS without a component on a)
  w          pos4.w = -0.0 (background), NaN, 2 and 1e-45 on a pixel with P.x = NaN

Lights (`directions()`): +-x, +-y, +-z; (0.6, 0.8, 0) and its cyclic permutations, both signs;
one component 1e-40 (td = +inf, the K2 input rule; light_inputs' construction), per axis, both
signs of the other two; one generic direction and its opposite.  `light_list()`: the same as
directional lights plus one point and one spot light.

Voxel fields, n = 16 (`field(name)`): "slabs": every cell with x = 0, y = 0 or z = 0 is
occupied, plus the floating box and the tilted quad of light_inputs' generic field; "open": the
same without the slabs (CPU only: see tests/test_receiver_inputs_gpu.py).  On "slabs" a NaN
component converted to cell 0 of its axis lands in an occupied cell: arithmetic without the
rule gives 0 there, a wrong value in the walk's first cell, never a walk that does not end.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import light_inputs as LI
from trace_inputs import _exact_origin

F = np.float32
N_GRID = 16
G0, E = (0.0, 0.0, 0.0), 16.0
W = 64
NAN, INF = F(np.nan), F(np.inf)
BASE = np.array([8.3, 11.4, 9.6], F)          # a q inside the grid, in an empty cell of both fields
TILT = np.array([0.48, 0.6, 0.64], F)
NORMALS = [np.array(v, F) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))] + [TILT, -TILT]
ALBEDO = np.array([0.75, 0.5, 0.625, 0.1], F)
FAMILIES = ("nan_axis", "big", "edge", "w")

# expect: "one" (V = 1 whenever the pixel is walked), "floor" (the walk from floor(q)),
# "background" (pos4.w == 0)
# q: None, or (axis, the exact q on that axis) for the tests to hold the construction against
Entry = namedtuple("Entry", "name family P N expect planes_only q")
Frame = namedtuple("Frame", "pos nrm alb D S entry names n_clean")


def _axes(mask):
    return [a for a in range(3) if mask >> a & 1]


def catalogue():
    out = []

    def add(name, family, P, N, expect, w=1.0, planes_only=False, q=None):
        out.append(Entry(name, family, np.array([P[0], P[1], P[2], w], F), np.array(N, F), expect, planes_only, q))

    # ---- nan_axis ---------------------------------------------------------------------------
    for mask in range(1, 8):
        tag = "".join("xyz"[a] for a in _axes(mask))
        for k, nv in enumerate(NORMALS):
            P = BASE.copy()
            P[_axes(mask)] = NAN
            add(f"nan_{tag}_P_n{k}", "nan_axis", P, nv, "one")
            P, N = BASE.copy(), nv.copy()
            P[_axes(mask)] = INF
            N[_axes(mask)] = -INF
            add(f"nan_{tag}_infinf_n{k}", "nan_axis", P, N, "one", planes_only=True)
    # ---- big --------------------------------------------------------------------------------
    two31 = F(2.0 ** 31)
    big = (("+1e30", F(1e30)), ("-1e30", F(-1e30)), ("+inf", INF), ("-inf", -INF), ("+2^31", two31), ("-2^31", -two31),
           ("prev2^31", np.nextafter(two31, F(0))), ("-2^31-256", F(-2.0 ** 31 - 256.0)),
           ("far+", F(F(N_GRID) + F(1e3) * F(E))), ("far-", F(-F(1e3) * F(E))))
    for a in range(3):
        for vname, v in big:
            for k, nv in enumerate(NORMALS):
                P = BASE.copy()
                P[a] = v
                add(f"big_{'xyz'[a]}{vname}_n{k}", "big", P, nv, "one")
    # ---- edge -------------------------------------------------------------------------------
    n = F(N_GRID)
    tiny = (("-0", F(-0.0)), ("prev0_denormal", F(-1e-45)), ("prev0_normal", F(-2.0 ** -126)))
    edges = (("+0", F(0.0), 1.0), ("n", n, -1.0), ("prevn", np.nextafter(n, F(0)), -1.0), ("nextn", np.nextafter(n, INF), -1.0))
    for a in range(3):
        b = (a + 1) % 3
        for vname, target, na in edges:                       # through N: the exact-origin construction
            p, nc = _exact_origin(G0[a], E, N_GRID, float(target), na)
            P, N = BASE.copy(), np.zeros(3, F)
            P[a], N[a] = p, nc
            add(f"edge_{'xyz'[a]}{vname}_N", "edge", P, N, "floor" if 0 <= target < n else "one", q=(a, target))
        for vname, target in tiny:                            # through N: P_a = -0.0, N_a = target
            for sb in (1.0, -1.0):
                P, N = BASE.copy(), np.zeros(3, F)
                P[a], N[a], N[b] = F(-0.0), target, sb
                add(f"edge_{'xyz'[a]}{vname}_N{'+' if sb > 0 else '-'}", "edge", P, N, "floor" if vname == "-0" else "one",
                    q=(a, target))
        for vname, target in tuple((v, t) for v, t, _ in edges) + tiny:   # through P: N_a = 0
            for k, nv in enumerate(NORMALS):
                if nv[a] != 0:
                    continue
                P, N = BASE.copy(), nv.copy()
                P[a] = target
                N[a] = F(-0.0) if np.signbit(target) else F(0.0)       # (-0.0) + (+0.0) would be +0.0
                add(f"edge_{'xyz'[a]}{vname}_P_n{k}", "edge", P, N, "floor" if 0 <= target < n else "one", q=(a, target))
    # ---- w ----------------------------------------------------------------------------------
    for vname, w, expect in (("negzero", F(-0.0), "background"), ("nan", NAN, "one"), ("two", F(2), "one"),
                             ("denormal", F(1e-45), "one")):
        for k, nv in enumerate(NORMALS):
            P = BASE.copy()
            P[0] = NAN
            add(f"w_{vname}_n{k}", "w", P, nv, expect, w=w)
    names = [e.name for e in out]
    assert len(set(names)) == len(names)
    return out


def origin(P, N):
    """q = (P - g0) * inv_h + N in the kernels' binary32 order; [R, 3]."""
    with np.errstate(all="ignore"):
        return ((np.asarray(P, F)[..., :3] - np.asarray(G0, F)) * (F(N_GRID) / F(E)) + np.asarray(N, F)[..., :3]).astype(F)


# ---------------------------------------------------------------------------
# lights
# ---------------------------------------------------------------------------
Direction = namedtuple("Direction", "name d")
COLOUR = (1.0, 0.5, 0.25)


def directions():
    out = []
    for a in range(3):
        for s in (1.0, -1.0):
            d = [0.0, 0.0, 0.0]
            d[a] = s
            out.append(Direction(f"axis_{'xyz'[a]}{'+' if s > 0 else '-'}", np.array(d, F)))
    for a in range(3):                                     # one component exactly 0
        for s in (1.0, -1.0):
            d = [0.0, 0.0, 0.0]
            d[a], d[(a + 1) % 3] = s * 0.6, s * 0.8
            out.append(Direction(f"planar_{'xyz'[(a + 2) % 3]}0_{'+' if s > 0 else '-'}", np.array(d, F)))
    for a in range(3):                                     # td = +inf on axis a (K2 input rule)
        for o in (1.0, -1.0):
            d = [0.0, 0.0, 0.0]
            d[a], d[(a + 1) % 3], d[(a + 2) % 3] = 1e-40, o * 0.8, o * 0.907
            out.append(Direction(f"tiny_{'xyz'[a]}1e-40_{'pos' if o > 0 else 'neg'}", np.array(d, F)))
    out.append(Direction("generic+", np.array((0.3, 1.0, 0.2), F)))
    out.append(Direction("generic-", np.array((-0.35, -0.7, -0.61), F)))
    assert all(LI.direction_status(e.d) == LI.VCT_OK for e in out)
    with np.errstate(all="ignore"):
        assert all(np.isinf(F(1.0) / np.abs(LI.normalised(e.d))).sum() == (0 if e.name.startswith("generic") else
                                                                           2 if e.name.startswith("axis") else 1) for e in out)
    return out


def light_list():
    """The directions as directional lights, then a point and a spot light inside the grid."""
    import vct
    out = [vct.directional_light([float(v) for v in e.d], COLOUR) for e in directions()]
    out.append(vct.point_light((8.2, 13.3, 7.9), (3.0, 2.0, 1.0), 30.0))
    out.append(vct.spot_light((7.5, 15.0, 9.5), (0.1, -1.0, 0.05), (2.0, 2.0, 3.0), 40.0, cos_inner=0.9, cos_outer=0.2))
    return out


# ---------------------------------------------------------------------------
# voxel fields
# ---------------------------------------------------------------------------
_fields = {}


def field(name):
    """-> light_inputs.Field on the grid (G0, E, N_GRID)."""
    if name not in _fields:
        b = LI._Builder(N_GRID, exact=True)
        s = N_GRID / 16.0
        if name == "slabs":
            m = float(N_GRID)
            b.quad((0.5, 0, 0), (0, m, 0), (0, 0, m), 0)             # cells x = 0, normal +x
            b.quad((0, 0.5, 0), (0, 0, m), (m, 0, 0), 2)             # cells y = 0, normal +y
            b.quad((0, 0, 0.5), (m, 0, 0), (0, m, 0), 3)             # cells z = 0, normal +z
        else:
            assert name == "open", name
        b.box((5.3 * s, 6.2 * s, 4.4 * s), (9.6 * s, 9.7 * s, 8.3 * s), 1)                  # light_inputs._generic's
        b.quad((2.1 * s, 3.0 * s, 11.0 * s), (9.0 * s, 6.0 * s, 1.5 * s), (-1.0 * s, 5.0 * s, 3.0 * s), 3)
        _fields[name] = b.field(name, "receiver")
        assert _fields[name].g0 == G0 and _fields[name].E == E
    return _fields[name]


def check_field(name, ao):
    """What the field names promise, on the oracle's K1 output."""
    occ = np.asarray(ao)[..., 3] != 0
    face = occ[:, :, 0].all() and occ[:, 0, :].all() and occ[0, :, :].all()
    assert face == (name == "slabs"), name
    if name == "open":
        assert not occ[:, :, 0].any() and not occ[0, :, :].any(), name
    assert occ[1:, 1:, 1:].sum() > 100 and not occ[int(BASE[2]), int(BASE[1]), int(BASE[0])]
    q = BASE.astype(np.int64)
    assert not occ[q[2], q[1] + 1, q[0]] and not occ[q[2], q[1] - 1, q[0]]


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
def build(f, ao, nm, entries=None, composite=True, seed=5):
    """The field's clean frame (light_inputs.gbuffer_of: one pixel per occupied voxel, its albedo
    made positive) padded to whole rows, then the entries, one pixel each.  composite: the
    planes_only entries are left out.  -> Frame (D, S: random finite planes)."""
    cat = catalogue() if entries is None else entries
    sel = [i for i, e in enumerate(cat) if not (composite and e.planes_only)]
    pos, nrm, alb = (a.reshape(-1, 4) for a in LI.gbuffer_of(f, ao, nm, W))
    with np.errstate(all="ignore"):
        alb = (np.abs(alb) + F(0.25)).astype(F)
    n_clean = pos.shape[0]
    rows = (len(sel) + W - 1) // W
    P, N, A = (np.zeros((rows * W, 4), F) for _ in range(3))
    entry = np.full(n_clean + rows * W, -1, np.int32)
    for k, i in enumerate(sel):
        P[k], N[k, :3], A[k] = cat[i].P, cat[i].N, ALBEDO
        entry[n_clean + k] = i
    pos, nrm, alb = np.concatenate([pos, P]), np.concatenate([nrm, N]), np.concatenate([alb, A])
    h = pos.shape[0] // W
    assert h <= 48
    rng = np.random.default_rng(seed)
    D = rng.random((h, W, 4)).astype(F)
    S = (rng.random((h, W, 4)) * 0.2).astype(F)
    sh = (h, W, 4)
    return Frame(pos.reshape(sh), nrm.reshape(sh), alb.reshape(sh), D, S, entry.reshape(h, W), [e.name for e in cat],
                 n_clean)


def small_frames(cat=None):
    """(13 x 7: every fifth entry, 91 pixels of the nan_axis, big and edge families; 8 x 8: a block of nan_xyz pixels with
    N = +y, which no light with l.y <= 0 needs) -> [(name, pos, nrm, entries)], for the visibility
    planes."""
    cat = catalogue() if cat is None else cat
    part = cat[::5][:91]
    pos = np.array([e.P for e in part], F).reshape(7, 13, 4)
    nrm = np.zeros((7, 13, 4), F)
    nrm[..., :3] = np.array([e.N for e in part], F).reshape(7, 13, 3)
    e = next(e for e in cat if e.name == "nan_xyz_P_n2")
    bp, bn = np.tile(e.P, (8, 8, 1)).astype(F), np.zeros((8, 8, 4), F)
    bn[..., :3] = e.N
    return [("partial 13x7", pos, nrm, part), ("NaN block 8x8", bp, bn, [e] * 64)]


# ---------------------------------------------------------------------------
# the hand-written result
# ---------------------------------------------------------------------------
def old_start_test(q, n):
    """A.3's start test on the converted cell: floor(q) in [0, n) on every axis, for q an int
    holds (numpy int64 here; the caller passes only such q).  -> [R] bool"""
    v = np.floor(np.asarray(q, F)).astype(np.int64)
    return np.all((v >= 0) & (v < n), axis=-1)


def unguarded_device_walk(occ, q, l, cap):
    """A model of dda_visibility as gfx950 runs it WITHOUT the receiver rule, for one receiver: the
    float -> int conversion turns NaN into 0 and saturates the rest, a NaN tm loses every <=.
    -> (V, cells tested); V is None when the walk has not ended after `cap` cells.  Only the CPU
    tests use it, to show what the catalogue's fields do to a kernel that lacks the guard."""
    n = occ.shape[0]
    q, l = np.asarray(q, F), np.asarray(l, F)
    with np.errstate(all="ignore"):
        fl = np.floor(q)
        v = [0 if np.isnan(x) else int(min(max(float(x), -2.0 ** 31), 2.0 ** 31 - 1)) for x in fl]
        if any(c < 0 or c >= n for c in v):
            return F(1.0), 0
        s = [1 if x > 0 else (-1 if x < 0 else 0) for x in l]
        td = [F(1.0) / np.abs(x) if sa else F(np.inf) for x, sa in zip(l, s)]
        s = [0 if np.isinf(t) else sa for t, sa in zip(td, s)]
        tm = [(F(c + 1) - x) * t if sa > 0 else ((x - F(c)) * t if sa < 0 else F(np.inf))
              for c, x, t, sa in zip(v, q, td, s)]
        for cells in range(1, cap + 1):
            if occ[v[2], v[1], v[0]]:
                return F(0.0), cells
            a = 0 if (tm[0] <= tm[1] and tm[0] <= tm[2]) else (1 if tm[1] <= tm[2] else 2)
            v[a] += s[a]
            if v[a] < 0 or v[a] >= n:
                return F(1.0), cells
            tm[a] = tm[a] + td[a]
    return None, cap


def ndl_of(N, d):
    """dot3(N, l) for the raw direction d, float32, l normalised as the host does."""
    l = LI.normalised(d)
    N = np.asarray(N, F)
    with np.errstate(all="ignore"):
        return ((N[..., 0] * l[0] + N[..., 1] * l[1]) + N[..., 2] * l[2]).astype(F)


def expected_v(frame, cat, occ, d):
    """V per pixel for the directional light d, by hand: NaN where the pixel is background or
    skips the light (ndl > 0 fails); 1 for an entry that expects "one"; the walk from floor(q)
    for the rest (clean pixels included; their q fits an int).  -> [h, w] float32"""
    h, w = frame.entry.shape
    pos, nrm = frame.pos.reshape(-1, 4), frame.nrm.reshape(-1, 4)
    ent = frame.entry.ravel()
    V = np.full(h * w, NAN, F)
    ndl = ndl_of(nrm, d)
    with np.errstate(all="ignore"):
        walked = (pos[:, 3] != 0) & (ndl > 0)
    one = np.array([i >= 0 and cat[i].expect == "one" for i in ent])
    V[walked & one] = 1.0
    k = np.flatnonzero(walked & ~one)
    q = origin(pos[k], nrm[k])
    assert np.isfinite(q).all() and np.abs(q).max() < 1e6
    V[k] = LI.walk_count(occ, q, LI.normalised(d))[0]
    return V.reshape(h, w)


def composite_expect(frame, d, colour, V):
    """The composite of include/vct_spec.h around a given V, plainly: final = (((A * c) * ndl) * V
    + A * D) + S at a walked pixel, (A * D) + S + 0 at a skipped one, the clear colour with
    alpha 0 at a background pixel.  -> [h, w, 4] float32"""
    h, w = frame.entry.shape
    out = np.empty((h, w, 4), F)
    out[...] = np.array([0.2, 0.3, 0.3, 0.0], F)
    c = np.asarray(colour, F)
    ndl = ndl_of(frame.nrm, d)
    A, D, S = frame.alb[..., :3], frame.D[..., :3], frame.S[..., :3]
    with np.errstate(all="ignore"):
        valid = frame.pos[..., 3] != 0
        walked = valid & (ndl > 0)
        direct = np.zeros((h, w, 3), F)
        direct[walked] = (((A * c[None, None, :]) * ndl[..., None]) * V[..., None])[walked]
        fin = (direct + A * D) + S
    out[valid, :3] = fin[valid]
    out[valid, 3] = 1.0
    return out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def describe(frame, diff):
    ys, xs = np.nonzero(diff)
    return [(int(y), int(x), frame.names[frame.entry[y, x]] if frame.entry[y, x] >= 0 else "clean")
            for y, x in zip(ys[:12], xs[:12])]
