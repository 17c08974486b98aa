"""The dynamic layer's reference (TEST INFRASTRUCTURE): a composition of oracle calls, no new
arithmetic.  include/vct_spec.h "dynamic layer": after vct_voxelize_dynamic(D) on a static
mesh S the context is the context after vct_voxelize(union(S, D)), so the reference of every
comparison is the oracle (or a fresh context) run on `union`.

Also the catalogue of layers the GPU tests use, chosen on the CPU (tests/test_dynamic.py
asserts what each name promises against the oracle's coverage counts):
  air       a 12-triangle box in empty space: every voxel it hits is empty in S
  floor     a box standing on the Cornell floor: hits voxels S occupies and voxels S leaves empty
  tet       a tetrahedron beside `floor` (the solids are disjoint, 0.02 apart, so they share
            voxels), cutting into the short box
  over      a box overlapping `tet`
  straddle  a box through the right wall and the grid's +x face
  outside   a box wholly outside the grid: no candidates
  empty     no triangles
REPLACE is the sequence floor -> tet -> over -> none; PATH the 24 positions of the moving box.
"""
from __future__ import annotations

import numpy as np

F = np.float32
GRIDS = (16, 32)


def union(static, layer):
    """static, layer: (verts (V, F) float32, idx (3T,) uint32, tri_mat (T,) uint32, kd (M, 4)
    float32) -> the concatenated mesh: the layer's indices and material ids offset."""
    sv, si, sm, sk = static
    lv, li, lm, lk = layer
    sv, lv = np.asarray(sv, F), np.asarray(lv, F)
    if lv.shape[0] == 0:
        lv = lv.reshape(0, sv.shape[1])
    assert sv.shape[1] == lv.shape[1]
    return (np.concatenate([sv, lv]).astype(F),
            np.concatenate([np.asarray(si, np.uint32), np.asarray(li, np.uint32) + np.uint32(sv.shape[0])]),
            np.concatenate([np.asarray(sm, np.uint32), np.asarray(lm, np.uint32) + np.uint32(len(sk))]),
            np.concatenate([np.asarray(sk, F).reshape(-1, 4), np.asarray(lk, F).reshape(-1, 4)]))


def static_arrays():
    from vct import scenes
    return scenes.cornell().arrays()


def box(lo, hi, kd=(0.2, 0.3, 0.9)):
    from vct import scenes
    s = scenes.Scene("box")
    s.box(tuple(lo), tuple(hi), s.material(kd))
    return s.arrays()


def tet(p0, p1, p2, p3, kd=(0.9, 0.6, 0.1)):
    from vct import scenes
    s = scenes.Scene("tet")
    m = s.material(kd)
    for a, b, c in ((p0, p1, p2), (p0, p1, p3), (p1, p2, p3), (p2, p0, p3)):
        s.tri(a, b, c, m)
    return s.arrays()


def empty():
    from vct import VERTEX_FLOATS
    return (np.zeros((0, VERTEX_FLOATS), F), np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.ones((1, 4), F))


def layers():
    return {
        "air": box((-0.3, 0.3, 0.3), (0.0, 0.55, 0.6)),
        "floor": box((-0.2, -1.0, 0.5), (0.1, -0.7, 0.8)),
        "tet": tet((0.12, -0.98, 0.55), (0.4, -0.98, 0.55), (0.26, -0.98, 0.85), (0.26, -0.45, 0.7)),
        "over": box((0.2, -0.9, 0.6), (0.45, -0.65, 0.9), kd=(0.5, 0.1, 0.7)),
        "straddle": box((0.9, -0.2, -0.2), (1.4, 0.1, 0.1)),
        "outside": box((2.0, 2.0, 2.0), (2.3, 2.3, 2.3)),
        "empty": empty(),
    }


ADD = ("air", "floor", "tet", "straddle", "outside", "empty")
REPLACE = ("floor", "tet", "over", "empty")


def path(steps=24):
    """The moving box: a loop of period 8 (three turns in 24 steps), so it re-enters the voxels
    it left; every position differs from the one before."""
    out = []
    for k in range(steps):
        a = 2.0 * np.pi * (k % 8) / 8.0
        c = np.array([-0.1 + 0.35 * np.cos(a), -0.5 + 0.3 * np.sin(a), 0.55 + 0.1 * np.sin(2 * a)])
        out.append(box(c - 0.13, c + 0.13))
    return out


_cache = {}


def coverage(n, mesh):
    """The oracle's (sums [n^3, 6], counts [n^3]) of a mesh on scenes.grid_for_unit_box(n)."""
    from oracle import oracle as O
    from vct import scenes
    g0, E = scenes.grid_for_unit_box(n)
    return O.voxelize(n, g0, E, *mesh)


def static_coverage(n):
    if ("S", n) not in _cache:
        _cache[("S", n)] = coverage(n, static_arrays())
    return _cache[("S", n)]


def layer_coverage(n, name):
    if (name, n) not in _cache:
        _cache[(name, n)] = coverage(n, layers()[name])
    return _cache[(name, n)]


def reference(n, layer, light=None):
    """oracle.pipeline of union(Cornell, layer) on the unit-box grid."""
    from oracle import oracle as O
    from vct import scenes
    g0, E = scenes.grid_for_unit_box(n)
    return O.pipeline(n, g0, E, *union(static_arrays(), layer), light or scenes.LIGHT_DIR, scenes.LIGHT_COLOR)
