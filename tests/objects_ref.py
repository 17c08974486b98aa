"""The object set's reference (TEST INFRASTRUCTURE): the transform rule in numpy and a
composition of oracle calls, no new GI arithmetic.  include/vct_spec.h "dynamic objects": after
any sequence of vct_objects_define / vct_objects_update calls the context is the context after
vct_voxelize(union(S, T(O_0, P_0), T(O_1, P_1), ...)), so the reference of every comparison is
the oracle (or a fresh context) run on `posed_union`.

Also the catalogue of objects the GPU tests use: tests/dynamic_ref.py's shapes, moved to object
space (centred on their bounding box) with the pose that puts them back.  tests/test_objects.py
asserts what each name promises against the oracle's coverage counts:
  air       a 12-triangle box in empty space
  floor     a box standing on the Cornell floor: voxels S occupies and voxels S leaves empty
  tet       a tetrahedron beside `floor`, cutting into the short box
  over      a box overlapping `tet`
  straddle  a box through the right wall and the grid's +x face
  outside   a box that lands wholly outside the grid: no candidates
  none      an object with no triangles
"""
from __future__ import annotations

import numpy as np

import dynamic_ref as D

F = np.float32
GRIDS = (16, 32)
# the set's one material table; an object's triangles name a row
KD = np.array([[0.2, 0.3, 0.9, 1.0], [0.9, 0.6, 0.1, 1.0], [0.5, 0.1, 0.7, 1.0]], F)
NAMES = ("air", "floor", "tet", "over", "straddle", "outside", "none")
_ROW = {"tet": 1, "over": 2}

POSE = np.dtype([("m", np.float32, 16), ("visible", np.uint32), ("reserved", np.uint32, 3)])


def transform(verts, m):
    """The transform rule on the first three floats of every vertex record: float32, one rounding
    per operation, in the rule's order; m = 16 floats, column-major."""
    v = np.array(verts, F, copy=True)
    m = np.asarray(m, F).reshape(16)
    x, y, z = v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            v[:, r] = ((m[r] * x + m[4 + r] * y).astype(F) + (m[8 + r] * z).astype(F)).astype(F) + m[12 + r]
    return v


def pose(placement=None, visible=True):
    """vct.objects.pose, kept apart so that the reference does not lean on the code under test."""
    p = np.zeros((), POSE)
    m = np.eye(4, dtype=F)
    if placement is not None:
        a = np.asarray(placement, F)
        if a.shape == (3,):
            m[:3, 3] = a
        else:
            m = a.reshape(4, 4)
    p["m"] = m.T.reshape(16)
    p["visible"] = 1 if visible else 0
    return p


def pose_array(records):
    out = np.zeros(len(records), POSE)
    for j, r in enumerate(records):
        out[j] = r
    return out


def posed(objects, poses, kd=KD):
    """The objects under their poses as one world-space mesh (verts, idx, tri_mat, kd), in
    definition order; a hidden object's vertices are NaN.  kd None: albedo 1."""
    nf = max([np.asarray(o[0]).shape[1] for o in objects] + [3])
    vs, is_, ms, base = [], [], [], 0
    for o, p in zip(objects, poses):
        v = np.zeros((np.asarray(o[0]).shape[0], nf), F)
        v[:, :np.asarray(o[0]).shape[1]] = o[0]
        v = transform(v, p["m"])
        if not int(p["visible"]):
            v[:, :3] = np.nan
        vs.append(v)
        is_.append(np.asarray(o[1], np.uint32) + np.uint32(base))
        t = np.asarray(o[1]).size // 3
        ms.append(np.asarray(o[2], np.uint32) if len(o) > 2 and o[2] is not None and kd is not None else np.zeros(t, np.uint32))
        base += v.shape[0]
    table = np.asarray(kd, F).reshape(-1, 4) if kd is not None else np.ones((1, 4), F)
    return (np.concatenate(vs) if vs else np.zeros((0, nf), F), np.concatenate(is_) if is_ else np.zeros(0, np.uint32),
            np.concatenate(ms) if ms else np.zeros(0, np.uint32), table)


def posed_union(static, objects, poses, kd=KD):
    """union(S, T(O_0, P_0), T(O_1, P_1), ...): dynamic_ref.union extended to several meshes."""
    layer = posed(objects, poses, kd)
    sv = np.asarray(static[0], F)
    lv = np.zeros((layer[0].shape[0], sv.shape[1]), F)
    k = min(sv.shape[1], layer[0].shape[1])
    lv[:, :k] = layer[0][:, :k]
    return D.union(static, (lv, layer[1], layer[2], layer[3]))


def _centred(mesh, row):
    v, i, _, _ = mesh
    v = np.array(v, F, copy=True)
    if v.shape[0] == 0:
        return (v, i, np.zeros(0, np.uint32)), pose()
    c = ((v[:, :3].min(0) + v[:, :3].max(0)) * F(0.5)).astype(F)
    v[:, :3] -= c
    return (v, np.asarray(i, np.uint32), np.full(i.size // 3, row, np.uint32)), pose(c)


def catalogue():
    """name -> (object-space mesh (verts, idx, tri_material), the pose that places it)."""
    L = D.layers()
    return {k: _centred(L["empty" if k == "none" else k], _ROW.get(k, 0)) for k in NAMES}


def box_object(half=0.13, row=0):
    """dynamic_ref.path's box, centred on the origin."""
    v, i, _, _ = D.box((-half,) * 3, (half,) * 3)
    return np.asarray(v, F), np.asarray(i, np.uint32), np.full(i.size // 3, row, np.uint32)


def coverage(n, objects, poses, kd=KD):
    """The oracle's (sums, counts) of the posed objects voxelized alone."""
    return D.coverage(n, posed(objects, poses, kd))


def touched(n, old, new):
    """Voxels with a non-zero oracle count for the moved objects' old or new triangles voxelized
    alone; old, new: world-space meshes (as `posed` returns them)."""
    return int(((D.coverage(n, old)[1] > 0) | (D.coverage(n, new)[1] > 0)).sum())
