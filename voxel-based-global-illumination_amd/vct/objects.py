"""Dynamic objects (include/vct_objects.h): poses and a small keeper of a set.

    from vct import objects
    s = objects.ObjectSet(ctx, [(verts, idx, tri_material), ...], kd4)     # every object hidden
    s.move([2], [objects.pose((0.1, 0.0, 0.3))])                           # show object 2 there
    s.move([0, 2], [objects.pose(matrix4x4), objects.pose(visible=False)])

A pose is one vct_object_pose record: a column-major 4x4 (only the affine part is read) and the
visible word.  include/vct_spec.h "dynamic objects" has the transform rule.
"""
from __future__ import annotations

import numpy as np

POSE = np.dtype([("m", np.float32, 16), ("visible", np.uint32), ("reserved", np.uint32, 3)])
assert POSE.itemsize == 80


def pose(placement=None, visible: bool = True) -> np.ndarray:
    """One POSE record.  placement: None (identity), a translation (3 values), or a 4x4 matrix
    in the mathematical layout (row r, column c: x' = M[0, 0] x + M[0, 1] y + M[0, 2] z + M[0, 3]),
    which is stored column-major as the C ABI reads it."""
    p = np.zeros((), POSE)
    m = np.eye(4, dtype=np.float32)
    if placement is not None:
        a = np.asarray(placement, dtype=np.float32)
        if a.shape == (3,):
            m[:3, 3] = a
        elif a.shape == (4, 4):
            m = a
        else:
            raise ValueError(f"pose: a translation (3,) or a matrix (4, 4), got {a.shape}")
    p["m"] = m.T.reshape(16)
    p["visible"] = 1 if visible else 0
    return p


def poses(records) -> np.ndarray:
    """A sequence of POSE records as one contiguous array."""
    out = np.zeros(len(records), POSE)
    for j, r in enumerate(records):
        out[j] = r
    return out


class ObjectSet:
    """Defines the set on `ctx` and remembers the last pose of every object."""

    def __init__(self, ctx, meshes, kd4=None):
        self.ctx = ctx
        self.meshes = list(meshes)
        ctx.objects_define(self.meshes, kd4)
        self.poses = poses([pose(visible=False)] * len(self.meshes))

    def __len__(self):
        return len(self.meshes)

    def move(self, ids, new_poses):
        """vct_objects_update of the objects `ids`; inject and build_mips follow as after voxelize."""
        ids = np.asarray(ids, np.uint32).reshape(-1)
        rec = poses(new_poses)
        self.ctx.objects_update(ids, rec)
        self.poses[ids] = rec

    def stats(self) -> dict:
        return self.ctx.objects_stats()
