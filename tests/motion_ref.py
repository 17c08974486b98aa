"""numpy restatement of include/vct_spec.h "object motion" (include/vct_motion.h; TEST
INFRASTRUCTURE).  Every float operation is a float32 numpy operation in the spec's order, fmaf
where the spec writes it (shading_ref.fmaf32), so the GPU kernel is compared with it bit for
bit: motion4, prev_nrm4 and stats.  `T=np.float64` runs the same formulas in float64 (the
float32 inputs taken exactly, fma = a * b + c), for the comparison that does not depend on
float32 rounding.
"""
import numpy as np

from shading_ref import fmaf32

F = np.float32
BACKGROUND, STILL, MOVED, APPEARED = 0, 1, 2, 3       # a pixel's class
WAS_HIDDEN, UNMOVED, OBJECT_MOVED = 0, 1, 2           # an object's flag
READ = (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14)      # the twelve floats the transform rule reads


def object_flags(cur, prev):
    """Per object: hidden in the snapshot, unmoved (the twelve floats bitwise equal) or moved."""
    cm = np.ascontiguousarray(cur["m"], F).view(np.uint32)[:, READ]
    pm = np.ascontiguousarray(prev["m"], F).view(np.uint32)[:, READ]
    same = (cm == pm).all(axis=1)
    return np.where(prev["visible"] == 0, WAS_HIDDEN, np.where(same, UNMOVED, OBJECT_MOVED))


def object_of(first, t):
    """The last object o with first[o] <= t (first: [n_objects + 1])."""
    return np.searchsorted(np.asarray(first[:-1], np.int64), np.asarray(t, np.int64), side="right") - 1


def _xform(T, v, m):
    """The transform rule per pixel: v [k, 3] object-space vertices, m [k, 16] matrices."""
    v, m = v.astype(T), m.astype(T)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((m[:, r] * x + m[:, 4 + r] * y) + m[:, 8 + r] * z) + m[:, 12 + r] for r in range(3)], -1)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _face_unit(p):
    """unit((p1 - p0) x (p2 - p0)) per pixel, and where unit() is defined; p: 3 x [k, 3]."""
    with np.errstate(all="ignore"):
        e1, e2 = p[1] - p[0], p[2] - p[0]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1)
        sq = _dot3(n, n)
        return n / np.sqrt(sq)[:, None], np.isfinite(sq) & (sq > 0)


def moved_terms(T, tri, bary, nrm, vpos, vidx, m_prev, m_cur):
    """The `else` case of the rule for k pixels on moved objects: tri [k] the set's triangle,
    bary [k, 2], nrm [k, 4] or None, m_prev / m_cur [k, 16].  -> (q [k, 3], n_prev [k, 3] (flipped
    as written) or None, ok [k]: both unit() defined), in number format T."""
    fma = fmaf32 if T is F else (lambda a, b, c: a * b + c)
    v = [np.asarray(vpos, F)[np.asarray(vidx, np.int64).reshape(-1, 3)[tri, j]] for j in range(3)]
    p = [_xform(T, v[j], m_prev) for j in range(3)]
    b1, b2 = bary[:, 0].astype(T)[:, None], bary[:, 1].astype(T)[:, None]
    with np.errstate(all="ignore"):
        q = np.asarray(fma(b2, p[2] - p[0], fma(b1, p[1] - p[0], p[0])), T)
    if nrm is None:
        return q, None, None
    n_prev, okp = _face_unit(p)
    n_cur, okc = _face_unit([_xform(T, v[j], m_cur) for j in range(3)])
    with np.errstate(all="ignore"):
        flip = _dot3(n_cur, nrm[:, :3].astype(T)) < 0
    return q, np.where(flip[:, None], -n_prev, n_prev), okp & okc


def motion(pos, nrm, tri_id, bary, n_static, first, vpos, vidx, cur, prev):
    """vct_objects_motion_device.  pos, nrm [h, w, 4] (nrm None: no prev_nrm4), tri_id [h, w]
    uint32, bary [h, w, 2]; first [n_objects + 1]; vpos [V, 3] / vidx [3 T]: the set's packed
    object-space mesh; cur / prev: POSE arrays.  -> dict(motion [h, w, 4], prev_nrm [h, w, 4] or
    None, stats (valid, static_or_unmoved, moved, appeared), cls [h, w], obj [h, w] (-1: none))."""
    pos = np.ascontiguousarray(pos, F)
    h, w = pos.shape[:2]
    tri_id = np.ascontiguousarray(tri_id).view(np.uint32).reshape(h, w).astype(np.int64)
    bary = np.ascontiguousarray(bary, F).reshape(h, w, 2)
    n_set = int(first[-1])
    valid = pos[..., 3] != 0
    M = np.zeros((h, w, 4), F)
    M[valid, :3] = pos[valid, :3]
    M[valid, 3] = 1
    Q = None
    if nrm is not None:
        nrm = np.ascontiguousarray(nrm, F)
        Q = np.where(valid[..., None], nrm, F(0)).astype(F)
    cls = np.where(valid, STILL, BACKGROUND).astype(np.int8)
    obj = np.full((h, w), -1, np.int64)
    nowhere = valid & (tri_id >= n_static + n_set)
    inset = valid & (tri_id >= n_static) & ~nowhere
    t = np.where(inset, tri_id - n_static, 0)
    obj[inset] = object_of(first, t[inset])
    flags = object_flags(cur, prev)
    flag = np.where(inset, flags[np.where(inset, obj, 0)], UNMOVED)
    gone = nowhere | (inset & (flag == WAS_HIDDEN))
    mv = inset & (flag == OBJECT_MOVED)
    if mv.any():
        o = obj[mv]
        q, n_prev, ok = moved_terms(F, t[mv], bary[mv], None if nrm is None else nrm[mv], vpos, vidx,
                                    np.asarray(prev["m"], F)[o], np.asarray(cur["m"], F)[o])
        fin = np.isfinite(q).all(axis=1)
        rec = np.concatenate([q, np.ones((q.shape[0], 1), F)], -1).astype(F)
        rec[~fin] = 0
        M[mv] = rec
        c = cls[mv]
        c[:] = np.where(fin, MOVED, APPEARED)
        cls[mv] = c
        if nrm is not None:
            qn = Q[mv]
            qn[ok] = np.concatenate([n_prev[ok], np.zeros((int(ok.sum()), 1), F)], -1).astype(F)
            Q[mv] = qn
    M[gone] = 0
    cls[gone] = APPEARED
    n = lambda v: int((cls == v).sum())
    stats = (int(valid.sum()), n(STILL), n(MOVED), n(APPEARED))
    assert stats[0] == sum(stats[1:])
    return {"motion": M, "prev_nrm": Q, "stats": stats, "cls": cls, "obj": obj}


def check_args(width, height, n_prev, n_objects, has_nrm, has_prev_nrm):
    """The host rule apart from pointers: None, or what is wrong."""
    if width == 0 or height == 0 or width > 65536 or height > 65536 or width * height > 0x7FFFFFFF:
        return "bad frame size"
    if has_nrm != has_prev_nrm:
        return "nrm4 and prev_nrm4 go together"
    if n_prev != n_objects:
        return "n_prev != n_objects"
    return None
