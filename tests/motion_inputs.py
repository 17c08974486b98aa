"""Inputs the object-motion tests share (TEST INFRASTRUCTURE): the object sets, the frames, the
transitions a pose goes through between the snapshot and the frame, and the hostile planes.
Static scene: the Cornell box at 16^3, seen from temporal_inputs' CAM_A.

The sets
  catalogue   objects_ref.catalogue(): seven objects, each with the pose that places it
  seventy     70 one-triangle objects in a 10 x 7 array facing the camera: a wave of 64 pixels
              spans more than 64 objects of the index range
  many        4 096 one-triangle objects (VCT_MAX_OBJECTS) in a 64 x 64 array: the search over
              `first` at its full depth
  box         temporal_inputs' moving box as one object, centred on the origin: the temporal tests

A transition is (previous pose, current pose) of one object as functions of its placing matrix;
ROUNDS deals them out so that in round r object k goes through TRANSITIONS[(k + r) % len]: every
round holds every kind, and over the rounds every object goes through every kind.
"""
import numpy as np

import objects_ref as OR
import temporal_inputs as TI

F = np.float32
N = TI.N
FRAMES = TI.FRAMES + ((64, 48),)
ROUGH = 0.1
ANGLE = 40.0                                   # cos 40 = 0.766 < 0.9 = VCT_MIXED_NORMAL_COS
SCALE = (1.5, 0.7, 1.2)


def grid():
    from vct import scenes
    return scenes.grid_for_unit_box(N)


def static_arrays():
    import dynamic_ref
    return dynamic_ref.static_arrays()


def rot_y(deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    return m


def _mat(p):
    """The 4 x 4 matrix of a POSE record, mathematical layout, float64."""
    return np.asarray(p["m"], np.float64).reshape(4, 4).T


def _translate(t):
    m = np.eye(4)
    m[:3, 3] = t
    return m


def _poke(p, slot, value):
    q = p.copy()
    q["m"][slot] = value
    return q


def _pose(m, visible=True):
    return OR.pose(np.asarray(m, np.float64).astype(F), visible)


# name -> (previous pose, current pose) from the placing pose P
TRANSITIONS = (
    ("unmoved", lambda P: P, lambda P: P),
    ("translate", lambda P: P, lambda P: _pose(_translate(TI.BOX_T) @ _mat(P))),
    ("rotate", lambda P: P, lambda P: _pose(_mat(P) @ rot_y(ANGLE))),
    ("scale", lambda P: P, lambda P: _pose(_mat(P) @ np.diag(SCALE + (1.0,)))),
    ("appear", lambda P: _pose(_mat(P), visible=False), lambda P: P),
    ("vanish", lambda P: P, lambda P: _pose(_mat(P), visible=False)),
    ("prev nan", lambda P: _poke(P, 0, np.nan), lambda P: P),
    ("prev inf", lambda P: _poke(P, 13, np.inf), lambda P: P),
    ("minus zero", lambda P: _poke(P, 4, F(-0.0)), lambda P: P),      # equal as numbers, not as bits: moved
    ("unread slot", lambda P: _poke(P, 15, np.nan), lambda P: P),     # m[15] is not read: unmoved
)
ROUNDS = len(TRANSITIONS)


def round_poses(placing, r):
    """(prev, cur) POSE arrays of round r for a set placed by `placing`."""
    prev, cur = [], []
    for k, P in enumerate(placing):
        _, fp, fc = TRANSITIONS[(k + r) % len(TRANSITIONS)]
        prev.append(fp(P))
        cur.append(fc(P))
    return OR.pose_array(prev), OR.pose_array(cur)


def _triangles(nx, ny, lo, hi, z, size):
    """nx x ny one-triangle objects in object space (centred) and the translations that lay them
    out over [lo, hi]^2 at depth z, facing +z."""
    tri = np.array([[-size, -size, 0.0], [size, -size, 0.0], [0.0, size, 0.0]], F)
    meshes, placing = [], []
    for j in range(ny):
        for i in range(nx):
            x = lo + (hi - lo) * (i + 0.5) / nx
            y = lo + (hi - lo) * (j + 0.5) / ny
            meshes.append((tri.copy(), np.arange(3, dtype=np.uint32), np.array([(i + j) % 3], np.uint32)))
            placing.append(OR.pose((x, y, z)))
    return meshes, placing


_sets = {}


def object_set(name):
    """-> (meshes [(verts, idx, tri_material)], placing poses), built once."""
    if name not in _sets:
        if name == "catalogue":
            cat = OR.catalogue()
            _sets[name] = ([cat[k][0] for k in OR.NAMES], [cat[k][1] for k in OR.NAMES])
        elif name == "seventy":
            _sets[name] = _triangles(10, 7, -0.7, 0.7, 0.6, 0.09)
        elif name == "many":
            _sets[name] = _triangles(64, 64, -0.8, 0.8, 0.6, 0.02)
        elif name == "box":
            lo, hi = np.array(TI.BOX_LO, F), np.array(TI.BOX_HI, F)
            c = ((lo + hi) * F(0.5)).astype(F)
            v, i, _, _ = TI.box_arrays()
            v = np.array(v, F, copy=True)
            v[:, :3] -= c
            _sets[name] = ([(v, np.asarray(i, np.uint32), np.zeros(i.size // 3, np.uint32))], [OR.pose(c)])
        else:
            raise KeyError(name)
    return _sets[name]


SETS = ("catalogue", "seventy", "many")


def packed(meshes):
    """The set as the device keeps it: (vpos [V, 3], vidx [3 T] into vpos, first [n_objects + 1])."""
    vs, is_, first, base = [], [], [0], 0
    for m in meshes:
        v = np.asarray(m[0], F)[:, :3]
        vs.append(v)
        is_.append(np.asarray(m[1], np.uint32) + np.uint32(base))
        base += v.shape[0]
        first.append(first[-1] + np.asarray(m[1]).size // 3)
    return (np.concatenate(vs) if vs else np.zeros((0, 3), F), np.concatenate(is_) if is_ else np.zeros(0, np.uint32),
            np.array(first, np.int64))


def n_static():
    return static_arrays()[1].size // 3


_planes = {}


def cpu_planes(name, cur, w, h, cam=None):
    """shading_ref.planes over objects_ref.posed_union of the static scene and set `name` under
    `cur`, with a shading set that has every attribute absent; cached by the poses' bytes."""
    import gbuffer_ref as GR
    import shading_ref as SR
    from vct.shading import ShadingMaterial
    cam = cam or TI.cam_a()
    key = (name, cur.tobytes(), w, h, tuple(cam.position), cam.yaw, cam.pitch)
    if key not in _planes:
        meshes, _ = object_set(name)
        v, i, m, kd = OR.posed_union(static_arrays(), meshes, list(cur))
        g0, E = grid()
        rec = GR.k1_skip(GR.tri_records(v, i), v, i, N, g0, E)
        at = SR.Attrs(n_static(), [ShadingMaterial(roughness=ROUGH)])
        out = SR.planes(rec, kd[m][:, :3].astype(F), cam, w, h, ROUGH, at)
        for a in out.values():
            a.setflags(write=False)
        _planes[key] = out
    return _planes[key]


def hostile_planes(w, h, n_st, n_set, seed=5):
    """Planes no pass writes: ids just inside and outside every range, 0xFFFFFFFF, barycentrics
    that are NaN, infinite, negative or far outside the triangle, background pixels with ids,
    normals that are zero or NaN.  -> dict(pos, nrm, tri_id, bary)."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1, 1, (h, w, 4)).astype(F)
    pos[..., 3] = rng.choice(np.array([0.0, 1.0, -0.0, 2.5], F), (h, w))
    nrm = rng.uniform(-1, 1, (h, w, 4)).astype(F)
    nrm[rng.random((h, w)) < 0.1] = 0
    nrm[rng.random((h, w)) < 0.05] = np.nan
    edge = np.array([0, n_st - 1, n_st, n_st + max(n_set, 1) - 1, n_st + n_set, n_st + n_set + 1, 0x7FFFFFFF, 0x80000000,
                     0xFFFFFFFE, 0xFFFFFFFF], np.int64)
    ids = np.where(rng.random((h, w)) < 0.4, rng.choice(edge, (h, w)), n_st + rng.integers(0, max(n_set, 1), (h, w)))
    bary = rng.uniform(-0.5, 1.5, (h, w, 2)).astype(F)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0], F)
    hit = rng.random((h, w, 2)) < 0.15
    bary[hit] = rng.choice(bad, int(hit.sum()))
    return {"pos": pos, "nrm": nrm, "tri_id": (ids & 0xFFFFFFFF).astype(np.uint32), "bary": bary}
