"""Inputs the temporal-accumulation tests share (TEST INFRASTRUCTURE): the scene, the two
cameras, the frame sizes, the planes and the moving box.  tests/test_temporal.py asserts on the
CPU what the GPU tests rely on: under CAM_A every valid pixel reprojects onto itself, and the
step from CAM_A to CAM_B shows every class of pixel.
"""
import numpy as np

import lights_ref

F = np.float32
N = 16                                   # the Cornell scene's grid
FRAMES = ((1, 1), (13, 7), (32, 24), (33, 23))
COVERED = ((32, 24), (33, 23))           # frames on which the moved camera must show every class
EYE_A = (0.0, 0.0, 2.2)                  # the box fills the frame: CAM_B sees walls CAM_A does not
EYE_B, YAW_B, PITCH_B = (0.2, 0.1, 2.5), -93.0, 2.0
# the moving box: dynamic_ref's `air` box (nothing else is near it), and its translation
BOX_LO, BOX_HI = (-0.3, 0.3, 0.3), (0.0, 0.55, 0.6)
BOX_T = (0.09, -0.05, 0.04)


def cam_a():
    from vct.camera import Camera
    return Camera(position=EYE_A)


def cam_b():
    from vct.camera import Camera
    return Camera(position=EYE_B, yaw=YAW_B, pitch=PITCH_B)


def bad_cameras():
    """(name, VctCamera) for every way prev_cam breaks its rule."""
    out = []
    for field in ("position", "front", "up", "right"):
        for k, v in ((0, float("nan")), (1, float("inf")), (2, float("-inf"))):
            c = cam_a().to_ctypes()
            getattr(c, field)[k] = v
            out.append((f"{field}[{k}] = {v}", c))
    for zoom in (0.0, -0.0, -45.0, 180.0, float("nan"), float("inf")):
        c = cam_a().to_ctypes()
        c.zoom_deg = zoom
        out.append((f"zoom {zoom}", c))
    return out


def plane_eps():
    """One voxel of the scene's grid, the header default."""
    return F(F(lights_ref.cornell(N)["E"]) / F(N))


_gb = {}


def cpu_gbuffer(cam_name, w, h, box_at=None):
    """(pos, nrm, alb) of the Cornell scene under cam_a / cam_b from the CPU caster
    (scenes.raycast_numpy), with the box at BOX_LO + box_at when given; cached."""
    key = (cam_name, w, h, box_at)
    if key not in _gb:
        from vct import scenes
        s = scenes.cornell()
        if box_at is not None:
            lo, hi = (tuple(float(F(a) + F(t)) for a, t in zip(c, box_at)) for c in (BOX_LO, BOX_HI))
            s.box(lo, hi, s.material((0.2, 0.3, 0.9)))
        _gb[key] = scenes.raycast_numpy(s, {"a": cam_a, "b": cam_b}[cam_name](), w, h)
    return _gb[key]


def box_arrays(offset=(0.0, 0.0, 0.0)):
    """The box's mesh for vct_voxelize_dynamic, moved by `offset`."""
    import dynamic_ref
    lo, hi = (tuple(float(F(a) + F(t)) for a, t in zip(c, offset)) for c in (BOX_LO, BOX_HI))
    return dynamic_ref.box(lo, hi)


def planes(seed, w, h, n_planes):
    """n_planes [h][w][4] planes of finite floats of either sign, 0.25 <= |v| < 4."""
    rng = np.random.default_rng(seed)
    return [(rng.uniform(0.25, 4.0, (h, w, 4)) * rng.choice([-1.0, 1.0], (h, w, 4))).astype(F) for _ in range(n_planes)]


def box_motion(pos, offset):
    """motion4 of a frame whose box was moved by `offset` since the last one: pixels on the box
    (position inside its moved bounds, half a voxel of slack) were at P - offset, every other
    pixel where it is.  -> (motion4 [h][w][4] float32, on_box [h][w] bool)."""
    pos = np.ascontiguousarray(pos, F)
    slack = F(0.5) * plane_eps()
    lo = np.array(BOX_LO, F) + np.array(offset, F) - slack
    hi = np.array(BOX_HI, F) + np.array(offset, F) + slack
    on = (pos[..., 3] != 0) & ((pos[..., :3] >= lo) & (pos[..., :3] <= hi)).all(axis=-1)
    m = pos.copy()
    m[..., 3] = 1
    m[on, :3] = pos[on, :3] - np.array(offset, F)
    return m, on
