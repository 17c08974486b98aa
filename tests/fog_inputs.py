"""The inputs tests/test_fog.py (coverage, on the restatement alone) and tests/test_fog_gpu.py
(parity) share (TEST INFRASTRUCTURE ONLY): the cases, their G-buffers -- cast on the CPU by
scenes.raycast_numpy, so both sides see the same float32 positions -- and the restatement's
results for them, computed once.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import fog_ref as R
import trace_inputs as TI

F = np.float32
Case = namedtuple("Case", "name scene n level step w h eye yaw pitch cam aniso nd ambient density hostile")

EYE_ATRIUM_IN = (0.05, -0.35, 0.7)
CASES = [
    # the eye inside the Cornell box, a camera for the background rays, a hostile row
    Case("cornell_in_l1", "cornell", 32, 1, 1.0, 24, 16, R.EYE_IN, -90.0, 0.0, True, True, 9, 0.0, 2.0, True),
    # the eye outside the grid looking in, no camera (background pixels are null records), dense fog: T stop
    Case("cornell_out_l2", "cornell", 32, 2, 0.25, 33, 17, R.EYE_OUT, -90.0, 0.0, False, True, 9, 0.5, 12.0, False),
    # one pixel, and the ambient K4 launch on the narrowest synthetic frame (m = 4 records wide)
    Case("cornell_one_px_l3", "cornell", 32, 3, 4.0, 1, 1, R.EYE_OUT, -90.0, 0.0, True, True, 9, 0.5, 1.0, False),
    # looking past the box from outside: rays that miss the grid
    Case("cornell_miss_l1", "cornell", 32, 1, 4.0, 24, 16, (3.0, 0.5, 4.0), -60.0, 10.0, True, True, 0, 0.75, 1.0, False),
    Case("atrium_out_l1", "atrium", 32, 1, 1.0, 33, 17, R.EYE_OUT, -90.0, 0.0, True, True, 9, 0.25, 3.0, True),
    Case("atrium_in_l2", "atrium", 32, 2, 0.25, 24, 16, EYE_ATRIUM_IN, -100.0, 15.0, True, True, 0, 0.5, 6.0, False),
    Case("cornell64_iso_l2", "cornell", 64, 2, 1.0, 64, 48, R.EYE_OUT, -90.0, 0.0, True, False, 9, 0.0, 2.0, False),
]
BY_NAME = {c.name: c for c in CASES}


def fog_of(case):
    return R.fog(case.density, (0.9, 0.8, 0.7), case.ambient, case.level, case.step)


def camera(case):
    from vct.camera import Camera
    return Camera(position=case.eye, yaw=case.yaw, pitch=case.pitch)


HOSTILE_CLASSES = ("eye", "nan_x", "nan_y", "nan_z", "posinf", "neginf", "posw", "big", "denorm", "far", "near")


def hostile_class(name):
    """The class of a trace_inputs catalogue entry that a hostile row holds ('eye': P == eye)."""
    if name.startswith("p_nan_"):
        return "nan_" + name[-1]
    for prefix, cls in (("p_posinf", "posinf"), ("p_neginf", "neginf"), ("w_", "posw"), ("pos_big", "big"),
                        ("pos_denorm", "denorm")):
        if name.startswith(prefix):
            return cls
    if name.endswith("_far"):
        return "far"
    return "near"                                   # half a voxel / three voxels outside, the exact-origin pairs


def hostile_entries(g0, E, n):
    """trace_inputs' hostile positions and pos.w values, ordered so that the narrowest hostile row
    (23 entries after P == eye) holds every class: NaN on each axis, +inf, -inf, the hostile
    pos.w values, 1e30, denormal, far outside on every face, then the positions just outside."""
    entries = [e for e in TI.catalogue(g0, E, n)
               if e.family in ("position", "posw") or (e.family == "nonfinite" and e.name.startswith("p_"))]
    rank = {c: i for i, c in enumerate(HOSTILE_CLASSES)}
    return sorted(entries, key=lambda e: rank[hostile_class(e.name)])      # stable: catalogue order inside a class


_hostile = {}


def hostile_row(pos, nrm, alb, g0, E, n, eye):
    """Row 0 of the frame: P == eye, then hostile_entries() in turn.  -> the class of every pixel."""
    entries = hostile_entries(g0, E, n)
    w = pos.shape[1]
    classes = []
    for x in range(w):
        P = np.array([0.1, -0.1, 0.2, 1.0], F)
        N = np.array([0.0, 1.0, 0.0, 0.0], F)
        A = np.array([0.5, 0.5, 0.5, 0.1], F)
        if x == 0:
            P[:3] = np.array(eye, F)
            classes.append("eye")
        else:
            e = entries[(x - 1) % len(entries)]
            e.apply(P, N, A)
            classes.append(hostile_class(e.name))
        pos[0, x], nrm[0, x], alb[0, x] = P, N, A
    return classes


_gb, _ref = {}, {}


def gbuffer(case):
    """(pos4, nrm4, alb4) [h, w, 4] float32 of the case, cast on the CPU."""
    if case.name not in _gb:
        from vct import scenes
        sc = R.scene(case.scene, case.n, case.aniso)
        scene = scenes.cornell() if case.scene == "cornell" else scenes.atrium()
        pos, nrm, alb = (np.ascontiguousarray(a, F).reshape(case.h, case.w, 4)
                         for a in scenes.raycast_numpy(scene, camera(case), case.w, case.h))
        if case.hostile:
            _hostile[case.name] = hostile_row(pos, nrm, alb, sc["g0"], sc["E"], case.n, case.eye)
        for a in (pos, nrm, alb):
            a.setflags(write=False)
        _gb[case.name] = (pos, nrm, alb)
    return _gb[case.name]


def hostile_classes(case):
    """The class of every pixel of the case's hostile row (row 0), [] for a case without one."""
    gbuffer(case)
    return _hostile.get(case.name, [])


def reference(case):
    """The restatement on the case: dict(pos, build, rays, march), the march fed the
    restatement's own volume and rays."""
    if case.name not in _ref:
        sc = R.scene(case.scene, case.n, case.aniso)
        f = fog_of(case)
        pos = gbuffer(case)[0]
        A = None
        if case.ambient > 0:
            A = R.ambient(case.n, sc["g0"], sc["E"], sc["level0"], case.level, case.aniso, case.nd)
        b = R.build(case.n, sc["g0"], sc["E"], sc["alpha"], case.aniso, f, sc["lights"], [R.TAN] * len(sc["lights"]), A)
        ray4 = R.rays(case.n, sc["g0"], sc["E"], case.eye, pos, camera(case) if case.cam else None)
        m = R.march(case.n, sc["g0"], sc["E"], f, case.eye, ray4, b["S"])
        _ref[case.name] = {"pos": pos, "build": b, "rays": ray4, "march": m, "A": A}
    return _ref[case.name]
